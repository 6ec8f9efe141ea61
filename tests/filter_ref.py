"""FindIDsByFilter restated in plain Python (pkg/core/core.go:1766-1839; evaluateBooleanFilter :1900-2034; findFilterOperator
:1866-1897) over {id: {key: value}} plus a deleted set -- the reference the device filter (filter.hip) and kdb_filter_parse are
pinned to.  It follows the pattern of consensus_ref.py: the reference's own control flow, line for line, no shortcuts.

The metadata model is AddMetadataUnlocked's (:1640-1758): a string goes to the inverted index under its own text, a bool under
"true" / "false", a float (int) to the B-tree; VDelete removes a node's metadata (pkg/engine/ops.go:428), so a deleted id is in
no index, and `!=` starts from the non-deleted nodes (GetAllValidNodeIDs, hnsw_index.go:2884-2900).
"""
import math
import re

# regexp `(?i)\\s+OR\\s+` / `(?i)\\s+AND\\s+` (core.go:44,48); RE2's \\s is [\\t\\n\\f\\r ]
_OR = re.compile(r"[\t\n\f\r ]+[oO][rR][\t\n\f\r ]+")
_AND = re.compile(r"[\t\n\f\r ]+[aA][nN][dD][\t\n\f\r ]+")
_TRIM = " \t\n\v\f\r"  # strings.TrimSpace, ASCII part
# strconv.ParseFloat(s, 64) without an error: decimal or hexadecimal (p exponent required) floats, inf / infinity / nan
_DEC = re.compile(r"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?\Z")
_HEX = re.compile(r"[+-]?0[xX](?:[0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)[pP][+-]?[0-9]+\Z")
_SPECIAL = re.compile(r"[+-]?(?:inf|infinity|nan)\Z", re.I)


class FilterError(ValueError):
    pass


def parse_float(s):
    """the float64 ParseFloat returns, or None where it returns an error (syntax, or a value out of range)"""
    if _SPECIAL.match(s):
        return float(s)
    if _DEC.match(s):
        v = float(s)
    elif _HEX.match(s):
        try:
            v = float.fromhex(s)
        except OverflowError:
            return None
    else:
        return None
    return None if math.isinf(v) else v


def find_filter_operator(f):
    in_single = in_double = False
    for i, c in enumerate(f):
        if c == "'":
            if not in_double:
                in_single = not in_single
            continue
        if c == '"':
            if not in_single:
                in_double = not in_double
            continue
        if in_single or in_double:
            continue
        if f[i:i + 2] in ("!=", "<=", ">="):
            return f[i:i + 2], i
        if c in "=<>":
            return c, i
    return "", -1


def parse(filter_str):
    """The atoms FindIDsByFilter would evaluate, in order, as kdb_filter_parse reports them:
    [{key, value, op, is_numeric, number, end_block}]; FilterError where the reference returns an error (and for a NaN operand,
    which the device path refuses)."""
    f = filter_str.strip(_TRIM)
    if f == "":
        raise FilterError("empty filter")
    atoms = []
    for block in _OR.split(f):
        block = block.strip(_TRIM)
        if block == "":
            continue
        n_in_block = 0
        for sub in _AND.split(block):
            sub = sub.strip(_TRIM)
            if sub == "":
                continue
            op, at = find_filter_operator(sub)
            if at == -1:
                raise FilterError("invalid filter format")
            key = sub[:at].strip(_TRIM)
            value = sub[at + len(op):].strip(_TRIM).strip("'\"")
            num = parse_float(value)
            if num is not None and math.isnan(num):
                raise FilterError("NaN operand")
            if op in ("<", "<=", ">", ">=") and num is None:
                raise FilterError("value must be numeric for operator '%s'" % op)
            atoms.append({"key": key, "value": value, "op": op, "is_numeric": num is not None, "number": 0.0 if num is None else num,
                          "end_block": False})
            n_in_block += 1
        if n_in_block:
            atoms[-1]["end_block"] = True
    return atoms


class MetaDB:
    """docs: {internal id: {key: str | bool | int | float}}; deleted: ids whose node is soft-deleted (their metadata is gone)."""

    def __init__(self, docs, deleted=()):
        self.deleted = set(deleted)
        self.ids = sorted(docs)
        self.inv = {}    # key -> value text -> set(ids)      (invertedIndex)
        self.btree = {}  # key -> [(float64, id)]             (bTreeIndex)
        for i, meta in docs.items():
            if i in self.deleted:
                continue
            for k, v in meta.items():
                if isinstance(v, bool):
                    self.inv.setdefault(k, {}).setdefault("true" if v else "false", set()).add(i)
                elif isinstance(v, str):
                    self.inv.setdefault(k, {}).setdefault(v, set()).add(i)
                elif isinstance(v, (int, float)):
                    self.btree.setdefault(k, []).append((float(v), i))

    def all_valid(self):
        return {i for i in self.ids if i not in self.deleted}

    def evaluate(self, sub):
        sub = sub.strip(_TRIM)
        op, at = find_filter_operator(sub)
        if at == -1:
            raise FilterError("invalid filter format")
        key = sub[:at].strip(_TRIM)
        value = sub[at + len(op):].strip(_TRIM).strip("'\"")
        num = parse_float(value)
        if num is not None and math.isnan(num):
            raise FilterError("NaN operand")
        if op in ("=", "!="):
            matched = set()
            if num is not None and key in self.btree:
                matched |= {i for x, i in self.btree[key] if x == num}
            matched |= self.inv.get(key, {}).get(value, set())
            return matched if op == "=" else self.all_valid() - matched
        if num is None:
            raise FilterError("value must be numeric for operator '%s'" % op)
        items = self.btree.get(key, [])
        if op == "<":
            return {i for x, i in items if x < num}
        if op == "<=":
            return {i for x, i in items if x <= num}
        if op == ">":
            return {i for x, i in items if x > num}
        return {i for x, i in items if x >= num}

    def find_ids(self, filter_str):
        f = filter_str.strip(_TRIM)
        if f == "":
            raise FilterError("empty filter")
        final = set()
        for block in _OR.split(f):
            block = block.strip(_TRIM)
            if block == "":
                continue
            cur = None
            for sub in _AND.split(block):
                sub = sub.strip(_TRIM)
                if sub == "":
                    continue
                s = self.evaluate(sub)
                cur = set(s) if cur is None else cur & s
                if not cur:
                    break
            if cur is None:
                continue
            final |= cur
        return final


def bitset(ids, words):
    """an id set as the dense list the device writes: `words` uint64 words, bit id"""
    import numpy as np
    w = np.zeros(words, dtype=np.uint64)
    a = np.fromiter(ids, dtype=np.uint64, count=len(ids))
    if a.size:
        np.bitwise_or.at(w, (a >> np.uint64(6)).astype(np.int64), np.uint64(1) << (a & np.uint64(63)))
    return w


def run_program(terms, cells):
    """kdb_filter_plan.h's kdb_filter_run in Python: terms = [(op, flags, col, code, value)], cells[col] = the id's value
    (float, NaN = absent, for a numeric column; int code, 0 = absent, for a code column).  Without the AND with live."""
    prog, block, clause, inv, first = False, True, False, False, True
    for op, flags, col, code, value in terms:
        if op == 6:
            v = cells[col] == code
        elif op == 0:
            v = False
        else:
            x = cells[col]
            v = {1: x == value, 2: x < value, 3: x <= value, 4: x > value, 5: x >= value}[op]
        if first:
            clause, inv = v, bool(flags & 2)
        else:
            clause = clause or v
        first = False
        if not flags & 1:
            block = block and (clause != inv)
            first = True
            if flags & 4:
                prog = prog or block
                block = True
    return prog
