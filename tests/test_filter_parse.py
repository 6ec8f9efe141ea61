"""The filter string without a GPU: the plain-Python restatement of FindIDsByFilter (tests/filter_ref.py) reproduces the reference's
own filter tests (tests/golden/filter_kats.json), kdb_filter_parse -- through ctypes -- returns the atoms the restatement's parser
returns, compile_filter's programs evaluate (kdb_filter_run restated) to the restatement's id sets, and the new entry points refuse
bad arguments before they look for a device."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import filter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "filter_kats.json")))
OPS = {0: "=", 1: "!=", 2: "<", 3: "<=", 4: ">", 5: ">="}

EXTRA = [
    'tag = "a<=b"',                                    # operators inside quotes
    "tag = 'x>=1' AND v >= \"2\"",
    "a=1 and\tb=2 Or  c=3\tAND\td=4",                   # mixed case, tabs
    "a=1 OR AND AND",
    'age = "10"',                                      # numeric-looking string: both alternatives
    "age=10",
    "name = '\"quoted\"'",                             # values wrapped in mixed quotes
    "name=\"'x'\"\"",
    "name = 'O'Brien'",
    "a=1 OR",
    "a=1 AND ",
    "  x<1e3  ",
    "x<=-0.0 OR x>=+.5 OR x>0x1p-2",
    "x = 1_0",                                         # underscores: a string, not a number
    "x = ' 10'",                                       # blank inside the quotes: a string
    "x = 1e999",                                       # out of range: ParseFloat's error, a string
    "x = inf",
    "a=1 ORb=2",                                       # no split: one atom whose value holds the rest
    "a=1  OR  OR b=2",
    "k==v",
    "k=!v",
    "x !=",
]
ERRORS = ["", "   \t ", "no-operator-here", "x < abc", "x >= '1_0'", "x = nan", "x < NaN", "x != -nan", "OR AND", " OR "]


@pytest.fixture(scope="module")
def K():
    import kektordb_amd
    kektordb_amd.build_library()
    return kektordb_amd


def all_kat_filters():
    out = [c["filter"] for s in KATS["sets"] for c in s["cases"]]
    out += [c["filter"] for c in KATS["find_operator"]] + KATS["malformed_no_panic"]["filters"]
    return out


def test_restatement_reproduces_every_kat():
    for s in KATS["sets"]:
        ids = {d["name"]: i + 1 for i, d in enumerate(s["docs"])}
        for c in s["cases"]:
            db = R.MetaDB({i + 1: d["meta"] for i, d in enumerate(s["docs"][:c["n_docs"]])})
            got = db.find_ids(c["filter"])
            if "expected" in c:
                assert got == {ids[n] for n in c["expected"]}, (c, got)
            for n in c.get("includes", []):
                assert ids[n] in got, (c, got)
            for n in c.get("excludes", []):
                assert ids[n] not in got, (c, got)
    for c in KATS["find_operator"]:
        assert R.find_filter_operator(c["filter"]) == (c["op"], c["index"]), c
    db = R.MetaDB({1: KATS["malformed_no_panic"]["docs"][0]["meta"]})
    for f in KATS["malformed_no_panic"]["filters"]:  # the reference's test: no panic -- a set or an error
        try:
            assert isinstance(db.find_ids(f), set)
        except R.FilterError:
            pass


def same_atoms(K, f):
    from kektordb_amd.index import parse_filter
    try:
        want = R.parse(f)
    except R.FilterError:
        want = None
    try:
        got = parse_filter(f)
    except K.KdbError as e:
        assert "status -1" in str(e), e
        got = None
    if want is None or got is None:
        assert want is None and got is None, (f, want, got)
        return None
    assert len(got) == len(want), (f, got, want)
    for g, w in zip(got, want):
        assert (g["key"], g["value"], OPS[g["op"]], g["is_numeric"], g["end_block"]) == (w["key"], w["value"], w["op"], w["is_numeric"], w["end_block"]), (f, g, w)
        assert np.float64(g["number"]).tobytes() == np.float64(w["number"]).tobytes(), (f, g, w)  # bit for bit, -0.0 included
    return got


def test_parse_matches_the_restatement(K):
    n_ok = 0
    for f in all_kat_filters() + EXTRA + ERRORS:
        n_ok += same_atoms(K, f) is not None
    assert n_ok >= len(EXTRA) - 1
    for f in ERRORS:
        with pytest.raises(R.FilterError):
            R.parse(f)
    # the three error cases and the NaN operand, by message
    lib = K.load()
    n = C.c_uint32()
    for f, word in ((b"", b"empty filter"), (b"abc", b"invalid filter format"), (b"x < abc", b"numeric"), (b"x = NaN", b"NaN")):
        assert lib.kdb_filter_parse(f, None, 0, C.byref(n)) == -1
        assert word in lib.kdb_last_error(), (f, lib.kdb_last_error())
    # details the issue names
    a = same_atoms(K, 'age = "10"')[0]
    assert a["is_numeric"] and a["number"] == 10.0 and a["value"] == "10"
    a = same_atoms(K, 'tag = "a<=b"')[0]
    assert (a["key"], a["value"], a["op"]) == ("tag", "a<=b", 0)
    a = same_atoms(K, "a=1 and\tb=2 Or  c=3\tAND\td=4")
    assert [(x["key"], x["end_block"]) for x in a] == [("a", False), ("b", True), ("c", False), ("d", True)]
    assert same_atoms(K, "name = '\"quoted\"'")[0]["value"] == "quoted"
    # count first, then fill: a short buffer receives a prefix, n_atoms the total
    from kektordb_amd import _lib
    buf = (_lib.FilterAtom * 1)()
    assert lib.kdb_filter_parse(b"a=1 AND b=2 OR c=3", C.cast(buf, C.c_void_p), 1, C.byref(n)) == 0 and n.value == 3
    assert lib.kdb_filter_parse(None, None, 0, C.byref(n)) == -1 and lib.kdb_filter_parse(b"a=1", None, 0, None) == -1


def schema_of(docs):
    """key -> slots and dictionary, columns as arrays indexed by id: what a mirror keeps"""
    keys = sorted({k for m in docs.values() for k in m})
    schema, cols, slot = {}, {}, 0
    n = max(docs) + 1
    for k in keys:
        vals = {i: m[k] for i, m in docs.items() if k in m}
        ent = {"f64": None, "code": None, "dict": {}}
        if any(isinstance(v, (int, float)) and not isinstance(v, bool) for v in vals.values()):
            ent["f64"] = slot
            col = np.full(n, np.nan)
            for i, v in vals.items():
                if isinstance(v, (int, float)) and not isinstance(v, bool):
                    col[i] = float(v)
            cols[slot] = col
            slot += 1
        strs = {i: ("true" if v else "false") if isinstance(v, bool) else v for i, v in vals.items() if isinstance(v, (bool, str))}
        if strs:
            ent["code"] = slot
            for s in sorted(set(strs.values())):
                ent["dict"][s] = len(ent["dict"]) + 1
            col = np.zeros(n, dtype=np.uint32)
            for i, s in strs.items():
                col[i] = ent["dict"][s]
            cols[slot] = col
            slot += 1
        schema[k] = ent
    return schema, cols


def test_compiled_programs_evaluate_to_the_restatement(K):
    """compile_filter + kdb_filter_run (restated in filter_ref.run_program) == FindIDsByFilter, on every KAT and on documents that
    carry one key as a number in some nodes and as a string in others (the lenient union)"""
    from kektordb_amd.index import compile_filter
    sets = [({i + 1: d["meta"] for i, d in enumerate(s["docs"])}, [c["filter"] for c in s["cases"]]) for s in KATS["sets"]]
    mixed = {1: {"age": 10.0}, 2: {"age": "10"}, 3: {"age": "ten", "ok": True}, 4: {"ok": False, "age": -0.0}, 5: {}, 6: {"age": 11}}
    sets.append((mixed, ['age = "10"', "age=10", "age!=10", "age != '10' AND ok='true'", "age<11 OR ok!=false", "age=0", "nokey=1", "nokey!=1",
                         "nokey<3 OR age>=11", "age>=10 AND age<=10", "ok=true OR ok=false"]))
    for docs, filters in sets:
        for deleted in (set(), {2}):
            db = R.MetaDB(docs, deleted)
            schema, cols = schema_of(docs)
            for f in filters:
                prog = compile_filter(f, schema)
                terms = [(int(t["op"]), int(t["flags"]), int(t["col"]), int(t["code"]), float(t["value"])) for t in prog]
                got = {i for i in docs if i not in deleted and R.run_program(terms, {c: col[i] for c, col in cols.items()})}
                # a deleted node has no metadata in the reference; the device ANDs with live instead -- the same set
                assert got == db.find_ids(f), (f, deleted, got, db.find_ids(f))


def test_argument_validation_without_a_device(K):
    """the precedence of kdb_search_by_id: the handle, then B == 0, then the buffers -- all before any device call"""
    lib = K.load()
    from kektordb_amd import _lib
    t = (_lib.FilterTerm * 1)()
    offs = (C.c_uint32 * 2)(0, 1)
    assert lib.kdb_index_set_column(None, 0, 1, 1, 1, None) == -1 and b"null index" in lib.kdb_last_error()
    assert lib.kdb_index_set_column_dev(None, 0, 1, 1, 1, None) == -1
    assert lib.kdb_index_drop_column(None, 0) == -1
    assert lib.kdb_index_column_info(None, 0, None, None) == -1
    assert lib.kdb_filter_eval(None, t, offs, 1, None, 1, None) == -1 and b"null index" in lib.kdb_last_error()
    assert lib.kdb_filter_eval_dev(None, t, offs, 1, None, 1, None, None) == -1
    assert lib.kdb_search_filtered(None, None, 1, 1, 1, t, offs, 1, None, 0.1, 0, None, None, None, None, None) == -1
    assert b"null index" in lib.kdb_last_error()
    assert C.sizeof(_lib.FilterTerm) == 16 and C.sizeof(_lib.FilterAtom) == 32
    from kektordb_amd.index import TERM_DTYPE
    assert TERM_DTYPE.itemsize == 16
