"""Allow lists built on the device (kdb_index_set_column, kdb_filter_eval[_dev]; filter.hip): device lists and cardinalities against
tests/filter_ref.py -- the plain-Python FindIDsByFilter -- turned into bitsets.  Sets are compared exactly, word for word: bit 0,
the bits above count and the padding words included (the output is pre-filled with 0xFF so that a word nobody wrote shows).

The synthetic table: an F64 column with 30 % absent rows, the others drawn from {-1, -0.0, 0.0, 1, 0.1, float32(0.1), 16777216,
16777217} (the last pairs catch a compare done in single precision), a code column with codes 0..5 (0 = absent), 10 % deleted ids.
Programs are written as filter STRINGS, compiled by compile_filter and evaluated by the restatement from the same documents; a
64-term program and the raw flag shapes the strings cannot express are built term by term and evaluated by filter_ref.run_program."""
import json
import os

import numpy as np
import pytest

import filter_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "filter_kats.json")))
VALUES = [-1.0, -0.0, 0.0, 1.0, 0.1, float(np.float32(0.1)), 16777216.0, 16777217.0]
NAMES = ["", "a", "b", "c", "d", "e"]          # code -> string of the code column "cat"
SCHEMA = {"x": {"f64": 0, "code": None, "dict": {}}, "cat": {"f64": None, "code": 3, "dict": {s: c for c, s in enumerate(NAMES) if c}}}
FILTERS = [
    "x=1", "x<0.1", "x<=0.1", "x>0.1", "x>=0.1", "x=0", "x=-0.0", "x=16777217", "x>16777216", "x<=16777216", "x=0.10000000149011612",
    "cat=a", "cat='e'", "cat=zz", "nokey=1", "x!=1", "cat!=b", "nokey!=1",
    "x>=0 AND cat=c", "x<0 OR cat=d", "x>=-1 AND x<=1 AND cat!=a OR cat=a AND x>1", "cat=a OR cat=b OR cat=c OR cat=d OR cat=e",
    "x<-5", "x!=12345", "cat!=a AND cat!=b AND x!=0.1 OR x=0.1",
]


def table(count, seed=5):
    rng = np.random.default_rng(seed)
    x = np.full(count + 1, np.nan)
    have = rng.random(count + 1) >= 0.3
    x[have] = rng.choice(VALUES, int(have.sum()))
    code = rng.integers(0, 6, count + 1).astype(np.uint32)
    x[0], code[0] = 1.0, 1                      # id 0 names nobody, whatever the columns hold there
    dead = set(rng.choice(np.arange(1, count + 1), count // 10, replace=False).tolist()) if count >= 10 else set()
    docs = {}
    for i in range(1, count + 1):
        m = {}
        if not np.isnan(x[i]):
            m["x"] = float(x[i])
        if code[i]:
            m["cat"] = NAMES[code[i]]
        docs[i] = m
    return x, code, dead, docs


def make_index(hip, count, cap, x, code, dead):
    idx = hip.HipIndex(16, 0, 0, 8, 20, capacity=cap)
    idx.set_count(count)
    if dead:
        idx.Delete(sorted(dead))
    idx.set_column(0, 1, x[1:], 1)              # COL_F64 in slot 0
    idx.set_column(3, 2, code[1:], 1)           # COL_CODE in slot 3
    return idx


def eval_dev(idx, programs, words):
    import torch
    P = len(programs)
    d_lists = torch.full((P, words), -1, dtype=torch.int64, device="cuda")   # 0xFF in every byte
    d_card = torch.full((P,), 12345, dtype=torch.int32, device="cuda")
    idx.filter_eval_dev(programs, d_lists, d_card)
    idx.sync()
    return d_lists.cpu().numpy().view(np.uint64), d_card.cpu().numpy().view(np.uint32)


def check(lists, card, want_sets, words, count):
    for p, want in enumerate(want_sets):
        assert not want or (min(want) >= 1 and max(want) <= count)
        assert np.array_equal(lists[p], R.bitset(want, words)), (p, sorted(want)[:10], words, count)
        assert int(card[p]) == len(want), (p, card[p], len(want))


@pytest.fixture(scope="module")
def big(hip):
    """the 10 000-id table, its index (capacity above count) and the restatement: made once, never modified"""
    count = 10000
    x, code, dead, docs = table(count)
    idx = make_index(hip, count, count + 77, x, code, dead)
    db = R.MetaDB(docs, dead)
    return {"count": count, "x": x, "code": code, "dead": dead, "docs": docs, "db": db, "idx": idx, "want": {f: db.find_ids(f) for f in FILTERS}}


def test_kats_on_the_device(hip):
    from kektordb_amd.index import compile_filter
    from test_filter_parse import schema_of
    for s in KATS["sets"]:
        docs = {i + 1: d["meta"] for i, d in enumerate(s["docs"])}
        schema, cols = schema_of(docs)
        n = len(docs)
        idx = hip.HipIndex(16, 0, 0, 8, 20, capacity=n + 3)
        for slot, col in cols.items():
            idx.set_column(slot, 1 if col.dtype == np.float64 else 2, col[1:], 1)
        for c in s["cases"]:                    # the reference ran each case when only n_docs documents existed
            idx.set_count(c["n_docs"])
            db = R.MetaDB({i: m for i, m in docs.items() if i <= c["n_docs"]})
            words = (c["n_docs"] >> 6) + 1
            lists, card = eval_dev(idx, [compile_filter(c["filter"], schema)], words)
            want = db.find_ids(c["filter"])
            check(lists, card, [want], words, c["n_docs"])
            names = {d["name"]: i + 1 for i, d in enumerate(s["docs"])}
            if "expected" in c:
                assert want == {names[x] for x in c["expected"]}
        idx.set_count(n)                        # the host-output form, every document present
        f0 = s["cases"][0]["filter"]
        h_lists, h_card = idx.filter_eval([compile_filter(f0, schema)])
        check(h_lists, h_card, [R.MetaDB(docs).find_ids(f0)], (n >> 6) + 1, n)
        idx.close()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 1023, 1024, 1025, 10000])
def test_counts_and_padding(hip, count, big):
    """every size at which the tiling changes (one wave covers 1024 ids), capacity above count, words_per_list at the minimum and
    at minimum + 3; bit 0 and the bits above count are clear because the WHOLE buffer equals the restatement's bitset"""
    from kektordb_amd.index import compile_filter
    if count == 10000:
        idx, db = big["idx"], big["db"]
    else:
        x, code, dead, docs = table(count, seed=count)
        idx, db = make_index(hip, count, count + 130, x, code, dead), R.MetaDB(docs, dead)
    progs = [compile_filter(f, SCHEMA) for f in FILTERS]
    want = [big["want"][f] for f in FILTERS] if count == 10000 else [db.find_ids(f) for f in FILTERS]
    for extra in (0, 3):
        words = (count >> 6) + 1 + extra
        lists, card = eval_dev(idx, progs, words)
        check(lists, card, want, words, count)
        assert not (lists[:, 0] & np.uint64(1)).any()
    everything = {i for i in range(1, count + 1)} - (big["dead"] if count == 10000 else dead)
    assert want[FILTERS.index("x!=12345")] == everything and want[FILTERS.index("x<-5")] == set()
    if count != 10000:
        idx.close()


@pytest.mark.parametrize("P", [1, 2, 31, 32, 33, 130])
def test_program_counts(hip, big, P):
    """P around the chunk of 32 programs that share a column fetch, and several chunks"""
    from kektordb_amd.index import compile_filter
    fs = [FILTERS[(7 * p + P) % len(FILTERS)] for p in range(P)]
    words = (big["count"] >> 6) + 1
    lists, card = eval_dev(big["idx"], [compile_filter(f, SCHEMA) for f in fs], words)
    check(lists, card, [big["want"][f] for f in fs], words, big["count"])


def test_raw_programs(hip, big):
    """what strings do not express: every op in one 64-term program, NOT on a two-alternative clause over two columns, a clause of
    NEVERs, and the host-output form with and without lists"""
    from kektordb_amd.index import TERM_DTYPE
    E, O, N = 4, 1, 2
    long_prog = []
    for i in range(64):   # 32 blocks of (x <op> v AND code == c), op and constants cycling through every op and value
        if i % 2 == 0:
            long_prog.append((1 + (i // 2) % 5, 0, 0, 0, VALUES[(i // 2) % len(VALUES)]))
        else:
            long_prog.append((6, E, 3, 1 + (i // 2) % 5, 0.0))
    progs = [
        long_prog,
        [(1, O | N, 0, 0, 1.0), (6, E, 3, 2, 0.0)],                       # NOT (x == 1 OR cat == b)
        [(0, O, 0, 0, 0.0), (0, E, 0, 0, 0.0)],                          # nothing
        [(0, N | E, 0, 0, 0.0)],                                         # everything live
        [(6, N, 3, 1, 0.0), (5, E, 0, 0, 0.0), (2, O, 0, 0, -0.5), (6, E, 3, 5, 0.0)],   # (NOT a AND x >= 0) OR (x < -0.5 OR e)
    ]
    arr = [np.array(p, dtype=TERM_DTYPE) for p in progs]
    count, x, code, dead = big["count"], big["x"], big["code"], big["dead"]
    want = [{i for i in range(1, count + 1) if i not in dead and R.run_program(p, {0: x[i], 3: int(code[i])})} for p in progs]
    assert want[2] == set() and len(want[3]) == count - len(dead) and 0 < len(want[0]) < count
    words = (count >> 6) + 1
    lists, card = eval_dev(big["idx"], arr, words)
    check(lists, card, want, words, count)
    h_lists, h_card = big["idx"].filter_eval(arr, words + 3)
    check(h_lists, h_card, want, words + 3, count)
    none, only_card = big["idx"].filter_eval(arr, want_lists=False)
    assert none is None and np.array_equal(only_card, h_card)
    # ... and lists without cardinalities (out_card == NULL; the Python wrapper always asks for them): bit for bit the _dev lists
    from kektordb_amd.index import _ptr, pack_programs
    terms, offs = pack_programs(arr)
    only_lists = np.full((len(arr), words), 0xee, dtype=np.uint64)
    assert big["idx"].L.kdb_filter_eval(big["idx"].h, _ptr(terms), _ptr(offs), len(arr), _ptr(only_lists), words, None) == 0
    assert np.array_equal(only_lists, lists)


def test_many_columns_per_chunk(hip):
    """a chunk that reads more than 4 columns goes through its tile 8 words at a time, more than 8 columns 4 words at a time: three
    chunks that read 10, 5 and 1 columns, on a count whose last tile is partial and whose padding ends inside a pass"""
    from kektordb_amd.index import TERM_DTYPE
    count = 1500
    rng = np.random.default_rng(31)
    dead = set(rng.choice(np.arange(1, count + 1), count // 10, replace=False).tolist())
    idx = hip.HipIndex(16, 0, 0, 8, 20, capacity=count + 40)
    idx.set_count(count)
    idx.Delete(sorted(dead))
    cols, kinds = {}, {}
    for slot in (0, 2, 3, 5, 6, 8, 9, 12, 13, 15):           # ten live slots, numeric and code columns alternating
        if slot % 2 == 0:
            col = np.full(count + 1, np.nan)
            have = rng.random(count + 1) >= 0.3
            col[have] = rng.choice(VALUES, int(have.sum()))
            kinds[slot] = 1
        else:
            col = rng.integers(0, 4, count + 1).astype(np.uint32)
            kinds[slot] = 2
        cols[slot] = col
        idx.set_column(slot, kinds[slot], col[1:], 1)
    slots = sorted(cols)

    def term(slot, i, flags):
        return (1 + i % 5, flags, slot, 0, VALUES[i % len(VALUES)]) if kinds[slot] == 1 else (6, flags, slot, 1 + i % 3, 0.0)

    progs = []
    for p in range(32):      # chunk 0: all ten columns -- each program ORs one term per column, every other one under NOT
        use = [slots[(p + i) % 10] for i in range(1 + p % 10)]
        progs.append([term(s_, p + i, (2 if i == 0 and p % 2 else 0) | (1 if i + 1 < len(use) else 4)) for i, s_ in enumerate(use)])
    for p in range(32):      # chunk 1: five columns, ANDed blocks
        use = [slots[(p + i) % 5] for i in range(1 + p % 5)]
        progs.append([term(s_, p + i, 4 if i + 1 == len(use) else 0) for i, s_ in enumerate(use)])
    for p in range(7):       # chunk 2: one column
        progs.append([term(15, p, 4)])
    want = [{i for i in range(1, count + 1) if i not in dead and R.run_program(p, {s_: (cols[s_][i] if kinds[s_] == 1 else int(cols[s_][i])) for s_ in slots})}
            for p in progs]
    assert sum(1 for w in want if 0 < len(w) < count - len(dead)) > 40
    arr = [np.array(p, dtype=TERM_DTYPE) for p in progs]
    for extra in (0, 3):
        words = (count >> 6) + 1 + extra
        lists, card = eval_dev(idx, arr, words)
        check(lists, card, want, words, count)
    idx.close()


def test_refusals(hip, big):
    from kektordb_amd.index import TERM_DTYPE
    idx = big["idx"]
    bad = [
        [(1, 0, 0, 0, 1.0)],                       # no END_BLOCK
        [(1, 4, 1, 0, 1.0)],                       # slot 1 is empty
        [(1, 4, 3, 0, 1.0)],                       # slot 3 holds codes
        [(6, 4, 0, 1, 0.0)],                       # slot 0 holds numbers
        [(7, 4, 0, 0, 0.0)],                       # no such op
        [(1, 4, 0, 0, float("nan"))],              # NaN operand
        [(0, 0, 0, 0, 0.0)] * 64 + [(0, 4, 0, 0, 0.0)],   # 65 terms
    ]
    for p in bad:
        with pytest.raises(hip.KdbError, match="status -1"):
            idx.filter_eval([np.array(p, dtype=TERM_DTYPE)])
    ok = np.array([(0, 4, 0, 0, 0.0)], dtype=TERM_DTYPE)
    with pytest.raises(hip.KdbError, match="status -1"):
        idx.filter_eval([ok], words_per_list=(big["count"] >> 6))          # one word short
    with pytest.raises(hip.KdbError, match="status -1"):
        idx.set_column(0, 2, np.ones(3, dtype=np.uint32), 1)                # the slot holds the other kind
    with pytest.raises(hip.KdbError, match="status -1"):
        idx.set_column(16, 1, np.ones(3), 1)
    with pytest.raises(hip.KdbError, match="status -1"):
        idx.set_column(5, 1, np.array([1.0, np.inf]), 1)                    # JSON carries no infinity
    assert idx.column_info(5) == (0, 0)                                      # ... and the refusal allocated nothing
    with pytest.raises(hip.KdbError, match="status -1"):
        idx.set_column(0, 1, np.ones(2), big["count"] + 77)                 # past the capacity
    assert idx.column_info(0) == (1, (big["count"] + 78) * 8) and idx.column_info(3) == (2, (big["count"] + 78) * 4)


def test_partial_update_reserve_compress_drop(hip):
    """n = 1 mid-range changes exactly that id; after kdb_index_reserve old ids evaluate as before and new ids are absent; after
    kdb_index_compress the new index evaluates identically; a dropped slot is refused"""
    from kektordb_amd.index import compile_filter
    count = 1500
    x, code, dead, docs = table(count, seed=77)
    idx = hip.HipIndex(16, 0, 0, 8, 20, capacity=count + 5)
    idx.upload_rows(np.random.default_rng(1).random((count, 16), dtype=np.float32), 1)   # (compress wants rows)
    idx.set_count(count)
    idx.Delete(sorted(dead))
    idx.set_column(0, 1, x[1:], 1)
    idx.set_column(3, 2, code[1:], 1)
    fs = ["x=1", "cat=a", "x!=1 AND cat!=a", "x>=0"]
    progs = [compile_filter(f, SCHEMA) for f in fs]
    words = (count >> 6) + 1
    before, _ = eval_dev(idx, progs, words)
    check(before, _, [R.MetaDB(docs, dead).find_ids(f) for f in fs], words, count)
    # VSetMetadata: one id, both columns
    victim = next(i for i in range(700, 800) if i not in dead and docs[i].get("x", -1.0) >= 0 and docs[i]["x"] != 1.0 and docs[i].get("cat") != "a")
    idx.set_column(0, 1, np.array([1.0]), victim)
    idx.set_column(3, 2, np.array([1], dtype=np.uint32), victim)
    docs[victim] = {"x": 1.0, "cat": "a"}
    after, card = eval_dev(idx, progs, words)
    check(after, card, [R.MetaDB(docs, dead).find_ids(f) for f in fs], words, count)
    diff = before ^ after
    assert all(int(diff[p, victim >> 6]) == 1 << (victim & 63) for p in range(3)) and int(np.count_nonzero(diff)) == 3
    # reserve: the columns move; ids above the old capacity are absent (NaN / code 0), not zero
    idx.reserve(4000)
    assert idx.column_info(0) == (1, 4001 * 8) and idx.column_info(3) == (2, 4001 * 4) and idx.column_info(1) == (0, 0)
    idx.set_count(3000)
    words2 = (3000 >> 6) + 1
    grown, card2 = eval_dev(idx, progs + [compile_filter("x=0", SCHEMA), compile_filter("x!=0", SCHEMA)], words2)
    db = R.MetaDB({**docs, **{i: {} for i in range(count + 1, 3001)}}, dead)
    check(grown, card2, [db.find_ids(f) for f in fs + ["x=0", "x!=0"]], words2, 3000)
    assert np.array_equal(grown[:4, :words - 1], after[:, :words - 1])
    idx.set_count(count)
    # compress: same ids, same capacity, columns copied on the device
    for prec in (1,):
        new = idx.Compress(prec)
        assert new.column_info(0) == (1, 4001 * 8) and new.column_info(3) == (2, 4001 * 4)
        got, card3 = eval_dev(new, progs, words)
        assert np.array_equal(got, after) and np.array_equal(card3, card)
        new.close()
    idx.drop_column(3)
    assert idx.column_info(3) == (0, 0)
    with pytest.raises(hip.KdbError, match="status -1"):
        idx.filter_eval([progs[1]])
    lists, _ = idx.filter_eval([progs[0]])
    assert np.array_equal(lists[0], after[0])
    idx.close()


def test_dev_form_feeds_a_search_on_the_same_stream(hip, oracle):
    """kdb_filter_eval_dev on a non-default stream, then kdb_search_batch_multi_dev on the same stream with no host synchronisation
    in between: the answers of the host-list path (search_batch with the restatement's bitset)"""
    import torch
    from kektordb_amd.index import compile_filter
    O = oracle
    n, dim, k, ef = 2000, 16, 5, 40
    rng = np.random.default_rng(7)
    X = rng.random((n, dim), dtype=np.float32)
    o = O.OracleIndex(dim, O.L2, O.F32, 8, 20, seed=3)
    o.add_many(X)
    idx = hip.HipIndex(dim, 0, 0, 8, 20, capacity=n + 9)
    idx.upload_rows(o.rows()[1:], 1)
    idx.upload_graph_obj(o.export_graph())
    x, code, dead, docs = table(n, seed=3)
    idx.Delete(sorted(dead))
    idx.set_column(0, 1, x[1:], 1)
    idx.set_column(3, 2, code[1:], 1)
    fs = ["cat=a OR cat=b OR x>=1", "x!=1", "x<-5"]
    progs = [compile_filter(f, SCHEMA) for f in fs]
    db = R.MetaDB(docs, dead)
    Q = rng.random((48, dim), dtype=np.float32)
    of_q = np.array([(b % 4) - 1 for b in range(48)], dtype=np.int32)          # -1 = no filter
    words = (n >> 6) + 1
    side = torch.cuda.Stream()
    d_q = torch.from_numpy(Q).cuda()
    d_of = torch.from_numpy(of_q).cuda()
    d_lists = torch.full((3, words), -1, dtype=torch.int64, device="cuda")
    oi = torch.zeros((48, k), dtype=torch.int32, device="cuda")
    od = torch.zeros((48, k), dtype=torch.float32, device="cuda")
    oc = torch.zeros(48, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    idx.filter_eval_dev(progs, d_lists, None, stream=side.cuda_stream)
    idx.search_batch_multi_dev(d_q, k, ef, d_lists, d_of, oi, od, oc, stream=side.cuda_stream)
    side.synchronize()
    ids, dist, cnt = oi.cpu().numpy().view(np.uint32), od.cpu().numpy(), oc.cpu().numpy().view(np.uint32)
    for g in (-1, 0, 1, 2):
        sel = np.nonzero(of_q == g)[0]
        allow = None if g < 0 else R.bitset(db.find_ids(fs[g]), words)
        wi, wd, wc = idx.search_batch(Q[sel], k, ef, allow_bits=allow)
        assert np.array_equal(cnt[sel], wc)
        for j, b in enumerate(sel):
            c = int(wc[j])
            assert np.array_equal(ids[b, :c], wi[j, :c]) and np.array_equal(dist[b, :c].view(np.uint32), wd[j, :c].view(np.uint32))
        if g == 2:
            assert not cnt[sel].any()
    idx.close()
