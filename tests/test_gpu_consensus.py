"""kdb_consensus_batch[_dev] / kdb_belief_batch[_dev] (consensus.hip): CalculateConsensus on the device for id lists.

The bars, against the numpy restatement (tests/consensus_ref.py) of the rows kdb_index_decode_rows gives:
  * bit for bit: n_found, n_active, the centroid, every entry of out_gram (the float64 accumulators: dots, squared norms, dots
    against the centroid, the zeroed rows of entries that are not active) and the -1.0 markers of out_similarity;
  * absolute 2^-46 (1.4e-14): similarities, variance, max_pair.  The accumulators are exact; what remains is one sqrt product, one
    divide and a sum of at most 64 squares of values in [0, 1] -- a few 1e-15 -- and the bound also covers a device sqrt or divide
    that is one ulp off;
  * absolute 1e-10: the score, on lists whose reference maxVar >= 0.05 (decided on the reference side; the test asserts that these
    are at least nine in ten of its lists of more than one node): the error is at most dvar / maxVar^2 + 2 dmax / maxVar, about 6e-12
    there.  A short list whose two or three nodes lie closer together than that is held to the same propagation with its own
    maxVar.  On the all-duplicates list the score is exactly 1.0.
Indexes for the consensus call alone hold rows only (no graph): 600 rows, 5 % deleted.  The belief call is a composition: its search
half must equal kdb_search_batch (ids, distance bits, counts, trace, counters), its consensus half kdb_consensus_batch on those
outputs, bit for bit (the same kernel on the same inputs)."""
import functools
import json
import os
import threading

import numpy as np
import pytest

from consensus_ref import restate, same
from test_gpu_refine import Case  # noqa: F401  (the graphs of the belief tests: cases A and D, through test_gpu_search_by_id.setup)

pytestmark = pytest.mark.gpu

L2, COSINE = 0, 1
F32, F16, I8 = 0, 1, 2
NOPE = 0xffffffff
TIED = 0x80000000
TOL = 2.0 ** -46
N = 600
NAN_ID, ZERO_ID = 77, 78          # float32 indexes: a row holding a NaN, a zero row; no other list draws them
COUNTS = [10, 0, 1, 2, 3, 50, 64]
SPECS = {"f32_3": (F32, 3), "f32_100": (F32, 100), "f32_772": (F32, 772), "f32_768": (F32, 768), "f32_1536": (F32, 1536),
         "f16_72": (F16, 72), "i8_100": (I8, 100)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Rows:
    """one rows-only index and the host copy of its decoded rows"""

    def __init__(self, name):
        import kektordb_amd as hip
        prec, dim = SPECS[name]
        rng = np.random.default_rng(1000 + dim + prec)
        self.name, self.prec, self.dim = name, prec, dim
        idx = self.idx = hip.HipIndex(dim, COSINE if prec == I8 or dim in (3, 768) else L2, prec, 8, 40, capacity=N + 8)
        x = rng.standard_normal((N, dim)).astype(np.float32)
        x[1::2] += np.float32(2.0) * x[0::2]                     # correlated neighbours: pair distances off the clamp as well
        if prec == F32:
            x[NAN_ID - 1, min(1, dim - 1)] = np.nan
            x[ZERO_ID - 1] = 0.0
            idx.upload_rows(x, 1)
        elif prec == F16:
            idx.upload_rows(x.astype(np.float16).view(np.uint16), 1)
        else:
            amax = float(np.abs(x).max())                        # Quantizer.Train's AbsMax, then Quantize
            idx.set_quantizer(amax)
            idx.upload_rows(np.clip(np.rint(x / np.float32(amax) * np.float32(127.0)), -127, 127).astype(np.int8), 1)
        idx.set_count(N)
        self.dead = rng.choice(np.arange(21, N + 1), N // 20, replace=False).astype(np.uint32)
        self.dead = self.dead[(self.dead != NAN_ID) & (self.dead != ZERO_ID)]
        idx.Delete(self.dead)
        self.deleted = np.zeros(N + 1, dtype=bool)
        self.deleted[self.dead] = True
        wide, found = idx.decode_rows(np.arange(N + 1, dtype=np.uint32))         # kdb_index_decode_rows: what a node's vector IS
        assert np.array_equal(found, ~self.deleted & (np.arange(N + 1) > 0))
        self.wide = wide
        self.pool = np.array([i for i in range(21, N + 1) if i not in (NAN_ID, ZERO_ID)], dtype=np.uint32)   # deleted ids included
        # active mask: about a third of the ids cleared; ids 1..10 all cleared, of 11..20 only 15 set
        act = rng.random(N + 1) >= 1.0 / 3.0
        act[1:11] = False
        act[11:21] = False
        act[15] = True
        self.act = act
        self.act_bits = np.zeros((N >> 6) + 1, dtype=np.uint64)
        for i in np.nonzero(act)[0]:
            self.act_bits[i >> 6] |= np.uint64(1) << np.uint64(i & 63)

    def found(self, ids):
        ids = np.asarray(ids, dtype=np.int64)
        ok = (ids >= 1) & (ids <= N)
        ok[ok] = ~self.deleted[ids[ok]]
        return ok

    def lists(self, B, seed, stride=64):
        """B lists: counts cycle through COUNTS; lists of 10 or more hold a deleted id, 0, count + 1, 0xffffffff and a repeat; with
        B >= 7 list 0 has no active node under the mask and list 4 exactly one; odd lists carry bit 31 in their count"""
        rng = np.random.default_rng(seed)
        ids = rng.choice(self.pool, (B, stride)).astype(np.uint32)
        cnt = np.array([COUNTS[b % 7] for b in range(B)], dtype=np.uint32)
        for b in range(B):
            c = int(cnt[b])
            if c >= 10:
                pos = rng.choice(c, 6, replace=False)
                ids[b, pos[:5]] = [int(self.dead[b % len(self.dead)]), 0, N + 1, NOPE, ids[b, pos[5]]]
            elif c >= 2 and b % 2:
                ids[b, 0] = [0, int(self.dead[0]), N + 1, NOPE][(b // 7) % 4]
        if B >= 7:
            ids[0, :10] = np.arange(1, 11)
            ids[4, :3] = [11, 15, 12]
        cnt[1::2] |= np.uint32(TIED)
        return ids, cnt

    def want(self, ids, cnt, Q, masked):
        B, S = ids.shape
        ok = self.found(ids) & (np.arange(S)[None, :] < (cnt & 0x7fffffff)[:, None])
        safe = np.where(ok, ids, 0).astype(np.int64)
        active = self.act[safe] if masked else np.ones((B, S), dtype=bool)
        return restate(self.wide[safe], ok, active, Q)


@functools.lru_cache(maxsize=None)
def rows_of(name):
    return Rows(name)


def near(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and bool(np.all(np.abs(a[~na] - b[~nb]) <= tol))


def same_where_not_nan(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint8), b[~nb].view(np.uint8))


def check(got, want, eq=same, score_rows=None, tag=None):
    """the bars of the module docstring; eq: the bit-for-bit comparison"""
    g, w = got["rec"], want["rec"]
    print(tag, "max |d similarity|", np.nanmax(np.abs(got["similarity"] - want["similarity"]), initial=0.0),
          "max |d variance|", np.nanmax(np.abs(g["variance"] - w["variance"]), initial=0.0),
          "max |d max_pair|", np.nanmax(np.abs(g["max_pair"] - w["max_pair"]), initial=0.0),
          "max |d score|", np.nanmax(np.abs(g["score"] - w["score"]), initial=0.0))
    assert np.array_equal(g["n_found"], w["n_found"]) and np.array_equal(g["n_active"], w["n_active"]), tag
    assert eq(got["centroid"], want["centroid"]), tag
    assert eq(got["gram"], want["gram"]), tag
    miss = want["similarity"] == -1.0
    assert np.array_equal(got["similarity"] == -1.0, miss), tag
    assert near(got["similarity"], want["similarity"], TOL), tag
    assert near(g["variance"], w["variance"], TOL) and near(g["max_pair"], w["max_pair"], TOL), tag
    rows = np.ones(len(w), dtype=bool) if score_rows is None else score_rows
    many = w["n_active"] > 1
    big = rows & many & (w["max_pair"] >= 0.05)                 # decided on the reference side
    assert big.sum() * 10 >= (rows & many).sum() * 9, tag       # ... which holds for (nearly) every list of more than one node
    assert near(g["score"][big | (rows & ~many)], w["score"][big | (rows & ~many)], 1e-10), tag
    # the few short lists whose nodes all lie close together (two or three points in three dimensions): the same error
    # propagation with their own maxVar, dvar / maxVar^2 + 2 dmax var / maxVar^3 with dvar = dmax = 2^-46
    for b in np.nonzero(rows & many & ~big & (w["max_pair"] >= 1e-6))[0]:
        mv, var = float(w["max_pair"][b]), float(w["variance"][b])
        assert abs(float(g["score"][b]) - float(w["score"][b])) <= TOL / mv ** 2 + 2.0 * TOL * var / mv ** 3, (tag, b)
    assert (g["score"][w["n_active"] == 0] == 0.0).all() and (g["score"][w["n_active"] == 1] == 1.0).all()


PLAN = [(name, B) for name in SPECS for B in (1, 7, 300) if B < 300 or SPECS[name][1] <= 100]


@pytest.mark.parametrize("name,B", PLAN)
def test_consensus_equals_the_restatement(name, B):
    R = rows_of(name)
    ids, cnt = R.lists(B, seed=B)
    Q = np.random.default_rng(B + 1).standard_normal((B, R.dim)).astype(np.float32)
    for masked in (False, True):
        got = R.idx.consensus(ids, cnt, Q, R.act_bits if masked else None, want_centroid=True, want_gram=True)
        want = R.want(ids, cnt, Q, masked)
        check(got, want, tag=(name, B, masked))
        if masked and B >= 7:
            assert got["rec"]["n_active"][0] == 0 and got["rec"]["n_found"][0] == 10 and not got["centroid"][0].any() and not got["gram"][0].any()
            assert got["rec"]["n_active"][4] == 1 and same(got["centroid"][4], R.wide[15])
            assert (got["similarity"][0, :10] != -1.0).all()     # historical nodes still get a similarity
    assert (got["rec"]["n_found"] < (cnt & 0x7fffffff)).any() or B == 1
    # counts == NULL: every list has `stride` entries; queries == NULL: no similarities
    s = 13
    got = R.idx.consensus(ids[:, :s], None, None, None, want_centroid=True, want_gram=True)
    want = R.want(ids[:, :s], np.full(B, s, dtype=np.uint32), None, False)
    assert got["similarity"] is None
    got["similarity"] = want["similarity"]
    check(got, want, tag=(name, B, "full lists"))


@pytest.mark.parametrize("name", ["f32_100", "f16_72", "i8_100", "f32_1536"])
def test_dev_form_on_a_side_stream_equals_the_host_form(name):
    import torch
    R = rows_of(name)
    B, S = 7, 64
    ids, cnt = R.lists(B, seed=3)
    Q = np.random.default_rng(4).standard_normal((B, R.dim)).astype(np.float32)
    host = R.idx.consensus(ids, cnt, Q, R.act_bits, want_centroid=True, want_gram=True)
    d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
    d_cnt = torch.from_numpy(cnt.view(np.int32)).cuda()
    d_q = torch.from_numpy(Q).cuda()
    d_act = torch.from_numpy(R.act_bits.view(np.int64)).cuda()
    d_out = torch.full((B, 32), 0xee, dtype=torch.uint8, device="cuda")
    d_sim = torch.full((B, S), 7.0, dtype=torch.float64, device="cuda")
    d_cen = torch.full((B, R.dim), 7.0, dtype=torch.float32, device="cuda")
    d_gram = torch.full((B, S + 1, S + 1), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    R.idx.consensus_dev(d_ids, d_out, d_cnt, d_q, d_act, d_sim, d_cen, d_gram, stream=side.cuda_stream)
    side.synchronize()
    from kektordb_amd.index import CONSENSUS_DTYPE
    assert same(d_out.cpu().numpy().view(CONSENSUS_DTYPE).ravel(), host["rec"])
    assert same(d_sim.cpu().numpy(), host["similarity"]) and same(d_cen.cpu().numpy(), host["centroid"]) and same(d_gram.cpu().numpy(), host["gram"])


def test_special_lists_nan_zero_row_and_duplicates():
    R = rows_of("f32_100")
    ids, cnt = R.lists(7, seed=9)
    cnt &= np.uint32(0x7fffffff)
    ids[2, :6], cnt[2] = [30, NAN_ID, 31, 32, 33, 34], 6         # the row holding a NaN
    ids[3, :5], cnt[3] = [40, 40, 40, 40, 40], 5                 # duplicates only
    ids[6, :7], cnt[6] = [50, ZERO_ID, 51, 52, 53, 54, 55], 7    # a zero row: distance 1 to everything
    for i in (30, 31, 32, 33, 34, 40, 50, 51, 52, 53, 54, 55):
        assert not R.deleted[i]
    Q = np.random.default_rng(10).standard_normal((7, R.dim)).astype(np.float32)
    got = R.idx.consensus(ids, cnt, Q, None, want_centroid=True, want_gram=True)
    want = R.want(ids, cnt, Q, False)
    plain = np.array([True, True, False, False, True, True, True])
    check(got, want, eq=same_where_not_nan, score_rows=plain, tag="special")
    assert np.isnan(want["rec"]["variance"][2]) and np.isnan(want["similarity"][2, 1]) and np.isnan(want["rec"]["score"][2])
    assert np.isnan(got["rec"]["score"][2]) and not np.isnan(got["rec"]["max_pair"][2])      # `d > maxVar` is false for a NaN
    assert np.isnan(got["centroid"][2]).sum() == 1 and not np.isnan(np.delete(got["similarity"][2], 1)).any()
    assert got["rec"]["score"][3] == 1.0 and want["rec"]["score"][3] == 1.0 and got["rec"]["max_pair"][3] < 1e-10
    # the other lists of the batch are bit for bit as alone
    for b in (0, 1, 3, 4, 5, 6):
        alone = R.idx.consensus(ids[b:b + 1], cnt[b:b + 1], Q[b:b + 1], None, want_centroid=True, want_gram=True)
        for f in ("rec", "similarity", "centroid", "gram"):
            assert same(alone[f][0], got[f][b]), (b, f)


def test_reference_kats_on_the_device():
    import kektordb_amd as hip
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "consensus_kats.json")))
    idx = hip.HipIndex(3, COSINE, F32, 8, 40, capacity=8)
    idx.upload_rows(np.eye(3, dtype=np.float32), 1)
    idx.set_count(3)
    for c in kats["cases"]:
        v = np.array(c["vectors"], dtype=np.float32).reshape(len(c["vectors"]), 3)
        ids = np.zeros((1, 3), dtype=np.uint32)
        ids[0, :len(v)] = [1 + int(np.argmax(r)) for r in v]     # every KAT vector is a unit vector: a row of the identity
        assert same(np.eye(3, dtype=np.float32)[ids[0, :len(v)] - 1], v)
        got = idx.consensus(ids, np.array([len(v)], dtype=np.uint32))["rec"]
        score, var = float(got["score"][0]), float(got["variance"][0])
        if c["should_be_near"]:
            assert 0.0 <= score <= 1.0
        else:
            assert abs(score - c["expected_score"]) <= kats["tolerance"] and abs(var - c["expected_variance"]) <= kats["tolerance"], (c["name"], score, var)
    idx.Close()


def test_invalid_arguments(hip):
    R = rows_of("f32_100")
    idx = R.idx
    ids = np.ones((2, 65), dtype=np.uint32)
    with pytest.raises(hip.KdbError, match=r"status -1"):
        idx.consensus(ids)                                       # stride 65
    with pytest.raises(hip.KdbError, match=r"status -1"):
        idx.consensus(ids[:, :10], np.array([3, 11], dtype=np.uint32))   # a count above the stride
    with pytest.raises(hip.KdbError, match=r"status -1"):
        idx.consensus(ids[:, :10], np.array([3, 11 | TIED], dtype=np.uint32))
    with pytest.raises(hip.KdbError, match=r"status -1"):
        idx.consensus(ids[:, :10], flags=1)
    from kektordb_amd.index import CONSENSUS_DTYPE, _ptr
    rec = np.zeros(2, dtype=CONSENSUS_DTYPE)
    rec["score"] = 5.0
    sim = np.full((2, 10), 5.0)
    a = np.ascontiguousarray(ids[:, :10])
    assert idx.L.kdb_consensus_batch(idx.h, _ptr(a), None, 2, 10, None, None, 0, _ptr(rec), _ptr(sim), None, None) == -1   # similarities without queries
    assert (rec["score"] == 5.0).all() and (sim == 5.0).all()    # nothing was launched
    q = np.zeros((2, R.dim), dtype=np.float32)
    for k in (0, 65):
        with pytest.raises(hip.KdbError, match=r"status -1"):
            idx.belief(q, k)
    out = idx.consensus(np.zeros((0, 10), dtype=np.uint32))      # B == 0
    assert out["rec"].shape == (0,)


# ---- belief = search, then consensus ---------------------------------------------------------------------------------------------
def ctr(idx):
    c = idx.counters()
    return c["n_dist"], c["n_hops"], c["n_tied"], c["n_dropped"]


def test_belief_without_similarities_host_form_equals_dev_form():
    """out_similarity == NULL (the Python wrapper always asks for the similarities): the host-pointer call against the _dev call on
    the same inputs, bit for bit, with and without the allow list and the active list; the records equal those of the call that
    does return similarities"""
    import torch
    from test_gpu_search_by_id import setup
    from kektordb_amd.index import CONSENSUS_DTYPE, _ptr
    S = setup("A")
    idx = S.idx
    B, k, ef = 5, 4, 100
    d64 = S.prec == I8
    flags = idx._by_id_flags(False, d64, False, False)
    Q = np.ascontiguousarray(belief_queries(S, 47)[:B])
    act = np.full((S.n >> 6) + 1, 0x6db6db6db6db6db6, dtype=np.uint64)      # two ids of three active
    even = np.ascontiguousarray(S.even, dtype=np.uint64)
    d_q = torch.from_numpy(Q).cuda()
    for allow, active in ((None, None), (even, None), (None, act), (even, act)):
        ids = np.zeros((B, k), dtype=np.uint32)
        dist = np.full((B, k), np.inf, dtype=np.float64 if d64 else np.float32)
        cnt = np.zeros(B, dtype=np.uint32)
        rec = np.zeros(B, dtype=CONSENSUS_DTYPE)
        assert idx.L.kdb_belief_batch(idx.h, _ptr(Q), B, k, ef, _ptr(allow), _ptr(active), flags, _ptr(ids), _ptr(dist), _ptr(cnt), _ptr(rec), None) == 0
        oi = torch.full((B, k), -1, dtype=torch.int32, device="cuda")
        od = torch.full((B, k), -7.0, dtype=torch.float64 if d64 else torch.float32, device="cuda")
        oc = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        orec = torch.zeros((B, 32), dtype=torch.uint8, device="cuda")
        d_al = None if allow is None else torch.from_numpy(allow.view(np.int64)).cuda()
        d_act = None if active is None else torch.from_numpy(active.view(np.int64)).cuda()
        torch.cuda.synchronize()
        idx.belief_dev(d_q, k, ef, oi, od, oc, orec, None, d_al, d_act, dist64=d64)
        idx.sync()
        tag = (allow is not None, active is not None)
        assert same(oi.cpu().numpy().view(np.uint32), ids) and same(od.cpu().numpy(), dist) and same(oc.cpu().numpy().view(np.uint32), cnt), tag
        assert same(orec.cpu().numpy().view(CONSENSUS_DTYPE).ravel(), rec), tag
        full = idx.belief(Q, k, ef, allow, active, dist64=d64)
        assert same(full[0], ids) and same(full[1], dist) and same(full[2], cnt) and same(full[3], rec), tag
        assert (cnt > 0).all() and (active is None or (rec["n_active"] < rec["n_found"]).any()), tag


def belief_queries(S, seed):
    rng = np.random.default_rng(seed)
    return (S.wide[rng.choice(S.live, 203, replace=False)] + np.float32(0.05) * rng.standard_normal((203, S.dim)).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("name", ["A", "D"])
def test_belief_is_search_then_consensus(name):
    import torch
    from test_gpu_search_by_id import setup
    from kektordb_amd.index import CONSENSUS_DTYPE
    S = setup(name)
    idx = S.idx
    Q = belief_queries(S, 31)
    act = np.zeros((S.n >> 6) + 1, dtype=np.uint64)
    for i in range(1, S.n + 1):
        if i % 3:
            act[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    d64 = S.prec == I8
    for k in (1, 10, 50):
        for allow in (None, S.even):
            wi, wd, wc, (wnd, wnh) = idx.search_batch(Q, k, 100, allow, trace=True, dist64=d64)
            want_ctr = ctr(idx)
            gi, gd, gc, rec, sim, (gnd, gnh) = idx.belief(Q, k, 100, allow, None, trace=True, dist64=d64)
            assert ctr(idx) == want_ctr, (name, k)
            assert same(gi, wi) and same(gd, wd) and same(gc, wc) and same(gnd, wnd) and same(gnh, wnh), (name, k, allow is not None)
            alone = idx.consensus(wi, wc, Q, None)
            assert same(rec, alone["rec"]) and same(sim, alone["similarity"]), (name, k, allow is not None)
            assert (rec["n_found"] == (wc & 0x7fffffff)).all() and (wc > 0).all()
            if k == 10:                                          # historical nodes; the _dev form on a side stream
                gi, gd, gc, rec, sim = idx.belief(Q, k, 100, allow, act, dist64=d64)
                alone = idx.consensus(wi, wc, Q, act)
                assert same(gi, wi) and same(gd, wd) and same(gc, wc) and same(rec, alone["rec"]) and same(sim, alone["similarity"])
                assert (rec["n_active"] < rec["n_found"]).any()
                d_q = torch.from_numpy(Q).cuda()
                oi = torch.full((203, k), -1, dtype=torch.int32, device="cuda")
                od = torch.full((203, k), -7.0, dtype=torch.float64 if d64 else torch.float32, device="cuda")
                oc = torch.full((203,), -1, dtype=torch.int32, device="cuda")
                orec = torch.zeros((203, 32), dtype=torch.uint8, device="cuda")
                osim = torch.full((203, k), 7.0, dtype=torch.float64, device="cuda")
                d_al = None if allow is None else torch.from_numpy(allow.view(np.int64)).cuda()
                d_act = torch.from_numpy(act.view(np.int64)).cuda()
                torch.cuda.synchronize()
                side = torch.cuda.Stream()
                idx.belief_dev(d_q, k, 100, oi, od, oc, orec, osim, d_al, d_act, stream=side.cuda_stream, dist64=d64)
                side.synchronize()
                assert same(oi.cpu().numpy().view(np.uint32), wi) and same(od.cpu().numpy(), wd) and same(oc.cpu().numpy().view(np.uint32), wc)
                assert same(orec.cpu().numpy().view(CONSENSUS_DTYPE).ravel(), alone["rec"]) and same(osim.cpu().numpy(), alone["similarity"])
    # against the restatement as well: the decoded rows of the ids the search returned
    ok = S.found(wi) & (np.arange(wi.shape[1])[None, :] < (wc & 0x7fffffff)[:, None])
    want = restate(S.wide[np.where(ok, wi, 0).astype(np.int64)], ok, np.ones_like(ok), Q)
    got = idx.consensus(wi, wc, Q, None, want_centroid=True, want_gram=True)
    assert same(got["centroid"], want["centroid"]) and same(got["gram"], want["gram"])
    assert near(got["similarity"], want["similarity"], TOL) and near(got["rec"]["variance"], want["rec"]["variance"], TOL)
    # BeliefState of the mirror class: k capped at 50, None where the reference returns an error
    bs = idx.BeliefState(Q[0], 70)
    r50 = idx.belief(Q[:1], 50, 100, dist64=d64)
    assert bs["sources"] == int(r50[3]["n_found"][0]) == len(bs["nodes"]) and bs["score"] == float(r50[3]["score"][0])
    assert bs["variance"] == float(r50[3]["variance"][0]) and bs["similarities"] == r50[4][0, :len(bs["nodes"])].tolist()
    ref = idx.SearchWithScores(Q[0], 50, efSearch=100)
    assert [r.DocID for r in bs["nodes"]] == [r.DocID for r in ref] and len(bs["similarities"]) == len(ref)
    assert idx.BeliefState(Q[0], 10, allowList=np.zeros((S.n >> 6) + 1, dtype=np.uint64)) is None      # no candidates


def test_concurrent_belief_and_search_callers_on_one_handle():
    from test_gpu_search_by_id import setup
    S = setup("A")
    idx = S.idx
    k, ef, calls = 10, 100, 60
    rng = np.random.default_rng(8)
    q_sets = [(S.wide[rng.choice(S.live, 5, replace=False)] + np.float32(0.01)).astype(np.float32) for _ in range(8)]
    want_b = [idx.belief(q, k, ef) for q in q_sets]
    want_q = [idx.search_batch(q, k, ef) for q in q_sets]
    bad = []

    def belief(t):
        for it in range(calls):
            j = (t + it) % 8
            got = idx.belief(q_sets[j], k, ef)
            if not all(same(a, b) for a, b in zip(got, want_b[j])):
                bad.append(("belief", t, it))

    def by_query(t):
        for it in range(calls):
            j = (t + it) % 8
            got = idx.search_batch(q_sets[j], k, ef)
            if not all(same(a, b) for a, b in zip(got, want_q[j])):
                bad.append(("query", t, it))

    th = [threading.Thread(target=belief, args=(t,)) for t in range(4)] + [threading.Thread(target=by_query, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad, bad[:5]
