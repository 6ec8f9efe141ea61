"""The oracle's candidate-heap peak (OracleIndex.last_peak_candidates, oracle/kdb_oracle.c search_layer) against a heapq restatement of
the walk, on the CPU: the GPU tests of the heap-order walk's HBM tail (tests/test_gpu_heap_tail.py) decide from this figure which
queries reach the tail and which overflow, so the figure itself is pinned here.

Random rows without duplicates (heapq orders equal distances by id, the reference by the history of its heaps: where no two
candidates in play are at one distance the two pop in the same order), 96 % and 50 % of the nodes below the top level soft-deleted,
squared L2 and cosine.  The restatement must first
reproduce the oracle's ids, n_dist and n_hops query for query -- only then does its peak say anything -- and then its largest
level-0 candidate-heap length must be the oracle's."""
import numpy as np
import pytest

import heap_tail_ref as R

K = 10


@pytest.mark.parametrize("metric,share,ef", [(R.L2, 0.96, 60), (R.L2, 0.96, 10), (R.COSINE, 0.96, 200), (R.L2, 0.5, 60)])
def test_peak_candidates_is_the_restated_walks(oracle, metric, share, ef):
    c = R.TailCorpus(oracle, 1500, 32, metric, R.F32, share, seed=11, dups=False)
    assert c.deleted.size >= int(share * 1400)
    peaks = []
    for b in range(R.NQ):
        oi, od, (ond, onh), peak = c.want(K, ef)[b]
        r = R.restated_walk(c, b, K, ef)
        assert r is not None
        assert r[0] == [int(x) for x in oi] and (r[1], r[2]) == (ond, onh), (b, r[:3], oi, ond, onh)
        assert r[4] == peak, (b, r[4], peak)
        peaks.append(peak)
    # the figure is a search's own: a handle that searched something else in between answers for that search
    oi, od = c.orc.search(c.Q[0], 1, ef=1)
    assert c.orc.last_peak_candidates() <= peaks[0]
    c.orc.search(c.Q[0], K, ef=ef)
    assert c.orc.last_peak_candidates() == peaks[0]


def test_peak_candidates_of_an_empty_index_and_k_zero(oracle):
    orc = oracle.OracleIndex(8, R.L2, R.F32, 4, 10, seed=1)
    assert orc.last_peak_candidates() == 0
    orc.search(np.zeros(8, np.float32), 3)
    assert orc.last_peak_candidates() == 0
    orc.add_many(np.eye(8, dtype=np.float32))
    orc.search(np.ones(8, np.float32), 3, ef=4)
    assert 1 <= orc.last_peak_candidates() <= 8
    orc.search(np.ones(8, np.float32), 0)
    assert orc.last_peak_candidates() == 0
