"""Graph-filter calls without a GPU: what kdb_index_set_relations and kdb_graph_filter_eval[_dev] can judge without the index is judged
before the handle is looked at, so a null handle reaches every such refusal; what needs a live index is in test_gpu_graph_filter.py."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def K():
    import kektordb_amd
    kektordb_amd.build_library()
    return kektordb_amd


def graph(K, **edit):
    """1 -> 3 (likes), 1 -> 1 (knows), 3 -> 3 (likes) over three nodes -- then one array of the view replaced"""
    g = K.RelationGraph([(1, "likes", 3), (1, "knows", 1), (3, "likes", 3)], 3)
    assert (g.off.tolist(), g.dst.tolist(), g.rel.tolist(), g.relations) == ([0, 0, 2, 2, 3], [3, 1, 3], [0, 1, 0], {"likes": 0, "knows": 1})
    assert g.rel_mask(["knows", "nobody"]) == 2 and g.query(3, ["likes", "knows"], "sideways", 9) == (3, 9, 3, 0, 3)
    for name, value in edit.items():
        setattr(g, name, np.asarray(value, dtype=getattr(g, name).dtype) if isinstance(getattr(g, name), np.ndarray) else value)
    return g


@pytest.mark.parametrize("edit,word", [
    (dict(off=[0, 1, 2, 2, 3]), b"start at 0"), (dict(off=[0, 0, 2, 1, 3]), b"never decrease"), (dict(dst=[3, 0, 3]), b"node 0"),
    (dict(dst=[3, 4, 3]), b"above n_nodes"), (dict(rel=[0, 64, 0]), b"64 or more"), (dict(n_nodes=0), b"n_nodes"), ({}, b"null index handle")])
def test_upload_refuses(K, edit, word):
    lib = K.load()
    assert lib.kdb_index_set_relations(None, C.byref(graph(K, **edit).view())) == -1
    assert word in lib.kdb_last_error(), lib.kdb_last_error()


@pytest.mark.parametrize("B,direction,outputs,and_pair,word", [
    (0, 0, True, (False, False), b"B outside"), (4097, 0, True, (False, False), b"B outside"), (1, 4, True, (False, False), b"direction"),
    (1, 0, False, (False, False), b"null"), (1, 0, True, (True, False), b"go together"), (1, 0, True, (False, True), b"go together"),
    (1, 0, True, (True, True), b"names no list"), (1, 0, True, (False, False), b"null index handle")])
def test_call_validation(K, B, direction, outputs, and_pair, word):
    lib = K.load()
    q = np.zeros(max(B, 1), dtype=K.index.GRAPH_QUERY_DTYPE)
    q["root"], q["direction"], q["rel_mask"] = 1, direction, 1
    buf = np.zeros(64, dtype=np.uint64).ctypes.data_as(C.c_void_p)
    out = buf if outputs else None
    and_lists, and_of = (buf if and_pair[0] else None), (buf if and_pair[1] else None)  # and_of_query[0] = 0 names no list of zero lists
    assert lib.kdb_graph_filter_eval(None, q.ctypes.data_as(C.c_void_p), B, out, 1, out, and_lists, 0, and_of) == -1
    assert word in lib.kdb_last_error(), lib.kdb_last_error()
    assert lib.kdb_graph_filter_eval_dev(None, q.ctypes.data_as(C.c_void_p), B, out, 1, out, and_lists, 0, and_of, None) == -1
    assert word in lib.kdb_last_error(), lib.kdb_last_error()
