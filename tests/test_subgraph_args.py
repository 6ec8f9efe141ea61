"""kdb_subgraph_extract[_dev] without a GPU: what needs no index is judged before the handle is looked at, so a null handle reaches it."""
import ctypes as C

import numpy as np
import pytest

import kektordb_amd as K


@pytest.mark.parametrize("B,flags,reserved,guides,words,outputs,word", [
    (0, 0, 0, False, 1, True, b"B outside"), (4097, 0, 0, False, 1, True, b"B outside"), (1, 2, 0, True, 1, True, b"flags"), (1, 0, 7, True, 1, True, b"reserved"),
    (1, 1, 0, False, 1, True, b"null guides"), (1, 0, 0, False, (1 << 30) + 1, True, b"words_per_list"), (1, 0, 0, False, 1, False, b"null"),
    (1, 1, 0, True, 1, True, b"null index handle")])
def test_call_validation(B, flags, reserved, guides, words, outputs, word):
    K.build_library()
    lib = K.load()
    assert K.RelationGraph([(1, "likes", 3), (1, "knows", 1)], 3).subgraph_query(1, ["knows"], 2, 0.25) == (1, 2, 1, 0, 2, 0.25)
    q = np.zeros(max(B, 1), dtype=K.index.SUBGRAPH_QUERY_DTYPE)
    q["root"], q["flags"], q["reserved"], q["rel_mask"] = 1, flags, reserved, 1
    buf = np.zeros(64, dtype=np.uint64).ctypes.data_as(C.c_void_p)
    out, gd = (buf if outputs else None), (buf if guides else None)
    assert lib.kdb_subgraph_extract(None, q.ctypes.data_as(C.c_void_p), B, gd, out, words, out, out, None, 0) == -1
    assert word in lib.kdb_last_error(), lib.kdb_last_error()
    assert lib.kdb_subgraph_extract_dev(None, q.ctypes.data_as(C.c_void_p), B, gd, out, words, out, out, None, 0, None) == -1
    assert word in lib.kdb_last_error(), lib.kdb_last_error()
