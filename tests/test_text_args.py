"""Text calls without a GPU: everything kdb_index_set_text, kdb_text_search_batch and kdb_hybrid_search_batch can judge without the
index is judged before the handle is looked at, so a null handle reaches every refusal (as test_abi.py reaches the library).  What
needs a live index -- an id above the capacity, an empty slot, kdb_index_text_info left unchanged -- is in test_gpu_text.py."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def K():
    import kektordb_amd
    kektordb_amd.build_library()
    return kektordb_amd


def snapshot(K, **edit):
    """token a: docs 1, 2, 5; token b: doc 3 -- then one field of the view replaced"""
    t = K.TextIndex({"a": [(1, 1), (2, 2), (5, 1)], "b": [(3, 7)]}, {1: 4, 2: 4, 3: 9, 5: 1})
    idf = edit.pop("idf", None)
    for name, value in edit.items():
        setattr(t, name, np.asarray(value, dtype=getattr(t, name).dtype) if isinstance(getattr(t, name), np.ndarray) else value)
    return t, idf


REFUSED = {
    "not ascending": (dict(post_doc=[1, 5, 2, 3]), b"ascending"),
    "repeated id": (dict(post_doc=[1, 2, 2, 3]), b"ascending"),
    "id 0": (dict(post_doc=[0, 2, 5, 3]), b"id 0"),
    "id above n_ids": (dict(post_doc=[1, 2, 6, 3]), b"above n_ids"),
    "tf 0": (dict(post_tf=[1, 0, 1, 7]), b"frequency of 0"),
    "df above total_docs": (dict(total_docs=2), b"longer than total_docs"),
    "negative avg_len": (dict(avg_len=-1.0), b"avg_len"),
    "infinite avg_len": (dict(avg_len=float("inf")), b"avg_len"),
    "NaN avg_len": (dict(avg_len=float("nan")), b"avg_len"),
    "NaN idf": (dict(idf=[1.0, float("nan")]), b"idf"),
    "infinite idf": (dict(idf=[float("inf"), 1.0]), b"idf"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_upload_refuses(K, case):
    lib = K.load()
    edit, word = REFUSED[case]
    t, idf = snapshot(K, **edit)
    assert lib.kdb_index_set_text(None, 0, C.byref(t.view(idf))) == -1
    assert word in lib.kdb_last_error(), lib.kdb_last_error()


def test_upload_accepts_the_unedited_view_up_to_the_handle(K):
    lib = K.load()
    t, _ = snapshot(K)
    assert lib.kdb_index_set_text(None, 0, C.byref(t.view([0.5, 1.5]))) == -1
    assert b"null index handle" in lib.kdb_last_error()
    assert lib.kdb_index_set_text(None, 4, C.byref(t.view())) == -1
    assert b"field 4" in lib.kdb_last_error()


@pytest.mark.parametrize("k,t_stride,alpha,word", [(0, 4, 0.5, b"k outside"), (1025, 4, 0.5, b"k outside"), (10, 33, 0.5, b"t_stride"),
                                                   (10, 4, float("nan"), b"NaN")])
def test_call_validation(K, k, t_stride, alpha, word):
    lib = K.load()
    buf = np.zeros(8192, dtype=np.uint64).ctypes.data_as(C.c_void_p)
    assert lib.kdb_hybrid_search_batch(None, buf, 1, k, 10, 0, buf, buf, t_stride, alpha, None, 0, buf, buf, buf) == -1
    assert word in lib.kdb_last_error(), lib.kdb_last_error()
    if alpha == alpha:
        assert lib.kdb_text_search_batch(None, 0, buf, buf, 1, t_stride, k, None, buf, buf, buf, None, None) == -1
        assert word in lib.kdb_last_error(), lib.kdb_last_error()
        assert lib.kdb_text_search_batch_dev(None, 0, buf, buf, 1, t_stride, k, None, buf, buf, buf, None, None, None) == -1
        assert word in lib.kdb_last_error(), lib.kdb_last_error()


def test_text_index_sorts_and_keeps_the_last_entry(K):
    t = K.TextIndex({"x": [(9, 1), (2, 3), (9, 4)], "y": [(5, 2)]}, {2: 7, 5: 1, 9: 3})
    assert (t.post_off.tolist(), t.post_doc.tolist(), t.post_tf.tolist()) == ([0, 2, 3], [2, 9, 5], [3, 4, 2])
    assert (t.doc_len.tolist(), t.total_docs, t.avg_len) == ([0, 0, 7, 0, 0, 1, 0, 0, 0, 3], 3, 11 / 3)
    assert t.tokens(["y", "nope", "x"]) == [1, K.index.NO_TOKEN, 0]
