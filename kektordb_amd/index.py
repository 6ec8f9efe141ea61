"""Host-side mirror of the reference's index interface for the search path.

`HipIndex` plays the role of `hnsw.Index` (pkg/core/hnsw/hnsw_index.go:42-135) for everything on
the hot path: SearchWithScores (:343), the graph/rows it searches, soft delete, plus the batch
entry points a Go shim's micro-batcher would call.  Names, argument meaning and error behaviour
follow the reference (`SearchWithScores(query, k, allowList, efSearch)` returns a possibly empty
list and never raises for an empty index / empty allow-list).  All compute goes through the C ABI
of include/kektor_hip.h into hand-written HIP kernels; there is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import KdbError, check

L2, COSINE = 0, 1
F32, F16, I8 = 0, 1, 2
SEARCH_NEEDS_REFINE = 1
SEARCH_PREPARED = 2
SEARCH_DIST_F64 = 8  # int8 indexes: distances come back as the reference's float64 (KDB_SEARCH_DIST_F64)
SEARCH_TIE_FLAG = 16    # KDB_SEARCH_TIE_FLAG: bit 31 of out_count marks a walk that met equal distances
SEARCH_HEAP_ORDER = 32  # KDB_SEARCH_HEAP_ORDER: such walks are repeated with the reference's two heaps
BY_ID_DROP_SELF = 256    # KDB_BY_ID_DROP_SELF: a by-id answer without the source's own id
VACUUM_ELECT_TOP_LEVEL = 1  # KDB_VACUUM_ELECT_TOP_LEVEL
COUNT_TIED = 0x80000000
COUNT_MASK = 0x7fffffff
MIXED_BAD_QUERY = 0x40000000  # KDB_MIXED_BAD_QUERY: a query of a mixed _dev batch outside the launch's bounds (count 0, never walked)
CONSENSUS_MAX_K = 64  # KDB_CONSENSUS_MAX_K
NO_FILTER = 0xFFFFFFFF  # KDB_NO_FILTER
# metadata filters on the device (kektor_hip.h, "metadata filters"): column kinds, term ops and flags, atom ops, limits
MAX_COLUMNS = 16
COL_F64, COL_CODE = 1, 2
FOP_NEVER, FOP_F64_EQ, FOP_F64_LT, FOP_F64_LE, FOP_F64_GT, FOP_F64_GE, FOP_CODE_EQ = 0, 1, 2, 3, 4, 5, 6
FT_OR_NEXT, FT_NOT, FT_END_BLOCK = 1, 2, 4
FA_EQ, FA_NE, FA_LT, FA_LE, FA_GT, FA_GE = 0, 1, 2, 3, 4, 5
FILTER_MAX_TERMS, FILTER_MAX_PROGRAMS = 64, 4096
FILTER_TILE_IDS, FILTER_CHUNK = 1024, 32  # kdb_filter_plan.h: ids one wave covers per list, programs that share a column fetch
TERM_DTYPE = np.dtype([("op", "u1"), ("flags", "u1"), ("col", "<u2"), ("code", "<u4"), ("value", "<f8")])  # kdb_filter_term
ROUTE_WALK, ROUTE_SCAN, ROUTE_EMPTY = 0, 1, 2  # out_route of kdb_search_filtered
# kdb_consensus: CalculateConsensus's score, variance and maxVar, len(nodes), len(activeNodes)
CONSENSUS_DTYPE = np.dtype([("score", "<f8"), ("variance", "<f8"), ("max_pair", "<f8"), ("n_found", "<u4"), ("n_active", "<u4")])

_ELEM = {F32: np.float32, F16: np.uint16, I8: np.int8}


@dataclass
class SearchResult:
    """types.SearchResult (pkg/core/types/types.go:12-15)."""
    DocID: int
    Score: float


def _ptr(a):
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)


def _tptr(t):
    """device pointer of a torch tensor (plumbing only)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _ready(stream):
    """Device tensors handed to the library must be complete.  With an explicit HIP stream the caller orders
    the work; without one the library runs on its own non-blocking stream, so wait for torch's current stream."""
    if not stream:
        import torch
        torch.cuda.current_stream().synchronize()


class HipIndex:
    def __init__(self, dim: int, metric: int = COSINE, precision: int = F32, m: int = 16,
                 ef_construction: int = 200, capacity: int = 1 << 20, device_id: int = 0, f16_shadow: bool = True,
                 walk_planes: bool = True):
        """f16_shadow: float32 indexes make a half-precision RANKING copy of the rows at their first exact scan (+50 % row
        memory from then on, answers unchanged); False sets KDB_INDEX_NO_F16_SHADOW (never).
        walk_planes: float32 cosine indexes of 768 columns make the walk planes (the rows as two 16-bit planes + a bound per
        row, +100 % row memory, answers unchanged) at their first large-batch walk; False sets KDB_INDEX_NO_WALK_PLANES (never)."""
        self.L = _lib.load()
        self.dim, self.metric, self.precision = int(dim), int(metric), int(precision)
        self.m = m if m > 0 else 16
        self.ef_construction = ef_construction if ef_construction > 0 else 200
        self.capacity = int(capacity)
        self.device_id = device_id
        self.needs_refine = False
        desc = _lib.IndexDesc(self.dim, self.metric, self.precision, self.m, self.ef_construction, self.capacity,
                              device_id, (0 if f16_shadow else 1) | (0 if walk_planes else 2))
        h = C.c_void_p()
        check(self.L.kdb_index_create(C.byref(desc), C.byref(h)), "kdb_index_create")
        self.h = h
        self._closed = False

    # ---- lifecycle (Close, hnsw_index.go:3533-3586) -------------------------------------------
    def Close(self):
        if not self._closed and self.h:
            self.L.kdb_index_destroy(self.h)
            self.h = None
            self._closed = True

    close = Close

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass

    def _live(self):
        if self._closed:
            raise KdbError("index is closed")

    def Compress(self, precision: int, rebuild_graph: bool = False) -> "HipIndex":
        """DB.Compress (pkg/core/core.go:1128-1290) on the device: a NEW index of `precision` (F16 / I8) from this
        float32 one -- quantizer trained and rows converted in HBM; the graph is kept, or rebuilt by the GPU builder
        with the new precision's distances (what the reference's AddBatch re-insertion does) when rebuild_graph is set."""
        self._live()
        h = C.c_void_p()
        check(self.L.kdb_index_compress(self.h, int(precision), 1 if rebuild_graph else 0, C.byref(h)), "kdb_index_compress")
        new = HipIndex.__new__(HipIndex)
        new.L, new.dim, new.metric, new.precision = self.L, self.dim, self.metric, int(precision)
        new.m, new.ef_construction, new.capacity, new.device_id = self.m, self.ef_construction, self.capacity, self.device_id
        new.needs_refine, new.h, new._closed = False, h, False
        return new

    def quantizer_absmax(self) -> float:
        a = C.c_float()
        check(self.L.kdb_index_get_quantizer(self.h, C.byref(a)), "kdb_index_get_quantizer")
        return float(a.value)

    # ---- population ------------------------------------------------------------------------------
    def upload_rows(self, rows, first_id: int = 1):
        """rows: (n, dim) array already in STORED form (see kdb_index_upload_rows) or a torch device tensor."""
        self._live()
        if hasattr(rows, "data_ptr"):
            assert rows.is_contiguous() and rows.shape[1] == self.dim
            _ready(None)
            check(self.L.kdb_index_upload_rows_dev(self.h, first_id, rows.shape[0], _tptr(rows)), "upload_rows_dev")
            return
        a = np.ascontiguousarray(rows, dtype=_ELEM[self.precision])
        assert a.ndim == 2 and a.shape[1] == self.dim
        check(self.L.kdb_index_upload_rows(self.h, first_id, a.shape[0], _ptr(a)), "upload_rows")

    def upload_arena(self, arena_dir: str, count: int, slot_table=None):
        """rows 1..count from the reference's arena files (pkg/storage/mmap/arena.go layout)."""
        st = None if slot_table is None else np.ascontiguousarray(slot_table, dtype=np.uint32)
        check(self.L.kdb_index_upload_arena(self.h, arena_dir.encode(), _ptr(st), int(count)), "upload_arena")

    def upload_norms(self, norms, first_id: int = 1):
        a = np.ascontiguousarray(norms, dtype=np.float32)
        check(self.L.kdb_index_upload_norms(self.h, first_id, a.shape[0], _ptr(a)), "upload_norms")

    def set_quantizer(self, abs_max: float):
        check(self.L.kdb_index_set_quantizer(self.h, float(abs_max)), "set_quantizer")

    def set_launch_timing(self, on: bool):
        """HIP events around the graph-search launches (launch_stats' kernel_ms); off saves two queue packets per call"""
        check(self.L.kdb_index_set_launch_timing(self.h, 1 if on else 0), "kdb_index_set_launch_timing")

    def caller_stats(self):
        """concurrent host-pointer calls: launches that left through a slot, the calls they carried, the largest launch, slots"""
        out = np.zeros(10, dtype=np.uint64)
        check(self.L.kdb_index_caller_stats(self.h, _ptr(out)), "kdb_index_caller_stats")
        return {"launches": int(out[0]), "calls": int(out[1]), "largest": int(out[2]), "slots": int(out[3]), "combined_calls": int(out[4]),
                "ns_to_launch": int(out[5]), "ns_launch_to_done": int(out[6]), "ns_in_launch": int(out[7]), "naps": int(out[8]), "wait_estimate_ns": int(out[9])}

    def reserve(self, new_capacity: int):
        """growNodes (hnsw_index.go:2732-2768): raise the capacity of a live index, on the device"""
        check(self.L.kdb_index_reserve(self.h, new_capacity), "kdb_index_reserve")
        self.capacity = max(getattr(self, "capacity", 0), new_capacity)

    def drop_f16_shadow(self, refuse_for_good: bool = False):
        check(self.L.kdb_index_drop_f16_shadow(self.h, 1 if refuse_for_good else 0), "kdb_index_drop_f16_shadow")

    def drop_walk_planes(self, refuse_for_good: bool = False):
        check(self.L.kdb_index_drop_walk_planes(self.h, 1 if refuse_for_good else 0), "kdb_index_drop_walk_planes")

    def set_count(self, count: int):
        check(self.L.kdb_index_set_count(self.h, int(count)), "set_count")

    def upload_graph(self, count, entry, max_level, levels, offsets, neighbors, deleted_bits=None):
        """Per-level CSR in the layout of kdb_graph_view (lists keep the reference's stored order)."""
        self._live()
        nl = max_level + 1
        levels = np.ascontiguousarray(levels, dtype=np.uint8)
        offs = [np.ascontiguousarray(o, dtype=np.uint64) for o in offsets[:nl]]
        nbrs = [np.ascontiguousarray(n if len(n) else np.zeros(1, np.uint32), dtype=np.uint32) for n in neighbors[:nl]]
        op = (C.c_void_p * max(nl, 1))(*[o.ctypes.data for o in offs])
        npp = (C.c_void_p * max(nl, 1))(*[n.ctypes.data for n in nbrs])
        db = None if deleted_bits is None else np.ascontiguousarray(deleted_bits, dtype=np.uint64)
        g = _lib.GraphView(int(count), int(entry), int(max_level), 0, levels.ctypes.data,
                           C.cast(op, C.c_void_p), C.cast(npp, C.c_void_p), None if db is None else db.ctypes.data)
        check(self.L.kdb_index_upload_graph(self.h, C.byref(g)), "upload_graph")

    def upload_graph_obj(self, graph):
        """graph: any object with count/entry/max_level/levels/offsets/neighbors/deleted_bits."""
        self.upload_graph(graph.count, graph.entry, graph.max_level, graph.levels, graph.offsets, graph.neighbors,
                          graph.deleted_bits)

    def Delete(self, ids: Sequence[int]):
        """soft delete by internal id (Node.Deleted, hnsw_index.go:2303)."""
        a = np.ascontiguousarray(ids, dtype=np.uint32)
        check(self.L.kdb_index_mark_deleted(self.h, _ptr(a), a.size), "mark_deleted")

    # ---- incremental refresh (writers touched a few nodes) ----------------------------------------------
    def append_nodes(self, first_id: int, levels):
        lv = np.ascontiguousarray(levels, dtype=np.uint8)
        check(self.L.kdb_index_append_nodes(self.h, int(first_id), lv.size, _ptr(lv)), "kdb_index_append_nodes")

    def patch_adjacency(self, level: int, ids, lists):
        """lists: one sequence of neighbour ids per node of `ids` (stored order)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        off = np.zeros(ids.size + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in lists])
        nb = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.uint32) for x in lists]) if len(lists) else
                                  np.zeros(0, np.uint32), dtype=np.uint32)
        if nb.size == 0:
            nb = np.zeros(1, np.uint32)
        check(self.L.kdb_index_patch_adjacency(self.h, int(level), ids.size, _ptr(ids), _ptr(off), _ptr(nb)),
              "kdb_index_patch_adjacency")

    def set_entry(self, entry: int, max_level: int):
        check(self.L.kdb_index_set_entry(self.h, int(entry), int(max_level)), "kdb_index_set_entry")

    def build(self, count: int, batch: int = 0, ef_construction: int = 0, seed: int = 1):
        """GPU batched construction over rows 1..count (addBatchInternal, hnsw_index.go:1479-2088)."""
        p = _lib.BuildParams(batch, ef_construction, seed, 0, 0)
        check(self.L.kdb_index_build(self.h, int(count), C.byref(p)), "kdb_index_build")

    def add_batch(self, first_id: int, levels, ef_construction: int = 0):
        """AddBatch (addBatchInternal, hnsw_index.go:1479-2088) for rows already uploaded at first_id.., linked as the
        reference links them (kdb_index_add_batch); levels: one per new node"""
        lv = np.ascontiguousarray(levels, dtype=np.uint8)
        check(self.L.kdb_index_add_batch(self.h, int(first_id), lv.size, _ptr(lv), int(ef_construction), 1), "kdb_index_add_batch")

    def add(self, first_id: int, levels, ef_construction: int = 0) -> dict:
        """Add (hnsw_index.go:472-809), the sequential single insert, for rows already uploaded at first_id.. (kdb_index_add):
        one node after another, each linked against the graph the nodes before it left; levels: one per new node, as drawn
        (capped at maxLevel+1 on the device side of the call); -> the call's statistics"""
        self._live()
        lv = np.ascontiguousarray(levels, dtype=np.uint8)
        p = _lib.AddParams(int(ef_construction), 0)
        st = _lib.AddStats()
        check(self.L.kdb_index_add(self.h, int(first_id), lv.size, _ptr(lv), C.byref(p), C.byref(st)), "kdb_index_add")
        return {f: int(getattr(st, f)) for f, _ in _lib.AddStats._fields_}

    def refine(self, ids=None, ef_construction: int = 0, chunk_nodes: int = 0) -> dict:
        """GraphOptimizer.Refine (optimizer.go:288-464) on the device (kdb_index_refine): the lists of `ids` (None: every live
        node) are computed again against the graph as it is and committed together; -> the call's statistics"""
        self._live()
        a = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
        p = _lib.RefineParams(int(ef_construction), 0, int(chunk_nodes))
        st = _lib.RefineStats()
        check(self.L.kdb_index_refine(self.h, _ptr(a), 0 if a is None else a.size, C.byref(p), C.byref(st)), "kdb_index_refine")
        return {"nodes_refined": int(st.nodes_refined), "lists_written": int(st.lists_written),
                "lists_changed": int(st.lists_changed), "dead_links_dropped": int(st.dead_links_dropped)}

    def RunTurboRefine(self) -> dict:
        """RunTurboRefine (optimizer.go:679-719): the whole graph with the index's efConstruction, then needs_refine is
        cleared (:716)"""
        st = self.refine()
        self.needs_refine = False
        return st

    def dead_link_scan(self, cap: Optional[int] = None):
        """the census of Vacuum (optimizer.go:165-193) on the device, read-only (kdb_index_dead_link_scan): -> (ascending ids of
        the live nodes that hold a link to a deleted node, dead links in live nodes' lists, deleted nodes); cap: at most that
        many ids are handed out (None: all of them)"""
        self._live()
        n, links, dead = C.c_uint32(), C.c_uint64(), C.c_uint64()
        if cap is None:
            check(self.L.kdb_index_dead_link_scan(self.h, None, 0, C.byref(n), C.byref(links), C.byref(dead)), "kdb_index_dead_link_scan")
            cap = n.value
        ids = np.zeros(max(int(cap), 1), dtype=np.uint32)
        check(self.L.kdb_index_dead_link_scan(self.h, _ptr(ids), int(cap), C.byref(n), C.byref(links), C.byref(dead)), "kdb_index_dead_link_scan")
        self.last_scan_nodes = int(n.value)                     # |R| whatever cap was
        return ids[:min(int(cap), n.value)], int(links.value), int(dead.value)

    def vacuum(self, ef_construction: int = 0, elect_top_level: bool = False, chunk_nodes: int = 0) -> dict:
        """GraphOptimizer.Vacuum (optimizer.go:133-277) on the device (kdb_index_vacuum): the live nodes that hold a link to a
        deleted node are re-linked as refine does it, a deleted entry point is replaced (the lowest live id, or with
        elect_top_level the live node of the highest level), the deleted nodes' lists and rows are cleared; -> the statistics"""
        self._live()
        p = _lib.VacuumParams(int(ef_construction), VACUUM_ELECT_TOP_LEVEL if elect_top_level else 0, int(chunk_nodes))
        st = _lib.VacuumStats()
        check(self.L.kdb_index_vacuum(self.h, C.byref(p), C.byref(st)), "kdb_index_vacuum")
        return {f: int(getattr(st, f)) for f, _ in _lib.VacuumStats._fields_ if f != "reserved"}

    def MaintenanceRun(self, task: str) -> bool:
        """MaintenanceRun (hnsw_index.go:976): "vacuum" -> Vacuum (true when there was a deleted node), "refine" -> Refine"""
        if task == "vacuum":
            return self.vacuum()["dead_nodes"] > 0
        if task == "refine":
            return self.refine()["nodes_refined"] > 0
        raise ValueError(f"unknown maintenance task {task!r}")

    def test_select_neighbors(self, cand_ids, cand_keys, cand_cnt, maxm: int):
        """TEST HOOK: the GPU builder's selectNeighbors on caller-supplied lists ([n_lists, stride] ids / ascending keys;
        keys are float32 ordering keys, or -- int8 indexes -- the float64 distances)"""
        self._live()
        ids = np.ascontiguousarray(cand_ids, dtype=np.uint32)
        keys = np.ascontiguousarray(cand_keys, dtype=np.float64 if self.precision == I8 else np.float32)
        cnt = np.ascontiguousarray(cand_cnt, dtype=np.uint32)
        n_lists, stride = ids.shape
        out = np.zeros((n_lists, maxm), dtype=np.uint32)
        oc = np.zeros(n_lists, dtype=np.uint32)
        check(self.L.kdb_test_select_neighbors(self.h, n_lists, stride, _ptr(ids), _ptr(keys), _ptr(cnt), int(maxm), _ptr(out),
                                               _ptr(oc)), "kdb_test_select_neighbors")
        return out, oc

    def graph_info(self):
        c, e, ml = C.c_uint32(), C.c_uint32(), C.c_int32()
        check(self.L.kdb_index_graph_info(self.h, C.byref(c), C.byref(e), C.byref(ml)), "graph_info")
        return c.value, e.value, ml.value

    def download_graph(self):
        """-> (count, entry, max_level, levels, offsets[list], neighbors[list])"""
        count, entry, max_level = self.graph_info()
        nl = max_level + 1
        sizes = np.zeros(max(nl, 1), dtype=np.uint64)
        check(self.L.kdb_index_download_graph(self.h, None, None, None, _ptr(sizes)), "download_graph(sizes)")
        levels = np.zeros(count + 1, dtype=np.uint8)
        offs = [np.zeros(count + 2, dtype=np.uint64) for _ in range(nl)]
        nbrs = [np.zeros(max(int(sizes[l]), 1), dtype=np.uint32) for l in range(nl)]
        op = (C.c_void_p * max(nl, 1))(*[o.ctypes.data for o in offs])
        npp = (C.c_void_p * max(nl, 1))(*[n.ctypes.data for n in nbrs])
        check(self.L.kdb_index_download_graph(self.h, _ptr(levels), C.cast(op, C.c_void_p), C.cast(npp, C.c_void_p),
                                              _ptr(sizes)), "download_graph")
        nbrs = [nbrs[l][:int(sizes[l])] for l in range(nl)]
        return count, entry, max_level, levels, offs, nbrs

    def download_rows(self, first_id: int, n: int):
        out = np.zeros((n, self.dim), dtype=_ELEM[self.precision])
        check(self.L.kdb_index_download_rows(self.h, first_id, n, _ptr(out)), "download_rows")
        return out

    # ---- search ----------------------------------------------------------------------------------
    def _flags(self, prepared=False):
        return (SEARCH_NEEDS_REFINE if self.needs_refine else 0) | (SEARCH_PREPARED if prepared else 0)

    def search_batch(self, queries, k: int, ef: int = 0, allow_bits=None, trace: bool = False, prepared=False,
                     fail_on_drop: bool = False, dist64: bool = False, tie_flag: bool = False, heap_order: bool = False):
        """B queries -> (ids [B,k] u32, raw dist [B,k] f32, count [B] u32[, (n_dist[B], n_hops[B])]).
        fail_on_drop: KDB_SEARCH_FAIL_ON_DROP -- raise KdbError (status -7) when a walk discarded pending deleted candidates
        dist64 (int8 indexes): dist is float64, the reference's own distances (KDB_SEARCH_DIST_F64)
        tie_flag: KDB_SEARCH_TIE_FLAG -- count[b] carries COUNT_TIED (bit 31) when query b's walk met equal distances
        heap_order: KDB_SEARCH_HEAP_ORDER -- such queries are walked again with the reference's two heaps (ids, order and
        counters are then the reference's, ties included)"""
        self._live()
        q = np.ascontiguousarray(queries, dtype=np.float32)
        assert q.ndim == 2 and q.shape[1] == self.dim
        B = q.shape[0]
        ids = np.zeros((B, k), dtype=np.uint32)
        dist = np.full((B, k), np.inf, dtype=np.float64 if dist64 else np.float32)
        cnt = np.zeros(B, dtype=np.uint32)
        ab = None if allow_bits is None else np.ascontiguousarray(allow_bits, dtype=np.uint64)
        nd = nh = None
        if trace:
            nd = np.zeros(B, dtype=np.uint32)
            nh = np.zeros(B, dtype=np.uint32)
            check(self.L.kdb_search_set_trace(self.h, _ptr(nd), _ptr(nh), 0), "set_trace")
        try:
            check(self.L.kdb_search_batch(self.h, _ptr(q), B, k, ef, _ptr(ab), self._flags(prepared) | (4 if fail_on_drop else 0) | (SEARCH_DIST_F64 if dist64 else 0)
                                          | (SEARCH_TIE_FLAG if tie_flag else 0) | (SEARCH_HEAP_ORDER if heap_order else 0),
                                          _ptr(ids), _ptr(dist), _ptr(cnt)), "kdb_search_batch")
        finally:
            if trace:
                self.L.kdb_search_set_trace(self.h, None, None, 0)
        if trace:
            return ids, dist, cnt, (nd, nh)
        return ids, dist, cnt

    def search_batch_dev(self, d_queries, k: int, ef: int, d_out_ids, d_out_dist, d_out_count, d_allow=None,
                         stream=None, prepared=False, dist64=False, tie_flag=False, heap_order=False):
        """torch device tensors in, asynchronous on `stream` (a raw hipStream_t int or None).
        dist64 (int8 indexes): d_out_dist is a float64 tensor (KDB_SEARCH_DIST_F64)"""
        self._live()
        _ready(stream)
        B = d_queries.shape[0]
        check(self.L.kdb_search_batch_dev(self.h, _tptr(d_queries), B, k, ef, _tptr(d_allow), self._flags(prepared) | (SEARCH_DIST_F64 if dist64 else 0)
                                          | (SEARCH_TIE_FLAG if tie_flag else 0) | (SEARCH_HEAP_ORDER if heap_order else 0),
                                          _tptr(d_out_ids), _tptr(d_out_dist), _tptr(d_out_count),
                                          C.c_void_p(stream) if stream else None), "kdb_search_batch_dev")

    def search_batch_mixed(self, queries, ks, efs, allow_bits=None, trace: bool = False, prepared=False, fail_on_drop: bool = False,
                           dist64: bool = False, tie_flag: bool = False, heap_order: bool = False, k_stride: Optional[int] = None):
        """B requests that differ in k and efSearch, one launch (kdb_search_batch_mixed): query b is answered as search_batch answers
        it alone with (ks[b], efs[b]).  -> (ids [B,stride] u32, raw dist [B,stride], count [B] u32[, (n_dist[B], n_hops[B])]) with
        stride = max(ks) unless k_stride says otherwise; positions [count, stride) of a row hold id 0 and +inf.  Keyword flags as for
        search_batch."""
        self._live()
        q = np.ascontiguousarray(queries, dtype=np.float32)
        assert q.ndim == 2 and q.shape[1] == self.dim
        B = q.shape[0]
        kk = np.ascontiguousarray(ks, dtype=np.uint32)
        ee = np.ascontiguousarray(efs, dtype=np.uint32)
        assert kk.shape == (B,) and ee.shape == (B,)
        stride = int(k_stride) if k_stride is not None else (int(kk.max()) if B else 1)
        ids = np.zeros((B, stride), dtype=np.uint32)
        dist = np.full((B, stride), np.inf, dtype=np.float64 if dist64 else np.float32)
        cnt = np.zeros(B, dtype=np.uint32)
        ab = None if allow_bits is None else np.ascontiguousarray(allow_bits, dtype=np.uint64)
        nd = nh = None
        if trace:
            nd = np.zeros(B, dtype=np.uint32)
            nh = np.zeros(B, dtype=np.uint32)
            check(self.L.kdb_search_set_trace(self.h, _ptr(nd), _ptr(nh), 0), "set_trace")
        try:
            check(self.L.kdb_search_batch_mixed(self.h, _ptr(q), B, _ptr(kk), _ptr(ee), stride, _ptr(ab),
                                                self._flags(prepared) | (4 if fail_on_drop else 0) | (SEARCH_DIST_F64 if dist64 else 0)
                                                | (SEARCH_TIE_FLAG if tie_flag else 0) | (SEARCH_HEAP_ORDER if heap_order else 0),
                                                _ptr(ids), _ptr(dist), _ptr(cnt)), "kdb_search_batch_mixed")
        finally:
            if trace:
                self.L.kdb_search_set_trace(self.h, None, None, 0)
        if trace:
            return ids, dist, cnt, (nd, nh)
        return ids, dist, cnt

    def search_batch_mixed_dev(self, d_queries, d_ks, d_efs, k_stride: int, ef_max: int, d_out_ids, d_out_dist, d_out_count, d_allow_lists=None,
                               d_allow_of_query=None, stream=None, prepared=False, dist64=False, tie_flag=False, heap_order=False):
        """torch device tensors in, asynchronous on `stream`: d_ks / d_efs [B] int32 (read as uint32), outputs [B, k_stride]; ef_max is
        the largest effective ef the batch holds.  d_allow_of_query given: d_allow_lists is [G, words] and query b uses list
        d_allow_of_query[b] (-1 = none), as search_batch_multi_dev; else d_allow_lists is one optional list for the whole batch.  A
        query outside the launch's bounds comes back as count 0 | MIXED_BAD_QUERY."""
        self._live()
        _ready(stream)
        B = int(d_queries.shape[0])
        G = words = 0
        if d_allow_of_query is not None:
            G, words = int(d_allow_lists.shape[0]), int(d_allow_lists.shape[1])
        check(self.L.kdb_search_batch_mixed_dev(self.h, _tptr(d_queries), B, _tptr(d_ks), _tptr(d_efs), k_stride, ef_max, _tptr(d_allow_lists), G, words,
                                                _tptr(d_allow_of_query), self._flags(prepared) | (SEARCH_DIST_F64 if dist64 else 0)
                                                | (SEARCH_TIE_FLAG if tie_flag else 0) | (SEARCH_HEAP_ORDER if heap_order else 0),
                                                _tptr(d_out_ids), _tptr(d_out_dist), _tptr(d_out_count), C.c_void_p(stream) if stream else None),
              "kdb_search_batch_mixed_dev")

    def mixed_stats(self):
        """kdb_index_mixed_stats: [launches that carried at least two distinct (k, effective ef), the calls they carried, callers that
        could not join an open launch because of their k or ef, 0]"""
        out = np.zeros(4, dtype=np.uint64)
        check(self.L.kdb_index_mixed_stats(self.h, _ptr(out)), "kdb_index_mixed_stats")
        return [int(x) for x in out]

    def flat_scan_batch(self, queries, k: int, allow_bits=None, dist64: bool = False):
        self._live()
        q = np.ascontiguousarray(queries, dtype=np.float32)
        B = q.shape[0]
        ids = np.zeros((B, k), dtype=np.uint32)
        dist = np.full((B, k), np.inf, dtype=np.float64 if dist64 else np.float32)
        cnt = np.zeros(B, dtype=np.uint32)
        ab = None if allow_bits is None else np.ascontiguousarray(allow_bits, dtype=np.uint64)
        check(self.L.kdb_flat_scan_batch(self.h, _ptr(q), B, k, _ptr(ab), self._flags() | (SEARCH_DIST_F64 if dist64 else 0), _ptr(ids), _ptr(dist),
                                         _ptr(cnt)), "kdb_flat_scan_batch")
        return ids, dist, cnt

    def flat_scan_batch_dev(self, d_queries, k, d_out_ids, d_out_dist, d_out_count, d_allow=None, stream=None, dist64=False):
        self._live()
        _ready(stream)
        B = d_queries.shape[0]
        check(self.L.kdb_flat_scan_batch_dev(self.h, _tptr(d_queries), B, k, _tptr(d_allow), self._flags() | (SEARCH_DIST_F64 if dist64 else 0),
                                             _tptr(d_out_ids), _tptr(d_out_dist), _tptr(d_out_count),
                                             C.c_void_p(stream) if stream else None), "kdb_flat_scan_batch_dev")

    def distance_batch(self, queries, ids, prepared=False):
        """raw accumulates [B, C] of B queries against ids[B, C] (0 = skip -> +inf)."""
        self._live()
        q = np.ascontiguousarray(queries, dtype=np.float32)
        ii = np.ascontiguousarray(ids, dtype=np.uint32)
        B, Cn = ii.shape
        out = np.zeros((B, Cn), dtype=np.float32)
        check(self.L.kdb_distance_batch(self.h, _ptr(q), B, _ptr(ii), Cn, self._flags(prepared), _ptr(out)),
              "kdb_distance_batch")
        return out

    def distance_batch_dev(self, d_queries, d_ids, d_out, stream=None, prepared=False):
        _ready(stream)
        B, Cn = d_ids.shape
        check(self.L.kdb_distance_batch_dev(self.h, _tptr(d_queries), B, _tptr(d_ids), Cn, self._flags(prepared),
                                            _tptr(d_out), C.c_void_p(stream) if stream else None),
              "kdb_distance_batch_dev")

    # ---- stored rows as queries (GetNodeData / VGetMany + SearchWithScores, on the device) -------------------------
    def decode_rows(self, ids):
        """GetNodeData(id).Vector (hnsw_index.go:2909-2959) for every id -> (vectors [n, dim] f32, found [n] bool): float32 rows as
        stored, float16 widened, int8 dequantised; an id that is 0, above count or deleted: a zero row, found False"""
        self._live()
        a = np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        out = np.zeros((a.size, self.dim), dtype=np.float32)
        found = np.zeros(a.size, dtype=np.uint8)
        check(self.L.kdb_index_decode_rows(self.h, _ptr(a), a.size, _ptr(out), _ptr(found)), "kdb_index_decode_rows")
        return out, found.astype(bool)

    def decode_rows_dev(self, d_ids, d_out, d_found=None, stream=None):
        """torch device tensors: d_ids [n] int32 / uint32, d_out [n, dim] float32, d_found [n] uint8 or None"""
        self._live()
        _ready(stream)
        check(self.L.kdb_index_decode_rows_dev(self.h, _tptr(d_ids), int(d_ids.shape[0]), _tptr(d_out), _tptr(d_found),
                                               C.c_void_p(stream) if stream else None), "kdb_index_decode_rows_dev")

    def _by_id_flags(self, fail_on_drop=False, dist64=False, tie_flag=False, heap_order=False, drop_self=False):
        return (self._flags() | (4 if fail_on_drop else 0) | (SEARCH_DIST_F64 if dist64 else 0) | (SEARCH_TIE_FLAG if tie_flag else 0)
                | (SEARCH_HEAP_ORDER if heap_order else 0) | (BY_ID_DROP_SELF if drop_self else 0))

    def search_by_id(self, ids, k: int, ef: int = 0, allow_bits=None, trace: bool = False, fail_on_drop: bool = False, dist64: bool = False,
                     tie_flag: bool = False, heap_order: bool = False, drop_self: bool = False, flags: int = 0):
        """search_batch with the stored rows of `ids` as the queries (kdb_search_by_id): what search_batch(decode_rows(ids)[0], ...)
        returns, bit for bit, with 4 bytes per query crossing the bus; a source id that is not found gets count 0.
        drop_self: the answer without the source's own id (the call runs with k + 1).  flags: further raw KDB_SEARCH_* bits"""
        self._live()
        a = np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        B = a.size
        out_ids = np.zeros((B, k), dtype=np.uint32)
        dist = np.full((B, k), np.inf, dtype=np.float64 if dist64 else np.float32)
        cnt = np.zeros(B, dtype=np.uint32)
        ab = None if allow_bits is None else np.ascontiguousarray(allow_bits, dtype=np.uint64)
        nd = nh = None
        if trace:
            nd = np.zeros(B, dtype=np.uint32)
            nh = np.zeros(B, dtype=np.uint32)
            check(self.L.kdb_search_set_trace(self.h, _ptr(nd), _ptr(nh), 0), "set_trace")
        try:
            check(self.L.kdb_search_by_id(self.h, _ptr(a), B, k, ef, _ptr(ab),
                                          self._by_id_flags(fail_on_drop, dist64, tie_flag, heap_order, drop_self) | int(flags),
                                          _ptr(out_ids), _ptr(dist), _ptr(cnt)), "kdb_search_by_id")
        finally:
            if trace:
                self.L.kdb_search_set_trace(self.h, None, None, 0)
        if trace:
            return out_ids, dist, cnt, (nd, nh)
        return out_ids, dist, cnt

    def search_by_id_dev(self, d_ids, k: int, ef: int, d_out_ids, d_out_dist, d_out_count, d_allow=None, stream=None, dist64=False,
                         tie_flag=False, heap_order=False, drop_self=False):
        """torch device tensors in (d_ids [B] int32 / uint32), asynchronous on `stream` (kdb_search_by_id_dev)"""
        self._live()
        _ready(stream)
        check(self.L.kdb_search_by_id_dev(self.h, _tptr(d_ids), int(d_ids.shape[0]), k, ef, _tptr(d_allow),
                                          self._by_id_flags(False, dist64, tie_flag, heap_order, drop_self), _tptr(d_out_ids), _tptr(d_out_dist),
                                          _tptr(d_out_count), C.c_void_p(stream) if stream else None), "kdb_search_by_id_dev")

    def flat_scan_by_id(self, ids, k: int, allow_bits=None, dist64: bool = False, drop_self: bool = False, flags: int = 0):
        """flat_scan_batch with the stored rows of `ids` as the queries (kdb_flat_scan_by_id)"""
        self._live()
        a = np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        B = a.size
        out_ids = np.zeros((B, k), dtype=np.uint32)
        dist = np.full((B, k), np.inf, dtype=np.float64 if dist64 else np.float32)
        cnt = np.zeros(B, dtype=np.uint32)
        ab = None if allow_bits is None else np.ascontiguousarray(allow_bits, dtype=np.uint64)
        check(self.L.kdb_flat_scan_by_id(self.h, _ptr(a), B, k, _ptr(ab), self._by_id_flags(dist64=dist64, drop_self=drop_self) | int(flags),
                                         _ptr(out_ids), _ptr(dist), _ptr(cnt)), "kdb_flat_scan_by_id")
        return out_ids, dist, cnt

    def flat_scan_by_id_dev(self, d_ids, k: int, d_out_ids, d_out_dist, d_out_count, d_allow=None, stream=None, dist64=False, drop_self=False):
        self._live()
        _ready(stream)
        check(self.L.kdb_flat_scan_by_id_dev(self.h, _tptr(d_ids), int(d_ids.shape[0]), k, _tptr(d_allow),
                                             self._by_id_flags(dist64=dist64, drop_self=drop_self), _tptr(d_out_ids), _tptr(d_out_dist),
                                             _tptr(d_out_count), C.c_void_p(stream) if stream else None), "kdb_flat_scan_by_id_dev")

    # ---- CalculateConsensus / VBeliefState on the device (consensus.hip) -------------------------------------------
    def consensus(self, ids, counts=None, queries=None, active_bits=None, want_centroid=False, want_gram=False, flags: int = 0):
        """CalculateConsensus (pkg/engine/epistemic_types.go:126-178) over the stored vectors of B id lists (kdb_consensus_batch).
        ids [B, stride] (stride <= 64); counts [B] or None (every list full; bit 31 of a search's count is ignored); queries [B, dim]
        or None; active_bits: dense uint64 bitset over ids, clear = historical (epistemic.go:104-111), None = all active.
        Returns a dict: rec (CONSENSUS_DTYPE [B]: score, variance, max_pair, n_found, n_active), similarity ([B, stride] f64, -1.0 =
        no node; None without queries), centroid ([B, dim] f32 or None), gram ([B, stride + 1, stride + 1] f64 or None)"""
        self._live()
        ii = np.ascontiguousarray(ids, dtype=np.uint32)
        assert ii.ndim == 2
        B, stride = ii.shape
        cn = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint32).ravel()
        assert cn is None or cn.size == B
        q = None if queries is None else np.ascontiguousarray(queries, dtype=np.float32)
        assert q is None or q.shape == (B, self.dim)
        ab = None if active_bits is None else np.ascontiguousarray(active_bits, dtype=np.uint64)
        rec = np.zeros(B, dtype=CONSENSUS_DTYPE)
        sim = None if q is None else np.zeros((B, stride), dtype=np.float64)
        cen = np.zeros((B, self.dim), dtype=np.float32) if want_centroid else None
        gram = np.zeros((B, stride + 1, stride + 1), dtype=np.float64) if want_gram else None
        check(self.L.kdb_consensus_batch(self.h, _ptr(ii), _ptr(cn), B, stride, _ptr(q), _ptr(ab), int(flags), _ptr(rec), _ptr(sim), _ptr(cen),
                                         _ptr(gram)), "kdb_consensus_batch")
        return {"rec": rec, "similarity": sim, "centroid": cen, "gram": gram}

    def consensus_dev(self, d_ids, d_out, d_counts=None, d_queries=None, d_active=None, d_similarity=None, d_centroid=None, d_gram=None,
                      stream=None):
        """torch device tensors: d_ids [B, stride] int32, d_out [B, 32] uint8 (kdb_consensus records: view as CONSENSUS_DTYPE on the
        host), d_counts [B] int32, d_queries [B, dim] f32, d_similarity [B, stride] f64, d_centroid [B, dim] f32,
        d_gram [B, stride + 1, stride + 1] f64; asynchronous on `stream` (kdb_consensus_batch_dev)"""
        self._live()
        _ready(stream)
        B, stride = int(d_ids.shape[0]), int(d_ids.shape[1])
        check(self.L.kdb_consensus_batch_dev(self.h, _tptr(d_ids), _tptr(d_counts), B, stride, _tptr(d_queries), _tptr(d_active), 0, _tptr(d_out),
                                             _tptr(d_similarity), _tptr(d_centroid), _tptr(d_gram), C.c_void_p(stream) if stream else None),
              "kdb_consensus_batch_dev")

    def belief(self, queries, k: int, ef: int = 100, allow_bits=None, active_bits=None, trace: bool = False, fail_on_drop: bool = False,
               dist64: bool = False, tie_flag: bool = False, heap_order: bool = False):
        """The search of Engine.VBeliefState (pkg/engine/epistemic.go:45) and the consensus of its results as one call
        (kdb_belief_batch): (ids, dist, count) exactly as search_batch returns them, then rec [B] and similarity [B, k] as consensus
        returns them for (ids, count, queries, active_bits)[, (n_dist, n_hops)]"""
        self._live()
        q = np.ascontiguousarray(queries, dtype=np.float32)
        assert q.ndim == 2 and q.shape[1] == self.dim
        B = q.shape[0]
        ids = np.zeros((B, k), dtype=np.uint32)
        dist = np.full((B, k), np.inf, dtype=np.float64 if dist64 else np.float32)
        cnt = np.zeros(B, dtype=np.uint32)
        rec = np.zeros(B, dtype=CONSENSUS_DTYPE)
        sim = np.zeros((B, k), dtype=np.float64)
        ab = None if allow_bits is None else np.ascontiguousarray(allow_bits, dtype=np.uint64)
        act = None if active_bits is None else np.ascontiguousarray(active_bits, dtype=np.uint64)
        nd = nh = None
        if trace:
            nd = np.zeros(B, dtype=np.uint32)
            nh = np.zeros(B, dtype=np.uint32)
            check(self.L.kdb_search_set_trace(self.h, _ptr(nd), _ptr(nh), 0), "set_trace")
        try:
            check(self.L.kdb_belief_batch(self.h, _ptr(q), B, k, ef, _ptr(ab), _ptr(act), self._by_id_flags(fail_on_drop, dist64, tie_flag, heap_order),
                                          _ptr(ids), _ptr(dist), _ptr(cnt), _ptr(rec), _ptr(sim)), "kdb_belief_batch")
        finally:
            if trace:
                self.L.kdb_search_set_trace(self.h, None, None, 0)
        if trace:
            return ids, dist, cnt, rec, sim, (nd, nh)
        return ids, dist, cnt, rec, sim

    def belief_dev(self, d_queries, k: int, ef: int, d_out_ids, d_out_dist, d_out_count, d_out, d_similarity=None, d_allow=None, d_active=None,
                   stream=None, dist64=False, tie_flag=False, heap_order=False):
        """torch device tensors in, asynchronous on `stream` (kdb_belief_batch_dev); d_out [B, 32] uint8 as in consensus_dev"""
        self._live()
        _ready(stream)
        check(self.L.kdb_belief_batch_dev(self.h, _tptr(d_queries), int(d_queries.shape[0]), k, ef, _tptr(d_allow), _tptr(d_active),
                                          self._by_id_flags(False, dist64, tie_flag, heap_order), _tptr(d_out_ids), _tptr(d_out_dist),
                                          _tptr(d_out_count), _tptr(d_out), _tptr(d_similarity), C.c_void_p(stream) if stream else None),
              "kdb_belief_batch_dev")

    def counters(self):
        c = _lib.Counters()
        check(self.L.kdb_get_counters(self.h, C.byref(c)), "get_counters")
        return {"n_dist": int(c.n_dist), "n_hops": int(c.n_hops), "bytes": int(c.bytes),
                "kernel_ms": float(c.last_kernel_ms), "n_dropped": int(c.n_dropped), "n_tied": int(c.n_tied)}

    def launch_stats(self, last_n: int):
        arr = (_lib.Counters * last_n)()
        check(self.L.kdb_get_launch_stats(self.h, last_n, arr), "get_launch_stats")
        return [{"n_dist": int(c.n_dist), "n_hops": int(c.n_hops), "bytes": int(c.bytes),
                 "kernel_ms": float(c.last_kernel_ms), "n_dropped": int(c.n_dropped), "n_tied": int(c.n_tied)} for c in arr]

    def sync(self):
        check(self.L.kdb_index_sync(self.h), "sync")

    def probe_gather(self, n_reads: int = 4_000_000, shadow: bool = False, walk_hi: bool = False):
        """measurement hook: GB/s of a uniform random whole-row gather on this index's rows (or its half-precision copy, or --
        walk_hi -- the high walk plane: 1536-byte rows at 768 columns, KDB_ERR_UNSUPPORTED until a planes walk has made the planes)"""
        ms, nbytes = C.c_float(), C.c_uint64()
        check(self.L.kdb_probe_gather(self.h, 2 if walk_hi else 1 if shadow else 0, n_reads, C.byref(ms), C.byref(nbytes)), "kdb_probe_gather")
        return nbytes.value / (ms.value * 1e-3) / 1e9

    def poison_lds(self, pattern: int = 0):
        """test hook: every CU's LDS filled with `pattern` (0 = pseudo-random words) -- a kernel that reads LDS it never wrote shows"""
        check(self.L.kdb_probe_poison_lds(self.h, int(pattern) & 0xffffffff), "kdb_probe_poison_lds")

    LAUNCH_SHAPE_FIELDS = ("search", "prec", "metric", "nch", "bs", "vis_hash_words", "waves", "planes", "heap_pass", "heap_nch",
                           "heap_hash_words", "heap_reg_results", "heap_overlap", "grid", "lds_bytes", "B")

    def launch_shape(self, last_n: int = 1):
        """test hook: which hnsw_search_kernel instantiation (and heap-order kernel) each of the last `last_n` launches took, oldest
        first (kdb_probe_launch_shape); a list of dicts over LAUNCH_SHAPE_FIELDS, all zero for a launch that was not a graph search"""
        nw = len(self.LAUNCH_SHAPE_FIELDS)
        arr = np.zeros((last_n, nw), dtype=np.uint32)
        check(self.L.kdb_probe_launch_shape(self.h, last_n, _ptr(arr)), "kdb_probe_launch_shape")
        return [dict(zip(self.LAUNCH_SHAPE_FIELDS, (int(x) for x in row))) for row in arr]

    HEAP_PLAN_FIELDS = ("hash_words", "reg_results", "nl_c", "cap_c", "lds_bytes", "grid", "tail_bytes")

    def heap_plan(self, k: int, ef: int, B: int):
        """test hook: the plan of the heap-order pass a search of B queries with (k, ef) would launch on this index as it stands
        (kdb_probe_heap_plan) -- a dict over HEAP_PLAN_FIELDS: a tied walk's candidate heap keeps its first nl_c entries in LDS,
        the rest up to cap_c in HBM; a walk that outgrows cap_c keeps the fast walk's answer and its tie bit.  Launches nothing."""
        self._live()
        arr = np.zeros(len(self.HEAP_PLAN_FIELDS), dtype=np.uint64)
        check(self.L.kdb_probe_heap_plan(self.h, int(k), int(ef), int(B), _ptr(arr)), "kdb_probe_heap_plan")
        return dict(zip(self.HEAP_PLAN_FIELDS, (int(x) for x in arr)))

    def probe_stream(self, shadow: bool = False):
        """measurement hook: GB/s of one coalesced pass over this index's rows (or its half-precision copy)"""
        ms, nbytes = C.c_float(), C.c_uint64()
        check(self.L.kdb_probe_stream(self.h, 1 if shadow else 0, C.byref(ms), C.byref(nbytes)), "kdb_probe_stream")
        return nbytes.value / (ms.value * 1e-3) / 1e9

    def merge_topk_dev(self, G, B, k, d_in_ids, d_in_dist, d_in_count, d_id_base, d_out_ids, d_out_dist, d_out_count,
                       stream=None):
        check(self.L.kdb_merge_topk_dev(self.h, G, B, k, _tptr(d_in_ids), _tptr(d_in_dist), _tptr(d_in_count),
                                        _tptr(d_id_base), _tptr(d_out_ids), _tptr(d_out_dist), _tptr(d_out_count),
                                        C.c_void_p(stream) if stream else None), "kdb_merge_topk_dev")

    def search_batch_multi_dev(self, d_queries, k: int, ef: int, d_allow_lists, d_allow_of_query, d_out_ids, d_out_dist,
                               d_out_count, stream=None, tie_flag=False, heap_order=False):
        """heterogeneous batch: d_allow_lists [G, words] int64/uint64 dense bitsets, d_allow_of_query [B] int32
        (-1 = no filter); per query the result of search_batch with its own list"""
        self._live()
        _ready(stream)
        B = int(d_queries.shape[0])
        G, words = int(d_allow_lists.shape[0]), int(d_allow_lists.shape[1])
        check(self.L.kdb_search_batch_multi_dev(self.h, _tptr(d_queries), B, k, ef, _tptr(d_allow_lists), G, words,
                                                _tptr(d_allow_of_query), self._flags(False) | (SEARCH_TIE_FLAG if tie_flag else 0)
                                                | (SEARCH_HEAP_ORDER if heap_order else 0), _tptr(d_out_ids), _tptr(d_out_dist),
                                                _tptr(d_out_count), C.c_void_p(stream) if stream else None),
              "kdb_search_batch_multi_dev")

    def flat_scan_groups_dev(self, d_queries, k: int, group_offsets, d_allow_lists, d_out_ids, d_out_dist, d_out_count,
                             max_total_allowed: int = 0, stream=None):
        """grouped exact scan: queries [group_offsets[g], group_offsets[g+1]) use dense list g of d_allow_lists [G, words]"""
        self._live()
        _ready(stream)
        off = np.ascontiguousarray(group_offsets, dtype=np.uint32)
        B = int(d_queries.shape[0])
        G, words = int(d_allow_lists.shape[0]), int(d_allow_lists.shape[1])
        assert off.size == G + 1
        check(self.L.kdb_flat_scan_groups_dev(self.h, _tptr(d_queries), B, k, G, _ptr(off), _tptr(d_allow_lists), words,
                                              int(max_total_allowed), self._flags(False), _tptr(d_out_ids), _tptr(d_out_dist),
                                              _tptr(d_out_count), C.c_void_p(stream) if stream else None),
              "kdb_flat_scan_groups_dev")

    def merge_topk_packed_dev(self, G, B, k, d_packed, stride_words, d_id_base, d_out_ids, d_out_dist, d_out_count,
                              stream=None):
        """merge over the packed per-shard blocks (ids | dist bits | count) that one all-gather delivers"""
        check(self.L.kdb_merge_topk_packed_dev(self.h, G, B, k, _tptr(d_packed), stride_words, _tptr(d_id_base),
                                               _tptr(d_out_ids), _tptr(d_out_dist), _tptr(d_out_count),
                                               C.c_void_p(stream) if stream else None), "kdb_merge_topk_packed_dev")

    def merge_topk_packed_f64_dev(self, G, B, k, d_packed, stride_words, d_id_base, d_out_ids, d_out_dist, d_out_count, stream=None):
        """int8 shards: blocks of dist64[B][k] | ids[B][k] | count[B]; d_out_dist is a float64 tensor"""
        check(self.L.kdb_merge_topk_packed_f64_dev(self.h, G, B, k, _tptr(d_packed), stride_words, _tptr(d_id_base),
                                                   _tptr(d_out_ids), _tptr(d_out_dist), _tptr(d_out_count),
                                                   C.c_void_p(stream) if stream else None), "kdb_merge_topk_packed_f64_dev")

    # ---- metadata filters on the device (filter.hip) ------------------------------------------------
    def set_column(self, col: int, kind: int, values, first_id: int = 1):
        """Metadata column `col` (COL_F64: float64, NaN = no value; COL_CODE: uint32 dictionary codes, 0 = no value) for ids
        first_id .. first_id + len(values) - 1; a torch device tensor goes through kdb_index_set_column_dev."""
        self._live()
        if hasattr(values, "data_ptr"):
            _ready(None)
            check(self.L.kdb_index_set_column_dev(self.h, col, kind, first_id, int(values.shape[0]), _tptr(values)), "kdb_index_set_column_dev")
            return
        v = np.ascontiguousarray(values, dtype=np.float64 if kind == COL_F64 else np.uint32)
        check(self.L.kdb_index_set_column(self.h, col, kind, first_id, int(v.shape[0]), _ptr(v)), "kdb_index_set_column")

    def drop_column(self, col: int):
        self._live()
        check(self.L.kdb_index_drop_column(self.h, col), "kdb_index_drop_column")

    def column_info(self, col: int):
        """(kind, bytes) of a slot; (0, 0) when it is empty"""
        self._live()
        kind, nbytes = C.c_uint32(), C.c_uint64()
        check(self.L.kdb_index_column_info(self.h, col, C.byref(kind), C.byref(nbytes)), "kdb_index_column_info")
        return int(kind.value), int(nbytes.value)

    def filter_eval(self, programs, words_per_list: int = 0, want_lists: bool = True):
        """programs: a list of TERM_DTYPE arrays (compile_filter makes them).  Returns (lists [P, words] uint64 or None, card [P])."""
        self._live()
        terms, offs = pack_programs(programs)
        P = offs.size - 1
        words = int(words_per_list) if words_per_list else (self.graph_info()[0] >> 6) + 1
        lists = np.zeros((P, words), dtype=np.uint64) if want_lists else None
        card = np.zeros(P, dtype=np.uint32)
        check(self.L.kdb_filter_eval(self.h, _ptr(terms), _ptr(offs), P, _ptr(lists), words, _ptr(card)), "kdb_filter_eval")
        return lists, card

    def filter_eval_dev(self, programs, d_lists, d_card=None, stream=None):
        """the same into device tensors: d_lists [P, words] int64 / uint64, d_card [P] int32 or None; asynchronous on `stream`"""
        self._live()
        _ready(stream)
        terms, offs = pack_programs(programs)
        P = offs.size - 1
        assert int(d_lists.shape[0]) == P
        check(self.L.kdb_filter_eval_dev(self.h, _ptr(terms), _ptr(offs), P, _tptr(d_lists), int(d_lists.shape[1]), _tptr(d_card),
                                         C.c_void_p(stream) if stream else None), "kdb_filter_eval_dev")

    def search_filtered(self, queries, k: int, ef: int, programs, prog_of_query, flat_selectivity: float = 0.1, tie_flag=False,
                        heap_order=False):
        """Engine.VSearch with a filter as one call (kdb_search_filtered): query b uses programs[prog_of_query[b]] (NO_FILTER / -1:
        none).  Returns (ids [B, k], dist [B, k], count [B], route [B], card [P])."""
        self._live()
        q = np.ascontiguousarray(queries, dtype=np.float32)
        B = q.shape[0]
        terms, offs = pack_programs(programs)
        P = offs.size - 1
        poq = np.ascontiguousarray(np.asarray(prog_of_query, dtype=np.int64) & 0xFFFFFFFF, dtype=np.uint32)
        assert poq.size == B
        ids = np.zeros((B, k), dtype=np.uint32)
        dist = np.zeros((B, k), dtype=np.float32)
        cnt = np.zeros(B, dtype=np.uint32)
        route = np.zeros(B, dtype=np.uint8)
        card = np.zeros(P, dtype=np.uint32)
        flags = (SEARCH_NEEDS_REFINE if self.needs_refine else 0) | (SEARCH_TIE_FLAG if tie_flag else 0) | (SEARCH_HEAP_ORDER if heap_order else 0)
        check(self.L.kdb_search_filtered(self.h, _ptr(q), B, k, ef, _ptr(terms), _ptr(offs), P, _ptr(poq), float(flat_selectivity), flags,
                                         _ptr(ids), _ptr(dist), _ptr(cnt), _ptr(route), _ptr(card)), "kdb_search_filtered")
        return ids, dist, cnt, route, card

    # ---- the reference's per-query API --------------------------------------------------------------
    def score(self, raw: float) -> float:
        """The reference's f64 epilogue: float64(sum) (distance_go.go:67) / 1.0-float64(dot) (:127)."""
        if self.precision == F32 and self.metric == COSINE:
            return 1.0 - float(raw)
        return float(raw)

    def SearchWithScores(self, query, k: int, allowList=None, efSearch: int = 0) -> List[SearchResult]:
        """core.VectorIndex.SearchWithScores (pkg/core/vector_index.go:35; hnsw_index.go:343-366).
        allowList: None (nil) or a dense uint64 bitset over internal ids (the shim converts roaring)."""
        if self._closed:
            return []
        q = np.asarray(query, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.dim:
            return []  # dimension mismatch is an error of searchInternal: logged, empty slice (:356-359)
        try:
            # int8: Score is the reference's float64 distance (hnsw_index.go:2429-2454), not its float rounding
            ids, dist, cnt = self.search_batch(q[None, :], k, efSearch, allowList, dist64=(self.precision == I8))
        except KdbError:
            return []  # the reference logs and returns an empty slice (:356-359)
        n = int(cnt[0])
        return [SearchResult(int(ids[0, i]), self.score(dist[0, i])) for i in range(n)]

    def VSearchSimilar(self, ids, k: int, allowList=None, efSearch: int = 0, dropSelf: bool = False) -> List[List[SearchResult]]:
        """One page of the Gardener's loop (pkg/cognitive/gardener.go:803-869: VGetMany, then VSearchWithScores with every
        vData.Vector) as one call: per id the list SearchWithScores(GetNodeData(id).Vector, k, allowList, efSearch) returns;
        an id that is not found gets an empty list (VGetMany does not return it).  dropSelf: without the id itself."""
        a = np.ascontiguousarray(ids, dtype=np.uint32).ravel()
        if self._closed:
            return [[] for _ in range(a.size)]
        try:
            out, dist, cnt = self.search_by_id(a, k, efSearch, allowList, dist64=(self.precision == I8), drop_self=dropSelf)
        except KdbError:
            return [[] for _ in range(a.size)]  # the reference logs and returns an empty slice (:356-359)
        return [[SearchResult(int(out[b, i]), self.score(dist[b, i])) for i in range(int(cnt[b]))] for b in range(a.size)]


    def BeliefState(self, query, k: int = 10, allowList=None, activeList=None, efSearch: int = 100) -> Optional[dict]:
        """The vector half of Engine.VBeliefState (pkg/engine/epistemic.go:22-182): search (k capped at 50, ef 100), then
        CalculateConsensus over the active results.  Returns None where the reference returns an error (no candidates, no active
        node), else {"score", "variance", "sources", "nodes": [SearchResult], "similarities": [float]}.
        activeList: dense uint64 bitset of the ids that are NOT historical (None: all)."""
        if self._closed:
            return None
        if k <= 0:
            k = 10
        k = min(k, 50)
        q = np.asarray(query, dtype=np.float32)
        if q.ndim != 1 or q.shape[0] != self.dim:
            return None
        try:
            ids, dist, cnt, rec, sim = self.belief(q[None, :], k, efSearch, allowList, activeList, dist64=(self.precision == I8))
        except KdbError:
            return None
        n = int(cnt[0]) & int(COUNT_MASK)
        if n == 0 or int(rec["n_found"][0]) == 0 or int(rec["n_active"][0]) == 0:
            return None
        found = [i for i in range(n) if sim[0, i] != -1.0]
        return {"score": float(rec["score"][0]), "variance": float(rec["variance"][0]), "sources": int(rec["n_found"][0]),
                "nodes": [SearchResult(int(ids[0, i]), self.score(dist[0, i])) for i in found],
                "similarities": [float(sim[0, i]) for i in found]}


def merge_topk(metric: int, ids, dist, count, k: int, id_base=None, precision: int = F32, out=None):
    """Host shard merge through the C ABI (kdb_merge_topk): ids/dist [G,B,k], count [G,B], id_base [G].
    A count may carry COUNT_TIED (bit 31): it is not part of the length, and the merged count carries it when a shard's did.
    out: (ids [B,k] uint32, dist [B,k] float32 -- float64 for int8 doubles --, count [B] uint32) to write into instead of new arrays."""
    L = _lib.load()
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    count = np.ascontiguousarray(count, dtype=np.uint32)
    base = None if id_base is None else np.ascontiguousarray(id_base, dtype=np.uint32)
    G, B = count.shape
    if precision == I8 and np.asarray(dist).dtype == np.float64:  # int8 shards: the reference's float64 distances, ordered as doubles
        # (chosen by the index's precision, not by the array's dtype alone: a float64 array of an f32 cosine index holds DOTS --
        # it is cast to float32 and merged on the key -dot below, as before)
        dist = np.ascontiguousarray(dist, dtype=np.float64)
        o_ids, o_dist, o_cnt = out if out is not None else (np.zeros((B, k), dtype=np.uint32), np.zeros((B, k), dtype=np.float64),
                                                            np.zeros(B, dtype=np.uint32))
        assert o_ids.dtype == np.uint32 and o_dist.dtype == np.float64 and o_cnt.dtype == np.uint32 and o_dist.shape == (B, k)
        check(L.kdb_merge_topk_f64(G, B, k, _ptr(ids), _ptr(dist), _ptr(count), _ptr(base), _ptr(o_ids), _ptr(o_dist), _ptr(o_cnt)), "kdb_merge_topk_f64")
        return o_ids, o_dist, o_cnt
    dist = np.ascontiguousarray(dist, dtype=np.float32)
    o_ids, o_dist, o_cnt = out if out is not None else (np.zeros((B, k), dtype=np.uint32), np.zeros((B, k), dtype=np.float32),
                                                        np.zeros(B, dtype=np.uint32))
    assert o_ids.dtype == np.uint32 and o_dist.dtype == np.float32 and o_cnt.dtype == np.uint32 and o_dist.shape == (B, k)
    check(L.kdb_merge_topk(metric, precision, G, B, k, _ptr(ids), _ptr(dist), _ptr(count), _ptr(base), _ptr(o_ids),
                           _ptr(o_dist), _ptr(o_cnt)), "kdb_merge_topk")
    return o_ids, o_dist, o_cnt


def arena_read_rows(arena_dir: str, dim: int, precision: int, first_id: int, n: int, slot_table=None) -> np.ndarray:
    """host-only reader of the reference's arena files (kdb_arena_read_rows)."""
    L = _lib.load()
    out = np.zeros((n, dim), dtype=_ELEM[precision])
    st = None if slot_table is None else np.ascontiguousarray(slot_table, dtype=np.uint32)
    check(L.kdb_arena_read_rows(arena_dir.encode(), dim, precision, _ptr(st), first_id, n, _ptr(out)), "arena_read_rows")
    return out


def dense_bitset(ids: Sequence[int], count: int) -> np.ndarray:
    """roaring.Bitmap -> dense uint64 words ((count>>6)+1), the form the allow-list crosses the ABI in."""
    w = np.zeros((count >> 6) + 1, dtype=np.uint64)
    a = np.asarray(list(ids), dtype=np.uint64)
    if a.size:
        np.bitwise_or.at(w, (a >> np.uint64(6)).astype(np.int64), np.uint64(1) << (a & np.uint64(63)))
    return w


def pack_programs(programs):
    """a list of TERM_DTYPE arrays -> (terms, prog_offsets) as kdb_filter_eval takes them"""
    progs = [np.ascontiguousarray(p, dtype=TERM_DTYPE).reshape(-1) for p in programs]
    offs = np.zeros(len(progs) + 1, dtype=np.uint32)
    if progs:
        offs[1:] = np.cumsum([p.size for p in progs])
    terms = np.concatenate(progs) if progs else np.zeros(0, dtype=TERM_DTYPE)
    if terms.size == 0:
        terms = np.zeros(1, dtype=TERM_DTYPE)  # (a pointer the library may refuse by its own rules, not a null one)
    return np.ascontiguousarray(terms), offs


def parse_filter(filter: str):
    """kdb_filter_parse (host only, no GPU needed): the atoms of a filter string, in order, as dicts
    {key, value, op (FA_*), is_numeric, number, end_block}.  Raises KdbError as the reference returns an error."""
    L = _lib.load()
    raw = filter.encode("utf-8")
    n = C.c_uint32()
    check(L.kdb_filter_parse(raw, None, 0, C.byref(n)), "kdb_filter_parse")
    atoms = (_lib.FilterAtom * max(1, n.value))()
    check(L.kdb_filter_parse(raw, C.cast(atoms, C.c_void_p), n.value, C.byref(n)), "kdb_filter_parse")
    out = []
    for a in atoms[:n.value]:
        out.append({"key": raw[a.key_off:a.key_off + a.key_len].decode("utf-8", "replace"),
                    "value": raw[a.val_off:a.val_off + a.val_len].decode("utf-8", "replace"), "op": int(a.op),
                    "is_numeric": bool(a.is_numeric), "number": float(a.number), "end_block": bool(a.flags & FT_END_BLOCK)})
    return out


def compile_filter(filter: str, schema: dict) -> np.ndarray:
    """A filter string -> one predicate program (TERM_DTYPE array) for this schema:
        schema[key] = {"f64": slot or None, "code": slot or None, "dict": {string value: code >= 1}}
    -- the key's numeric column (the reference's B-tree) and / or its code column with the caller's dictionary (its inverted index).
    `k = v`: F64_EQ if v is numeric and k has a numeric column, CODE_EQ if k has a code column and the dictionary knows v (the lenient
    union of core.go:1933-1944), NEVER if neither; `k != v` the same with NOT; a range operator is one F64 term, NEVER without a
    numeric column.  A filter whose blocks are all empty ("AND OR AND" never gets this far: it has no operator) compiles to NEVER."""
    terms = []
    for a in parse_filter(filter):
        sch = schema.get(a["key"]) or {}
        f64, code = sch.get("f64"), sch.get("code")
        alts = []
        if a["op"] in (FA_EQ, FA_NE):
            if a["is_numeric"] and f64 is not None:
                alts.append((FOP_F64_EQ, f64, 0, a["number"]))
            c = (sch.get("dict") or {}).get(a["value"]) if code is not None else None
            if c:
                alts.append((FOP_CODE_EQ, code, int(c), 0.0))
        elif f64 is not None:
            alts.append(({FA_LT: FOP_F64_LT, FA_LE: FOP_F64_LE, FA_GT: FOP_F64_GT, FA_GE: FOP_F64_GE}[a["op"]], f64, 0, a["number"]))
        if not alts:
            alts.append((FOP_NEVER, 0, 0, 0.0))
        for i, (op, col, c, val) in enumerate(alts):
            fl = (FT_OR_NEXT if i + 1 < len(alts) else 0) | (FT_NOT if i == 0 and a["op"] == FA_NE else 0)
            if i + 1 == len(alts) and a["end_block"]:
                fl |= FT_END_BLOCK
            terms.append((op, fl, col, c, val))
    if not terms:
        terms.append((FOP_NEVER, FT_END_BLOCK, 0, 0, 0.0))
    if len(terms) > FILTER_MAX_TERMS:
        raise KdbError(f"compile_filter: {len(terms)} terms, a program holds at most {FILTER_MAX_TERMS}")
    return np.array(terms, dtype=TERM_DTYPE)
