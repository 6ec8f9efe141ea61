// kdb_api_graph.hip -- host side of the C ABI (include/kektor_hip.h): the graph mirror -- upload, incremental refresh, download -- and
// the entry points of the builders (build.hip, add.hip, refine.hip), which run under KdbWriteLock on the index's own stream.
#include "kdb_internal.h"
#include "kdb_host.h"
#include <string.h>

extern "C" int kdb_index_upload_graph(kdb_index *idx, const kdb_graph_view *g) {
    KDB_CHECK_IDX(idx);
    if (!g || g->count > idx->cap || (g->count && (!g->levels || !g->offsets || !g->neighbors))) {
        kdb_set_error("upload_graph: bad graph view (count %u, capacity %u)", g ? g->count : 0, idx->cap);
        return KDB_ERR_INVALID;
    }
    if (g->max_level >= 0 && (g->entry == 0 || g->entry > g->count)) {
        kdb_set_error("upload_graph: entry point %u outside 1..%u", g->entry, g->count);
        return KDB_ERR_INVALID;
    }
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    idx->graph_epoch++; // (every writer of levels / up_idx / upper lists: the derived slot table is rebuilt by the next search)
    KDB_HIP(hipSetDevice(idx->device));
    const uint32_t n = g->count;
    const size_t n1 = (size_t)n + 1;
    std::vector<uint32_t> adj0(n1 * idx->deg0, 0u);
    std::vector<uint32_t> up_idx(n1, 0u);
    std::vector<uint8_t> levels(n1, 0);
    size_t slots = 0;
    for (uint32_t i = 1; i <= n; i++) {
        int lv = g->levels[i];
        if (lv > g->max_level) lv = g->max_level < 0 ? 0 : g->max_level;
        levels[i] = (uint8_t)lv;
        up_idx[i] = (uint32_t)slots;
        slots += (size_t)lv;
    }
    std::vector<uint32_t> adj_up(slots * idx->deg_up + 1, 0u);
    for (int l = 0; l <= g->max_level; l++) {
        const uint64_t *off = g->offsets[l];
        const uint32_t *nb = g->neighbors[l];
        const uint32_t cap = l == 0 ? idx->deg0 : idx->deg_up;
        for (uint32_t i = 1; i <= n; i++) {
            if ((int)levels[i] < l) continue;
            const uint64_t a = off[i], b = off[i + 1];
            if (b - a > cap) {
                kdb_set_error("upload_graph: node %u has %llu links at level %d (cap %u)", i, (unsigned long long)(b - a), l, cap);
                return KDB_ERR_INVALID;
            }
            uint32_t *dst = l == 0 ? &adj0[(size_t)i * idx->deg0] : &adj_up[((size_t)up_idx[i] + (size_t)(l - 1)) * idx->deg_up];
            for (uint64_t e = a; e < b; e++) {
                if (nb[e] == 0 || nb[e] > n) {
                    kdb_set_error("upload_graph: neighbour id %u of node %u out of range", nb[e], i);
                    return KDB_ERR_INVALID;
                }
                dst[e - a] = nb[e];
            }
        }
    }
    if (slots > idx->up_slots_cap) {
        if (idx->d_adj_up) {
            KDB_HIP(hipDeviceSynchronize()); // walks of callers' streams may still read the old pool
            KDB_HIP(hipFree(idx->d_adj_up));
        }
        idx->d_adj_up = nullptr;
        KDB_HIP(hipMalloc(&idx->d_adj_up, (slots * idx->deg_up + 1) * 4));
        idx->up_slots_cap = slots;
    } else if (!idx->d_adj_up) {
        KDB_HIP(hipMalloc(&idx->d_adj_up, 4 * (size_t)idx->deg_up + 4));
    }
    idx->up_slots = slots;
    KDB_HIP(hipMemcpyAsync(idx->d_adj0, adj0.data(), adj0.size() * 4, hipMemcpyHostToDevice, idx->stream));
    if (slots) KDB_HIP(hipMemcpyAsync(idx->d_adj_up, adj_up.data(), slots * idx->deg_up * 4, hipMemcpyHostToDevice, idx->stream));
    KDB_HIP(hipMemcpyAsync(idx->d_up_idx, up_idx.data(), n1 * 4, hipMemcpyHostToDevice, idx->stream));
    KDB_HIP(hipMemcpyAsync(idx->d_levels, levels.data(), n1, hipMemcpyHostToDevice, idx->stream));
    // deleted bits: uint64 words, bit id -> uint32 words (little endian: same bytes)
    const size_t dw32 = ((n1 + 31) / 32 + 3) & ~(size_t)3;
    std::vector<uint32_t> del(dw32, 0u);
    uint32_t ndel = 0;
    if (g->deleted_bits) {
        for (uint32_t i = 1; i <= n; i++)
            if ((g->deleted_bits[i >> 6] >> (i & 63)) & 1ull) {
                del[i >> 5] |= 1u << (i & 31);
                ndel++;
            }
    }
    KDB_HIP(hipMemcpyAsync(idx->d_deleted, del.data(), dw32 * 4, hipMemcpyHostToDevice, idx->stream));
    KDB_HIP(hipStreamSynchronize(idx->stream));
    idx->n_deleted = ndel;
    idx->count = n;
    idx->entry = g->entry;
    idx->max_level = g->max_level;
    idx->has_graph = true;
    idx->h_levels = std::move(levels);
    idx->h_up_idx = std::move(up_idx);
    return KDB_OK;
}

// ---------------------------------------------------------------------------------------------
// Incremental refresh of the mirror (writers touched a few nodes: no full re-upload)
// ---------------------------------------------------------------------------------------------
extern "C" int kdb_index_append_nodes(kdb_index *idx, uint32_t first_id, uint32_t n, const uint8_t *levels) {
    KDB_CHECK_IDX(idx);
    if (n == 0) return KDB_OK;
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    if (!levels || first_id != idx->count + 1 || (uint64_t)first_id + n - 1 > idx->cap) {
        kdb_set_error("append_nodes: ids must continue at count+1 = %u and stay within capacity %u", idx->count + 1, idx->cap);
        return KDB_ERR_INVALID;
    }
    if (idx->h_levels.size() != (size_t)idx->count + 1) {
        if (idx->count != 0) {
            kdb_set_error("append_nodes: the index holds no host-side level table (upload or build a graph first, or start empty)");
            return KDB_ERR_STATE;
        }
        idx->h_levels.assign(1, 0);
        idx->h_up_idx.assign(1, 0);
    }
    KDB_HIP(hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    size_t slots = idx->up_slots;
    // the derived upper-slot table (kdb_ensure_up_slots) is a function of levels / up_idx / the upper lists: nodes that
    // only exist at level 0 change none of its inputs, so the first search after such an append pays no rebuild
    for (uint32_t i = 0; i < n; i++)
        if (levels[i]) {
            idx->graph_epoch++;
            break;
        }
    std::vector<uint32_t> up_new(n);
    for (uint32_t i = 0; i < n; i++) {
        up_new[i] = (uint32_t)slots;
        slots += levels[i];
    }
    if (slots > idx->up_slots_cap || !idx->d_adj_up) { // grow the upper pool, keep what it holds
        const size_t ncap = slots + slots / 2 + 1024;
        uint32_t *nbuf = nullptr;
        KDB_HIP(hipMalloc(&nbuf, (ncap * idx->deg_up + 1) * 4));
        KDB_HIP(hipMemsetAsync(nbuf, 0, (ncap * idx->deg_up + 1) * 4, s));
        if (idx->d_adj_up && idx->up_slots)
            KDB_HIP(hipMemcpyAsync(nbuf, idx->d_adj_up, idx->up_slots * idx->deg_up * 4, hipMemcpyDeviceToDevice, s));
        KDB_HIP(hipStreamSynchronize(s));
        if (idx->d_adj_up) KDB_HIP(hipFree(idx->d_adj_up));
        idx->d_adj_up = nbuf;
        idx->up_slots_cap = ncap;
    } else { // recycled pool memory: the new nodes' upper rows start empty
        KDB_HIP(hipMemsetAsync(idx->d_adj_up + idx->up_slots * idx->deg_up, 0, (slots - idx->up_slots) * idx->deg_up * 4, s));
    }
    KDB_HIP(hipMemsetAsync(idx->d_adj0 + (size_t)first_id * idx->deg0, 0, (size_t)n * idx->deg0 * 4, s));
    KDB_HIP(hipMemcpyAsync(idx->d_levels + first_id, levels, n, hipMemcpyHostToDevice, s));
    KDB_HIP(hipMemcpyAsync(idx->d_up_idx + first_id, up_new.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    KDB_HIP(hipStreamSynchronize(s));
    idx->h_levels.insert(idx->h_levels.end(), levels, levels + n);
    idx->h_up_idx.insert(idx->h_up_idx.end(), up_new.begin(), up_new.end());
    idx->up_slots = slots;
    idx->count += n;
    return KDB_OK;
}

extern "C" int kdb_index_patch_adjacency(kdb_index *idx, uint32_t level, uint32_t n, const uint32_t *ids,
                                         const uint64_t *offsets, const uint32_t *neighbors) {
    KDB_CHECK_IDX(idx);
    if (n == 0) return KDB_OK;
    if (!ids || !offsets || (!neighbors && offsets[n] != offsets[0])) {
        kdb_set_error("patch_adjacency: null buffer");
        return KDB_ERR_INVALID;
    }
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    if (level >= 1) idx->graph_epoch++; // level-0 lists are no input of the derived upper-slot table
    if (idx->h_levels.size() != (size_t)idx->count + 1) {
        kdb_set_error("patch_adjacency: no graph to patch");
        return KDB_ERR_STATE;
    }
    const uint32_t deg = level == 0 ? idx->deg0 : idx->deg_up;
    std::vector<uint32_t> rows((size_t)n * deg, 0u), slots(n);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t id = ids[i];
        if (id == 0 || id > idx->count || idx->h_levels[id] < level) {
            kdb_set_error("patch_adjacency: node %u does not exist at level %u", id, level);
            return KDB_ERR_INVALID;
        }
        const uint64_t a = offsets[i], b = offsets[i + 1];
        if (b < a || b - a > deg) {
            kdb_set_error("patch_adjacency: node %u has %llu links at level %u (cap %u)", id, (unsigned long long)(b - a), level, deg);
            return KDB_ERR_INVALID;
        }
        for (uint64_t e = a; e < b; e++) {
            if (neighbors[e] == 0 || neighbors[e] > idx->count) {
                kdb_set_error("patch_adjacency: neighbour id %u of node %u out of range", neighbors[e], id);
                return KDB_ERR_INVALID;
            }
            rows[(size_t)i * deg + (e - a)] = neighbors[e];
        }
        slots[i] = level == 0 ? id : idx->h_up_idx[id] + (level - 1);
    }
    KDB_HIP(hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    KdbLaneGuard lane(idx, s);
    if (lane.rc) return lane.rc;
    KdbCarver cv;
    const size_t o_rows = cv.take(rows.size() * 4), o_slots = cv.take((size_t)n * 4);
    int rc = kdb_ensure_scratch(idx, cv.total() + 256);
    if (rc) return rc;
    unsigned char *const b = reinterpret_cast<unsigned char *>(kdb_cur(idx).d_scratch);
    uint32_t *d_rows = reinterpret_cast<uint32_t *>(b + o_rows), *d_slots = reinterpret_cast<uint32_t *>(b + o_slots);
    KDB_HIP(hipMemcpyAsync(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, s));
    KDB_HIP(hipMemcpyAsync(d_slots, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    rc = kdb_launch_adj_scatter(level == 0 ? idx->d_adj0 : idx->d_adj_up, deg, n, d_slots, d_rows, s);
    if (rc) return rc;
    KDB_HIP(hipStreamSynchronize(s)); // host buffers are consumed before returning
    return KDB_OK;
}

extern "C" int kdb_index_set_entry(kdb_index *idx, uint32_t entry, int32_t max_level) {
    KDB_CHECK_IDX(idx);
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    if (max_level >= 0 && (entry == 0 || entry > idx->count)) {
        kdb_set_error("set_entry: entry point %u outside 1..%u", entry, idx->count);
        return KDB_ERR_INVALID;
    }
    if (max_level >= 0 && idx->h_levels.size() == (size_t)idx->count + 1 && (int)idx->h_levels[entry] < max_level) {
        kdb_set_error("set_entry: node %u has level %u < max_level %d", entry, idx->h_levels[entry], max_level);
        return KDB_ERR_INVALID;
    }
    idx->entry = entry;
    idx->max_level = max_level;
    idx->has_graph = max_level >= 0;
    return KDB_OK;
}

extern "C" int kdb_index_mark_deleted(kdb_index *idx, const uint32_t *ids, uint32_t n) {
    KDB_CHECK_IDX(idx);
    if (n == 0) return KDB_OK;
    if (!ids) return KDB_ERR_INVALID;
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    KDB_HIP(hipSetDevice(idx->device));
    const size_t n1 = (size_t)idx->cap + 1;
    const size_t dw32 = ((n1 + 31) / 32 + 3) & ~(size_t)3;
    std::vector<uint32_t> del(dw32);
    KDB_HIP(hipMemcpyAsync(del.data(), idx->d_deleted, dw32 * 4, hipMemcpyDeviceToHost, idx->stream));
    KDB_HIP(hipStreamSynchronize(idx->stream));
    for (uint32_t i = 0; i < n; i++) {
        if (ids[i] == 0 || ids[i] > idx->count) continue;
        uint32_t &w = del[ids[i] >> 5];
        if (!(w & (1u << (ids[i] & 31)))) {
            w |= 1u << (ids[i] & 31);
            idx->n_deleted++;
        }
    }
    KDB_HIP(hipMemcpyAsync(idx->d_deleted, del.data(), dw32 * 4, hipMemcpyHostToDevice, idx->stream));
    KDB_HIP(hipStreamSynchronize(idx->stream));
    return KDB_OK;
}

extern "C" int kdb_index_graph_info(kdb_index *idx, uint32_t *count, uint32_t *entry, int32_t *max_level) {
    KDB_CHECK_IDX(idx);
    if (count) *count = idx->count;
    if (entry) *entry = idx->entry;
    if (max_level) *max_level = idx->max_level;
    return KDB_OK;
}

extern "C" int kdb_index_download_graph(kdb_index *idx, uint8_t *levels, uint64_t *const *offsets,
                                        uint32_t *const *neighbors, uint64_t *level_sizes) {
    KDB_CHECK_IDX(idx);
    if (!idx->has_graph) {
        kdb_set_error("download_graph: no graph present");
        return KDB_ERR_STATE;
    }
    std::lock_guard<std::mutex> lk(idx->mu);
    KDB_HIP(hipSetDevice(idx->device));
    const uint32_t n = idx->count;
    const size_t n1 = (size_t)n + 1;
    std::vector<uint32_t> adj0(n1 * idx->deg0), up_idx(n1), adj_up(idx->up_slots * idx->deg_up + 1);
    std::vector<uint8_t> lv(n1);
    KDB_HIP(hipMemcpyAsync(adj0.data(), idx->d_adj0, adj0.size() * 4, hipMemcpyDeviceToHost, idx->stream));
    KDB_HIP(hipMemcpyAsync(up_idx.data(), idx->d_up_idx, n1 * 4, hipMemcpyDeviceToHost, idx->stream));
    KDB_HIP(hipMemcpyAsync(lv.data(), idx->d_levels, n1, hipMemcpyDeviceToHost, idx->stream));
    if (idx->up_slots)
        KDB_HIP(hipMemcpyAsync(adj_up.data(), idx->d_adj_up, idx->up_slots * idx->deg_up * 4, hipMemcpyDeviceToHost, idx->stream));
    KDB_HIP(hipStreamSynchronize(idx->stream));
    if (levels) memcpy(levels, lv.data(), n1);
    for (int l = 0; l <= idx->max_level; l++) {
        uint64_t tot = 0;
        const uint32_t cap = l == 0 ? idx->deg0 : idx->deg_up;
        for (uint32_t i = 0; i <= n; i++) {
            if (offsets && offsets[l]) offsets[l][i] = tot;
            if (i == 0 || (int)lv[i] < l) continue;
            const uint32_t *src = l == 0 ? &adj0[(size_t)i * idx->deg0] : &adj_up[((size_t)up_idx[i] + (size_t)(l - 1)) * idx->deg_up];
            for (uint32_t e = 0; e < cap && src[e] != 0; e++) {
                if (neighbors && neighbors[l]) neighbors[l][tot] = src[e];
                tot++;
            }
        }
        if (offsets && offsets[l]) offsets[l][n + 1] = tot;
        if (level_sizes) level_sizes[l] = tot;
    }
    return KDB_OK;
}

extern "C" int kdb_index_build(kdb_index *idx, uint32_t count, const kdb_build_params *params) {
    KDB_CHECK_IDX(idx);
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    idx->graph_epoch++;
    KDB_HIP(hipSetDevice(idx->device));
    KdbLaneGuard lane(idx, idx->stream);
    if (lane.rc) return lane.rc;
    return kdb_build_graph(idx, count, params);
}

extern "C" int kdb_index_add_batch(kdb_index *idx, uint32_t first_id, uint32_t n, const uint8_t *levels, uint32_t ef_construction,
                                   uint32_t flags) {
    KDB_CHECK_IDX(idx);
    if (flags & ~KDB_ADD_REFERENCE_LINKS) {
        kdb_set_error("add_batch: unknown flag");
        return KDB_ERR_INVALID;
    }
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    idx->graph_epoch++;
    KDB_HIP(hipSetDevice(idx->device));
    KdbLaneGuard lane(idx, idx->stream);
    if (lane.rc) return lane.rc;
    return kdb_add_batch_ref(idx, first_id, n, levels, ef_construction);
}

extern "C" int kdb_index_add(kdb_index *idx, uint32_t first_id, uint32_t n, const uint8_t *levels, const kdb_add_params *params, kdb_add_stats *out) {
    KDB_CHECK_IDX(idx);
    if (params && params->flags) {
        kdb_set_error("add: unknown flag");
        return KDB_ERR_INVALID;
    }
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    // (graph_epoch: bumped by kdb_add_graph, and only when a new node has an upper level -- as kdb_index_append_nodes does it, so that
    // the first search after a level-0 insert pays no rebuild of the derived upper-slot table; a refused call touches nothing)
    KDB_HIP(hipSetDevice(idx->device));
    KdbLaneGuard lane(idx, idx->stream);
    if (lane.rc) return lane.rc;
    return kdb_add_graph(idx, first_id, n, levels, params ? params->ef_construction : 0u, out);
}

extern "C" int kdb_index_refine(kdb_index *idx, const uint32_t *ids, uint32_t n, const kdb_refine_params *params, kdb_refine_stats *out) {
    KDB_CHECK_IDX(idx);
    if (params && params->flags) {
        kdb_set_error("refine: unknown flag");
        return KDB_ERR_INVALID;
    }
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    idx->graph_epoch++;
    KDB_HIP(hipSetDevice(idx->device));
    KdbLaneGuard lane(idx, idx->stream);
    if (lane.rc) return lane.rc;
    return kdb_refine_graph(idx, ids, n, params ? params->ef_construction : 0u, params ? params->chunk_nodes : 0u, out);
}

extern "C" int kdb_index_vacuum(kdb_index *idx, const kdb_vacuum_params *params, kdb_vacuum_stats *out) {
    KDB_CHECK_IDX(idx);
    if (params && (params->flags & ~KDB_VACUUM_ELECT_TOP_LEVEL)) {
        kdb_set_error("vacuum: unknown flag");
        return KDB_ERR_INVALID;
    }
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    idx->graph_epoch++;
    KDB_HIP(hipSetDevice(idx->device));
    KdbLaneGuard lane(idx, idx->stream);
    if (lane.rc) return lane.rc;
    return kdb_vacuum_graph(idx, params ? params->ef_construction : 0u, params ? params->flags : 0u, params ? params->chunk_nodes : 0u, out);
}

extern "C" int kdb_index_dead_link_scan(kdb_index *idx, uint32_t *out_ids, uint32_t cap, uint32_t *n_nodes, uint64_t *n_dead_links, uint64_t *n_dead) {
    KDB_CHECK_IDX(idx);
    KdbWriteLock wl(idx); // writes nothing, but shares the index's stream and scratch with the writers
    KDB_HIP(hipSetDevice(idx->device));
    KdbLaneGuard lane(idx, idx->stream);
    if (lane.rc) return lane.rc;
    return kdb_dead_link_scan_graph(idx, out_ids, cap, n_nodes, n_dead_links, n_dead);
}

// test hook (see kektor_hip.h): host buffers in, selections out
extern "C" int kdb_test_select_neighbors(kdb_index *idx, uint32_t n_lists, uint32_t stride, const uint32_t *cand_ids,
                                         const void *cand_keys, const uint32_t *cand_cnt, uint32_t maxm, uint32_t *out_ids,
                                         uint32_t *out_cnt) {
    KDB_CHECK_IDX(idx);
    if (n_lists == 0) return KDB_OK;
    if (!cand_ids || !cand_keys || !cand_cnt || !out_ids || !out_cnt || stride == 0) {
        kdb_set_error("test_select_neighbors: null buffer");
        return KDB_ERR_INVALID;
    }
    for (uint32_t t = 0; t < n_lists; t++) {
        if (cand_cnt[t] > stride) {
            kdb_set_error("test_select_neighbors: list %u holds %u > stride %u entries", t, cand_cnt[t], stride);
            return KDB_ERR_INVALID;
        }
        for (uint32_t i = 0; i < cand_cnt[t]; i++)
            if (cand_ids[(size_t)t * stride + i] == 0 || cand_ids[(size_t)t * stride + i] > idx->cap) {
                kdb_set_error("test_select_neighbors: candidate id out of range");
                return KDB_ERR_INVALID;
            }
    }
    DevCall call(idx, nullptr);
    if (call.rc) return call.rc;
    hipStream_t s = call.s;
    const size_t nb = (size_t)n_lists * stride * 4;
    const size_t kb = (size_t)n_lists * stride * (idx->desc.precision == KDB_PREC_I8 ? 8 : 4); // int8: float64 distances
    KdbCarver cv;
    const size_t o_keys = cv.take(kb), o_ids = cv.take(nb), o_cnt = cv.take((size_t)n_lists * 4), o_ocnt = cv.take((size_t)n_lists * 4), // (8-byte keys first)
                 o_oid = cv.take((size_t)n_lists * maxm * 4);
    int rc = kdb_ensure_scratch(idx, cv.total() + 256);
    if (rc) return rc;
    unsigned char *b = reinterpret_cast<unsigned char *>(kdb_cur(idx).d_scratch);
    void *d_keys = b + o_keys;
    uint32_t *d_ids = reinterpret_cast<uint32_t *>(b + o_ids);
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(b + o_cnt);
    uint32_t *d_ocnt = reinterpret_cast<uint32_t *>(b + o_ocnt);
    uint32_t *d_oid = reinterpret_cast<uint32_t *>(b + o_oid);
    KDB_HIP(hipMemcpyAsync(d_ids, cand_ids, nb, hipMemcpyHostToDevice, s));
    KDB_HIP(hipMemcpyAsync(d_keys, cand_keys, kb, hipMemcpyHostToDevice, s));
    KDB_HIP(hipMemcpyAsync(d_cnt, cand_cnt, (size_t)n_lists * 4, hipMemcpyHostToDevice, s));
    rc = kdb_select_probe(idx, n_lists, stride, d_ids, d_keys, d_cnt, maxm, d_oid, d_ocnt, s);
    if (rc) return rc;
    KDB_HIP(hipMemcpyAsync(out_ids, d_oid, (size_t)n_lists * maxm * 4, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipMemcpyAsync(out_cnt, d_ocnt, (size_t)n_lists * 4, hipMemcpyDeviceToHost, s));
    KDB_HIP(hipStreamSynchronize(s));
    return KDB_OK;
}
