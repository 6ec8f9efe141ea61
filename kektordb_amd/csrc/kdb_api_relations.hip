// kdb_api_relations.hip -- host side of the C ABI (include/kektor_hip.h): the relation snapshot, graph filters and subgraph extraction.
#include "kdb_internal.h"
#include "kdb_host.h"
#include "kdb_subgraph_plan.h"
#include <algorithm>
#include <vector>

// ---------------------------------------------------------------------------------------------
// The relation graph in HBM (graph_filter.hip, kdb_graph_plan.h): the active out-edges of pkg/core/graph.go as a CSR over graph nodes
// and, built here, its transpose -- both in ONE allocation.  Everything a call can judge without the index is judged BEFORE the
// handle is looked at, so the checks run -- and are tested -- on a machine without a device.
// ---------------------------------------------------------------------------------------------
extern "C" int kdb_index_set_relations(kdb_index *idx, const kdb_relations_view *v) {
    uint64_t bad = 0;
    const int vrc = kdb_graph_validate_view(v, &bad);
    if (vrc) {
        kdb_set_error("set_relations: %s (at %llu)", kdb_graph_strerror(vrc), (unsigned long long)bad);
        return KDB_ERR_INVALID;
    }
    KDB_CHECK_IDX(idx);
    const uint64_t N = v->n_nodes, E = v->off[N + 1u];
    // the in-lists: a counting sort of the edges by destination, stable, so a node's in-edges keep the order of their sources
    std::vector<uint64_t> in_off(N + 2u, 0);
    for (uint64_t e = 0; e < E; e++) in_off[(uint64_t)v->dst[e] + 1u]++;
    for (uint64_t g = 1; g <= N + 1u; g++) in_off[g] += in_off[g - 1u];
    std::vector<uint32_t> in_dst(E);
    std::vector<uint8_t> in_rel(E);
    {
        std::vector<uint64_t> at(in_off.begin(), in_off.end() - 1);
        for (uint64_t g = 1; g <= N; g++)
            for (uint64_t e = v->off[g]; e < v->off[g + 1u]; e++) {
                const uint64_t p = at[v->dst[e]]++;
                in_dst[p] = (uint32_t)g;
                in_rel[p] = v->rel[e];
            }
    }
    KdbCarver cv; // out: off | dst | rel, then in: off | dst | rel
    const size_t ob = (size_t)(N + 2u) * 8, o_off0 = cv.take(ob), o_dst0 = cv.take((size_t)E * 4), o_rel0 = cv.take((size_t)E), o_off1 = cv.take(ob),
                 o_dst1 = cv.take((size_t)E * 4), o_rel1 = cv.take((size_t)E);
    KdbWriteLock wl(idx); // excludes host-pointer calls in flight
    KDB_HIP(hipSetDevice(idx->device));
    hipStream_t s = idx->stream;
    unsigned char *p = nullptr;
    KDB_HIP(hipMalloc(reinterpret_cast<void **>(&p), cv.total()));
    hipError_t e = hipMemcpyAsync(p + o_off0, v->off, ob, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p + o_off1, in_off.data(), ob, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && E) e = hipMemcpyAsync(p + o_dst0, v->dst, (size_t)E * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && E) e = hipMemcpyAsync(p + o_rel0, v->rel, (size_t)E, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && E) e = hipMemcpyAsync(p + o_dst1, in_dst.data(), (size_t)E * 4, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && E) e = hipMemcpyAsync(p + o_rel1, in_rel.data(), (size_t)E, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s); // host values are consumed
    if (e == hipSuccess) e = hipDeviceSynchronize();  // level kernels of callers' streams may still read the snapshot this one replaces
    if (e != hipSuccess) {
        (void)hipFree(p);
        kdb_set_error("set_relations: upload failed: %s", hipGetErrorString(e));
        return KDB_ERR_HIP;
    }
    kdb_rel_slot &sl = idx->relations;
    if (sl.blob) (void)hipFree(sl.blob);
    sl = kdb_rel_slot{};
    sl.blob = p;
    sl.dev.off[0] = reinterpret_cast<const uint64_t *>(p + o_off0), sl.dev.off[1] = reinterpret_cast<const uint64_t *>(p + o_off1);
    sl.dev.dst[0] = reinterpret_cast<const uint32_t *>(p + o_dst0), sl.dev.dst[1] = reinterpret_cast<const uint32_t *>(p + o_dst1);
    sl.dev.rel[0] = p + o_rel0, sl.dev.rel[1] = p + o_rel1;
    sl.dev.n_nodes = v->n_nodes;
    sl.n_edges = E;
    sl.bytes = cv.total();
    return KDB_OK;
}

extern "C" int kdb_index_drop_relations(kdb_index *idx) {
    KDB_CHECK_IDX(idx);
    KdbWriteLock wl(idx);
    kdb_rel_slot &sl = idx->relations;
    if (!sl.blob) return KDB_OK;
    KDB_HIP(hipSetDevice(idx->device));
    KDB_HIP(hipDeviceSynchronize()); // level kernels of callers' streams may still read the snapshot
    (void)hipFree(sl.blob);
    sl = kdb_rel_slot{};
    return KDB_OK;
}

extern "C" int kdb_index_relations_info(kdb_index *idx, uint32_t *n_nodes, uint64_t *n_edges, uint64_t *bytes) {
    KDB_CHECK_IDX(idx);
    std::lock_guard<std::mutex> lk(idx->mu);
    const kdb_rel_slot &sl = idx->relations;
    if (n_nodes) *n_nodes = sl.dev.n_nodes;
    if (n_edges) *n_edges = sl.n_edges;
    if (bytes) *bytes = sl.bytes;
    return KDB_OK;
}

// ---------------------------------------------------------------------------------------------
// resolveGraphFilter for B queries (graph_filter.hip).  The queries are a host array in both forms: the launcher stages them, with the
// frontier bitmaps, in the scratch of the call's lane.
// ---------------------------------------------------------------------------------------------
// what needs no index (n_nodes = 0xffffffff: every root passes), and under idx->mu what needs the snapshot and the count
static int graph_queries_check(const kdb_graph_query *queries, uint32_t B, uint32_t n_nodes, const void *and_lists, uint32_t n_and_lists,
                               const uint32_t *and_of_query) {
    if ((and_lists != nullptr) != (and_of_query != nullptr)) {
        kdb_set_error("graph_filter_eval: and_lists and and_of_query go together");
        return KDB_ERR_INVALID;
    }
    uint32_t bad = 0;
    const int vrc = kdb_graph_validate_queries(queries, B, n_nodes, and_of_query, n_and_lists, &bad);
    if (vrc) {
        kdb_set_error("graph_filter_eval: %s (query %u)", kdb_graph_strerror(vrc), bad);
        return KDB_ERR_INVALID;
    }
    return KDB_OK;
}
static int graph_call_check(const kdb_index *idx, const kdb_graph_query *queries, uint32_t B, uint64_t words_per_list, const void *and_lists,
                            uint32_t n_and_lists, const uint32_t *and_of_query) {
    if (!idx->relations.blob) {
        kdb_set_error("graph_filter_eval: the index holds no relation snapshot (kdb_index_set_relations)");
        return KDB_ERR_INVALID;
    }
    const uint64_t least = kdb_graph_min_words(idx->count, idx->relations.dev.n_nodes);
    if (words_per_list < least || words_per_list > KDB_GRAPH_MAX_WORDS) {
        kdb_set_error("graph_filter_eval: words_per_list %llu outside (max(count, n_nodes)>>6)+1 = %llu .. 2^30", (unsigned long long)words_per_list,
                      (unsigned long long)least);
        return KDB_ERR_INVALID;
    }
    return graph_queries_check(queries, B, idx->relations.dev.n_nodes, and_lists, n_and_lists, and_of_query);
}

extern "C" int kdb_graph_filter_eval_dev(kdb_index *idx, const kdb_graph_query *queries, uint32_t B, uint64_t *d_lists, uint64_t words_per_list,
                                         uint32_t *d_card, const uint64_t *d_and_lists, uint32_t n_and_lists, const uint32_t *and_of_query,
                                         void *stream) {
    int rc = graph_queries_check(queries, B, 0xffffffffu, d_and_lists, n_and_lists, and_of_query);
    if (rc) return rc;
    if (!d_lists) {
        kdb_set_error("graph_filter_eval: null d_lists");
        return KDB_ERR_INVALID;
    }
    KDB_CHECK_IDX(idx);
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    rc = graph_call_check(idx, queries, B, words_per_list, d_and_lists, n_and_lists, and_of_query);
    if (rc) return rc;
    return kdb_launch_graph_filter(idx, queries, B, d_lists, words_per_list, d_card, d_and_lists, and_of_query, call.s);
}

extern "C" int kdb_graph_filter_eval(kdb_index *idx, const kdb_graph_query *queries, uint32_t B, uint64_t *out_lists, uint64_t words_per_list,
                                     uint32_t *out_card, const uint64_t *and_lists, uint32_t n_and_lists, const uint32_t *and_of_query) {
    int rc = graph_queries_check(queries, B, 0xffffffffu, and_lists, n_and_lists, and_of_query);
    if (rc) return rc;
    if (!out_lists && !out_card) {
        kdb_set_error("graph_filter_eval: out_lists and out_card are both null");
        return KDB_ERR_INVALID;
    }
    KDB_CHECK_IDX(idx);
    KDB_HIP(hipSetDevice(idx->device));
    KdbRegion r_and, r_lists, r_card;
    KdbTurnOpt opt;
    opt.launch_first = and_lists == nullptr; // (the queries are staged by the launcher itself: without and-lists nothing is copied in here)
    return kdb_turn_call(
        idx, opt,
        [&](KdbStage &st) { // the kernels write both whatever the caller asked for: an output nobody wants stays on the device
            if (const int crc = graph_call_check(idx, queries, B, words_per_list, and_lists, n_and_lists, and_of_query)) return crc;
            const size_t lb = (size_t)words_per_list * 8;
            r_and = st.in(and_lists, (size_t)n_and_lists * lb);
            r_lists = out_lists ? st.out(out_lists, (size_t)B * lb) : st.dev((size_t)B * lb);
            r_card = out_card ? st.out(out_card, (size_t)B * 4) : st.dev((size_t)B * 4);
            return (int)KDB_OK;
        },
        [&](unsigned char *d, hipStream_t s) {
            return kdb_launch_graph_filter(idx, queries, B, r_lists.at<uint64_t>(d), words_per_list, r_card.at<uint32_t>(d), r_and.at<uint64_t>(d),
                                           and_of_query, s);
        });
}

// ---------------------------------------------------------------------------------------------
// VExtractSubgraph for B queries (subgraph.hip).  The queries are a host array in both forms, staged by the launcher with the prepared
// guides and the bitmaps in the scratch of the call's lane.
// ---------------------------------------------------------------------------------------------
// n_nodes = 0xffffffff: what needs no index; under idx->mu with the snapshot's n_nodes: the roots and the least words too
static int subgraph_check(const kdb_subgraph_query *queries, uint32_t B, uint32_t n_nodes, const void *guides, uint64_t words_per_list) {
    uint32_t bad = 0;
    const int vrc = kdb_subgraph_validate(queries, B, n_nodes, guides != nullptr, words_per_list, &bad);
    if (vrc) {
        kdb_set_error("subgraph_extract: %s (query %u)", kdb_subgraph_strerror(vrc), bad);
        return KDB_ERR_INVALID;
    }
    return KDB_OK;
}
static int subgraph_call_check(const kdb_index *idx, const kdb_subgraph_query *queries, uint32_t B, const void *guides, uint64_t words_per_list) {
    if (!idx->relations.blob) {
        kdb_set_error("subgraph_extract: the index holds no relation snapshot (kdb_index_set_relations)");
        return KDB_ERR_INVALID;
    }
    return subgraph_check(queries, B, idx->relations.dev.n_nodes, guides, words_per_list);
}

extern "C" int kdb_subgraph_extract_dev(kdb_index *idx, const kdb_subgraph_query *queries, uint32_t B, const float *d_guides, uint64_t *d_nodes,
                                        uint64_t words_per_list, uint32_t *d_n_nodes, uint32_t *d_n_edges, kdb_subgraph_edge *d_edges, uint32_t edge_cap,
                                        void *stream) {
    int rc = subgraph_check(queries, B, 0xffffffffu, d_guides, words_per_list);
    if (rc) return rc;
    if (!d_nodes || !d_n_nodes || !d_n_edges) {
        kdb_set_error("subgraph_extract: null d_nodes, d_n_nodes or d_n_edges");
        return KDB_ERR_INVALID;
    }
    KDB_CHECK_IDX(idx);
    DevCall call(idx, stream);
    if (call.rc) return call.rc;
    rc = subgraph_call_check(idx, queries, B, d_guides, words_per_list);
    if (rc) return rc;
    return kdb_launch_subgraph(idx, queries, B, d_guides, d_nodes, words_per_list, d_n_nodes, d_n_edges, d_edges, edge_cap, call.s);
}

extern "C" int kdb_subgraph_extract(kdb_index *idx, const kdb_subgraph_query *queries, uint32_t B, const float *guides, uint64_t *out_nodes,
                                    uint64_t words_per_list, uint32_t *out_n_nodes, uint32_t *out_n_edges, kdb_subgraph_edge *out_edges, uint32_t edge_cap) {
    int rc = subgraph_check(queries, B, 0xffffffffu, guides, words_per_list);
    if (rc) return rc;
    if (!out_nodes && !out_n_nodes && !out_n_edges && !(out_edges && edge_cap)) {
        kdb_set_error("subgraph_extract: every output is null");
        return KDB_ERR_INVALID;
    }
    KDB_CHECK_IDX(idx);
    KDB_HIP(hipSetDevice(idx->device));
    KdbRegion r_guides, r_nodes, r_nn, r_ne, r_edges;
    KdbTurnOpt opt;
    opt.launch_first = true; // (queries and guides are copied by the launcher and by run() below: the stage copies nothing in)
    return kdb_turn_call(
        idx, opt,
        [&](KdbStage &st) { // the kernels write bitmaps and counts whatever the caller asked for: an output nobody wants stays on the device
            if (const int crc = subgraph_call_check(idx, queries, B, guides, words_per_list)) return crc;
            const size_t lb = (size_t)words_per_list * 8;
            r_guides = st.dev(guides ? (size_t)B * idx->desc.dim * 4 : 0); // filled in run(): the rows of guided queries only
            r_nodes = out_nodes ? st.out(out_nodes, (size_t)B * lb) : st.dev((size_t)B * lb);
            r_nn = out_n_nodes ? st.out(out_n_nodes, (size_t)B * 4) : st.dev((size_t)B * 4);
            r_ne = out_n_edges ? st.out(out_n_edges, (size_t)B * 4) : st.dev((size_t)B * 4);
            r_edges = st.out(out_edges, (size_t)B * edge_cap * sizeof(kdb_subgraph_edge));
            return (int)KDB_OK;
        },
        [&](unsigned char *d, hipStream_t s) -> int {
            const size_t row = (size_t)idx->desc.dim * 4; // (pageable memory: consumed before hipMemcpyAsync returns)
            for (uint32_t b0 = 0, b1 = 0; guides && kdb_subgraph_guided_run(queries, B, b1, &b0, &b1);)
                KDB_HIP(hipMemcpyAsync(r_guides.at<unsigned char>(d) + b0 * row, guides + (size_t)b0 * idx->desc.dim, (b1 - b0) * row, hipMemcpyHostToDevice, s));
            return kdb_launch_subgraph(idx, queries, B, r_guides.at<float>(d), r_nodes.at<uint64_t>(d), words_per_list, r_nn.at<uint32_t>(d),
                                       r_ne.at<uint32_t>(d), r_edges.at<kdb_subgraph_edge>(d), edge_cap, s);
        });
}
