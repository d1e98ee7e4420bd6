// C ABI of libakaze_hip.so, part 4: descriptor_match (pair, multi-set, both directions), match_features, and the RANSAC pairs calls:
// what they all share (pairs_validate .. pairs_scans, the front and the tail: pairs_front, pairs_keep, pairs_tail), the call that draws
// its samples on the host between the two (match_pairs_impl<Model>), and its entry points for both models, one pair or many.
#include "akz_ctx.hpp"
#include "akz_match_rule.hpp"

// Merge of a query set's chunk records (rec[chunk][query], then room for n0 merged records), ratio test and ordered
// compaction: what every scan of one train set ends with (akz_descriptor_match_device, the guided scan), on c->stream.
int match_finish(akz_ctx* c, MatchRec* rec, uint32_t n0, uint32_t chunks, uint32_t thr, double lowes_ratio, akz_match* d_out,
                 uint64_t* d_n_out) {
    // more than a few chunks: a parallel merge first (the compaction is ONE workgroup, i.e. one compute unit's load path:
    // folding 11 chunks of 11 K queries there took 35 us against 5 for the 44-workgroup merge)
    // Query sets of a few workgroups and more: merge, ratio test and ordered compaction in ONE launch (k_match_merge_compact:
    // 44 workgroups for a 4K frame's 11 K rows); tiny ones keep the single-workgroup compaction
    // k_match_merge_compact is a chained look-back: a workgroup publishes its count, then waits for the counts of the
    // workgroups before it.  Two conditions keep that free of deadlock and of cross-talk, and both are enforced HERE:
    //   * every workgroup of the grid is resident at once (progress never depends on the order of dispatch): at most 1 024
    //     workgroups of 256 threads -- four per compute unit -- i.e. query sets of up to 262 144 rows; larger sets take the
    //     merge + single-workgroup compaction below;
    //   * match_state (told apart by epoch) belongs to ONE stream: this function, like every user of the context's matcher
    //     scratch (side 0: ms[0].rec, q8, t8, pop), enqueues on c->stream only -- launches of two epochs never overlap.
    if (n0 >= gates::kMergeCompactMinRows && n0 <= gates::kMergeCompactMaxRows) {
        // (the claim c->match_state.known: how much of the state holds no epoch beyond match_epoch -- a fresh block starts without
        // one, and it is dropped when the epoch wraps: words of 2^32 calls ago would read as published)
        const size_t need = launch::match_merge_compact_state_bytes(n0);
        if (++c->match_epoch == 0) {
            c->match_epoch = 1;
            c->match_state.known = 0;
        }
        if (c->match_state.known < need) {
            if (c->match_state.bytes < need) AKZ_TRY(ensure(c, c->match_state, need * 2));
            c->match_state.known = 0;
            AKZ_HIP_TRY(hipMemsetAsync(c->match_state.p, 0, c->match_state.bytes, c->stream));
            c->match_state.known = c->match_state.bytes;
        }
        launch::match_merge_compact(c->stream, rec, n0, chunks, thr, lowes_ratio * lowes_ratio, d_out,
                                    (unsigned long long*)d_n_out, c->match_state.p, c->match_epoch);
        AKZ_HIP_TRY(hipGetLastError());
        return AKZ_OK;
    }
    const bool premerge = chunks > gates::kPremergeChunks;
    if (premerge) launch::match_merge(c->stream, rec, n0, chunks, thr, rec + (size_t)chunks * n0);
    launch::match_compact(c->stream, premerge ? rec + (size_t)chunks * n0 : rec, n0, premerge ? 1u : chunks, thr,
                          lowes_ratio * lowes_ratio, d_out, (unsigned long long*)d_n_out);
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}
extern "C" {
// ---------------------------------------------------------------------------------------------
// descriptor_match
// ---------------------------------------------------------------------------------------------
// rows_le_61: every row uses at most its first 61 bytes (M-LDB descriptors: 486 bits; the matrix-core kernel keeps the
// train rows' bit counts in the K-columns of bytes 61..63 and ignores whatever those bytes hold)
static int match_device_impl(akz_ctx* c, const uint8_t* d_d0, uint64_t n0, const uint8_t* d_d1, uint64_t n1,
                             uint64_t distance_threshold, double lowes_ratio, akz_match* d_out, uint64_t* d_n_out,
                             bool rows_le_61) {
    AKZ_TRY(bind(c, true, false));  // (the matcher shares nothing with a finish half that may be running on the context's thread)
    if (!d_out || !d_n_out || (n0 && !d_d0) || (n1 && !d_d1) || n0 > 0x7fffffffull || n1 > 0x7fffffffull) {
        set_error("descriptor_match: bad arguments");
        return AKZ_ERR_INVALID_ARG;
    }
    const uint32_t thr = akz::clamp_threshold(distance_threshold);
    // the scan runs on the matrix cores (integer GEMM on the unpacked bits, identical records): 24 us against 29 for the
    // popcount kernel at 128 x 128, 35 against 190 at 1024 x 1024, 3.0 ms against 9.9 at 90 K x 90 K; mode 0 keeps the
    // popcount kernel selectable
    const bool mfma = n0 && n1 && c->settings.match_mode != 0 && rows_le_61;
    const uint32_t chunks = mfma ? launch::match_mfma_chunks((uint32_t)n0, (uint32_t)n1, c->settings.dbg_pair_chunks)
                                 : launch::match_num_chunks((uint32_t)n0, (uint32_t)n1);
    AKZ_TRY(ensure(c, c->ms[0].rec, std::max<uint64_t>(1, n0) * (chunks + 1) * sizeof(MatchRec)));
    MatchRec* rec = (MatchRec*)c->ms[0].rec.p;  // [chunk][query], then the merged records
    if (mfma) {
        const uint32_t q_rows = launch::match_mfma_rows((uint32_t)n0, true), t_rows = launch::match_mfma_rows((uint32_t)n1, false);
        AKZ_TRY(ensure(c, c->ms[0].q8, (size_t)q_rows * 512));
        AKZ_TRY(ensure(c, c->ms[0].t8, (size_t)t_rows * 512));
        AKZ_TRY(ensure(c, c->ms[0].pop, ((size_t)2 * q_rows + t_rows) * sizeof(uint32_t)));
        uint32_t* qpop = (uint32_t*)c->ms[0].pop.p;
        uint32_t* bound = qpop + q_rows;
        uint32_t* tpop = bound + q_rows;
        const bool fp4 = c->settings.match_mode >= 2;
        launch::unpack_pair(c->stream, d_d0, (uint32_t)n0, q_rows, (uint8_t*)c->ms[0].q8.p, qpop, bound, thr, d_d1, (uint32_t)n1, t_rows,
                            (uint8_t*)c->ms[0].t8.p, tpop, fp4);
        launch::match_mfma(c->stream, (const uint8_t*)c->ms[0].q8.p, qpop, (uint32_t)n0, (const uint8_t*)c->ms[0].t8.p,
                           (uint32_t)n1, thr, bound, chunks, rec, fp4);
    } else {
        launch::match(c->stream, d_d0, (uint32_t)n0, d_d1, (uint32_t)n1, thr, rows_le_61, chunks, rec);
    }
    return match_finish(c, rec, (uint32_t)n0, chunks, thr, lowes_ratio, d_out, d_n_out);
}

int akz_descriptor_match_device(akz_ctx* c, const uint8_t* d_d0, uint64_t n0, const uint8_t* d_d1, uint64_t n1,
                                uint64_t distance_threshold, double lowes_ratio, akz_match* d_out,
                                uint64_t* d_n_out) {
    return match_device_impl(c, d_d0, n0, d_d1, n1, distance_threshold, lowes_ratio, d_out, d_n_out, true);
}

// One query set against several train sets in ONE matrix-core launch (all-pairs matching: a query image against
// the descriptor sets of all other images).  A pair of 11 K-row sets alone runs at 1.2 T pairs/s, a launch over
// many sets at the rate of one large product (3 T pairs/s), and every set is unpacked once per call.
// set_first (optional): first row of set k inside d_train (sets anywhere in one block of rows, e.g. a gather's); without
// it the sets follow each other
static int match_sets_impl(akz_ctx* c, const uint8_t* d_q, uint64_t n0, const uint8_t* d_train, const uint64_t* set_rows,
                           uint64_t n_sets, uint64_t distance_threshold, double lowes_ratio, akz_match* d_out, uint64_t* d_n_out,
                           akz_match* d_out_cols, uint64_t* d_n_cols, const uint64_t* set_first = nullptr, int side = 0) {
    AKZ_TRY(bind(c, true, false));
    const bool cols = d_n_cols != nullptr;  // the opposite direction too: every set's rows against the query set
    if ((n0 && !d_out) || !d_n_out || (n_sets && !set_rows) || (n0 && !d_q) || n0 > 0x7fffffffull || n_sets > 65535) {
        set_error("descriptor_match_sets: bad arguments");
        return AKZ_ERR_INVALID_ARG;
    }
    uint64_t total_rows = 0, last_row = 0;
    std::vector<uint64_t> first(n_sets);  // first row of every set in d_train
    for (uint64_t k = 0; k < n_sets; ++k) {
        first[(size_t)k] = set_first ? set_first[k] : total_rows;
        total_rows += set_rows[k];
        last_row = std::max(last_row, first[(size_t)k] + set_rows[k]);
    }
    if ((total_rows && !d_train) || total_rows > 0x7fffffffull || last_row > 0xffffffffull) {
        set_error("descriptor_match_sets: bad train sets");
        return AKZ_ERR_INVALID_ARG;
    }
    if (n_sets == 0) return AKZ_OK;
    if (cols && total_rows && !d_out_cols) {
        set_error("descriptor_match_sets_mutual: null output for the opposite direction");
        return AKZ_ERR_INVALID_ARG;
    }
    if (n0 == 0) {  // (no query rows: nothing can match in either direction)
        AKZ_HIP_TRY(hipMemsetAsync(d_n_out, 0, n_sets * sizeof(uint64_t), c->stream));
        if (cols) AKZ_HIP_TRY(hipMemsetAsync(d_n_cols, 0, n_sets * sizeof(uint64_t), c->stream));
        return AKZ_OK;
    }
    if (cols && c->settings.match_mode < 2) {  // both directions ride on the FP4 kernel only: the other kernels match direction by direction
        uint64_t off = 0;
        for (uint64_t k = 0; k < n_sets; ++k) {
            if (set_rows[k] == 0) AKZ_HIP_TRY(hipMemsetAsync(d_n_cols + k, 0, sizeof(uint64_t), c->stream));
            else
                AKZ_TRY(match_device_impl(c, d_train + first[(size_t)k] * 64, set_rows[k], d_q, n0, distance_threshold, lowes_ratio,
                                          d_out_cols + off, d_n_cols + k, true));
            off += set_rows[k];
        }
    }
    if (c->settings.match_mode == 0) {  // popcount kernel: set by set
        for (uint64_t k = 0; k < n_sets; ++k)
            AKZ_TRY(match_device_impl(c, d_q, n0, d_train + first[(size_t)k] * 64, set_rows[k], distance_threshold, lowes_ratio,
                                      d_out + k * n0, d_n_out + k, true));
        return AKZ_OK;
    }
    // (side 1: the finish stream and the second scratch set -- akz_match_all_pairs alternates; FP4 forms only)
    const bool alt = side == 1 && c->settings.match_mode >= 2;
    if (alt) AKZ_TRY(ensure_aux(c));
    hipStream_t st = alt ? c->aux : c->stream;
    CtxOwned::MatchSide& m = c->ms[alt];
    const bool mutual = cols && c->settings.match_mode >= 2;
    const uint32_t thr = akz::clamp_threshold(distance_threshold);
    const uint32_t tr = launch::match_mfma_tile_rows();
    const uint32_t q_rows = launch::match_mfma_rows((uint32_t)n0, true);
    // padded train image: every set starts on a tile boundary
    std::vector<uint32_t> tiles;  // {first source row, valid rows} per tile
    // every set is cut into `cps` chunks (ascending rows; a short set leaves its last chunks empty) so that the
    // workgroups fill whole rounds of the chip; the chunks of a set share its pruning bounds
    // (chunks are the launch's gridDim.y: at most 65535 of them)
    const uint32_t cps = std::max(1u, std::min(launch::match_mfma_multi_chunks((uint32_t)n0, (uint32_t)n_sets,
                                                                               (uint32_t)((total_rows / n_sets + tr - 1) / tr), c->settings.dbg_set_chunks),
                                               65535u / (uint32_t)n_sets));
    std::vector<launch::MatchChunkHost> chunks((size_t)n_sets * cps);
    std::vector<launch::MatchColSetHost> colsets(mutual ? (size_t)n_sets : 0);
    uint64_t src = 0;
    for (uint64_t k = 0; k < n_sets; ++k) {
        const uint32_t t0 = (uint32_t)(tiles.size() / 2), rows = (uint32_t)set_rows[k];
        if (mutual) colsets[(size_t)k] = launch::MatchColSetHost{t0 * tr, rows, (uint32_t)src};
        for (uint32_t r = 0; r < rows; r += tr) {
            tiles.push_back((uint32_t)(first[(size_t)k] + r));
            tiles.push_back(std::min(tr, rows - r));
        }
        const uint32_t t1 = (uint32_t)(tiles.size() / 2), per = (t1 - t0 + cps - 1) / cps;
        for (uint32_t j = 0; j < cps; ++j)
            chunks[k * cps + j] = launch::MatchChunkHost{std::min(t0 + j * per, t1), std::min(t0 + (j + 1) * per, t1), t0 * tr, rows,
                                                        (uint32_t)(k * q_rows), (uint32_t)(k * cps + j)};
        src += rows;
    }
    const uint32_t n_tiles = (uint32_t)(tiles.size() / 2), t_rows = std::max(1u, n_tiles) * tr;
    if ((uint64_t)n_sets * q_rows > 0x7fffffffull) {
        set_error("descriptor_match_sets: too many sets for this query set");
        return AKZ_ERR_INVALID_ARG;
    }
    // (both directions: the train image is also read as a QUERY image by the seed launch -- whole query blocks of rows)
    const uint32_t t_rows_q = mutual ? launch::match_mfma_rows(t_rows, true) : t_rows;
    AKZ_TRY(ensure(c, m.q8, (size_t)q_rows * 512));
    AKZ_TRY(ensure(c, m.t8, (size_t)t_rows_q * 512));
    AKZ_TRY(ensure(c, m.pop, ((size_t)q_rows * (1 + n_sets) + t_rows) * sizeof(uint32_t)));
    const size_t tab_tiles = std::max<size_t>(1, tiles.size()) * sizeof(uint32_t);
    const size_t tab_chunks = chunks.size() * sizeof(launch::MatchChunkHost), tab_cols = colsets.size() * sizeof(launch::MatchColSetHost);
    AKZ_TRY(ensure(c, m.tab, tab_tiles + tab_chunks + tab_cols));
    unsigned long long* cbest = nullptr;
    uint32_t *csecond = nullptr, *seed_bound = nullptr;
    MatchRec* seed_rec = nullptr;
    if (mutual) {  // per row of the padded train image: 8 + 4 (state) + 4 + 16 (seed launch) bytes
        AKZ_TRY(ensure(c, m.cols, (size_t)t_rows_q * 32));
        cbest = (unsigned long long*)m.cols.p;
        seed_rec = (MatchRec*)((char*)m.cols.p + (size_t)t_rows_q * 8);
        csecond = (uint32_t*)((char*)m.cols.p + (size_t)t_rows_q * 24);
        seed_bound = csecond + t_rows_q;
    }
    AKZ_TRY(ensure(c, m.rec, std::max<uint64_t>(1, n0) * chunks.size() * sizeof(MatchRec)));
    uint32_t* qpop = (uint32_t*)m.pop.p;
    uint32_t* bound = qpop + q_rows;
    uint32_t* tpop = bound + (size_t)n_sets * q_rows;
    uint32_t* d_tiles = (uint32_t*)m.tab.p;
    void* d_chunks = (char*)m.tab.p + tab_tiles;
    // The tables travel through a ring of pinned staging slots, so that the call returns without waiting for its copies
    // (a synchronisation here made every call of an all-pairs loop wait for the previous call's kernel).
    {
        constexpr int kRing = CtxOwned::MatchSide::kRing;
        const size_t need = tab_tiles + tab_chunks + tab_cols;
        if (m.ring.bytes / kRing < need) {
            AKZ_HIP_TRY(hipStreamSynchronize(st));
            AKZ_HIP_TRY(m.ring.release());
            AKZ_HIP_TRY(m.ring.acquire((need + need / 2 + 4096) * kRing, true));
        }
        const int slot = (int)(m.ring_next++ % kRing);
        if (m.ring_ev[slot]) AKZ_HIP_TRY(hipEventSynchronize(m.ring_ev[slot]));  // the copy that used this slot four calls ago
        else AKZ_TRY(m.ring_ev[slot].ensure());
        char* stage = (char*)m.ring.p + (size_t)slot * (m.ring.bytes / kRing);
        if (!tiles.empty()) std::memcpy(stage, tiles.data(), tiles.size() * sizeof(uint32_t));
        std::memcpy(stage + tab_tiles, chunks.data(), tab_chunks);
        if (tab_cols) std::memcpy(stage + tab_tiles + tab_chunks, colsets.data(), tab_cols);
        AKZ_HIP_TRY(hipMemcpyAsync(d_tiles, stage, need, hipMemcpyHostToDevice, st));
        AKZ_HIP_TRY(hipEventRecord(m.ring_ev[slot], st));
    }
    const bool fp4 = c->settings.match_mode >= 2;
    launch::unpack_bits(st, d_q, (uint32_t)n0, q_rows, true, (uint8_t*)m.q8.p, qpop, bound, thr, (uint32_t)n_sets,
                        nullptr, fp4);
    if (n_tiles)
        launch::unpack_bits(st, d_train, 0, n_tiles * tr, false, (uint8_t*)m.t8.p, tpop, nullptr, 0, 0, d_tiles, fp4);
    if (mutual) {
        // the opposite direction rides along: seed the train rows' state from the first rows of the query set, then one pass
        launch::match_cols_seed(st, (const uint8_t*)m.q8.p, (uint32_t)n0, (const uint8_t*)m.t8.p, n_tiles * tr, thr,
                                seed_bound, seed_rec, cbest, csecond);
        launch::match_fp4_multi_mutual(st, (const uint8_t*)m.q8.p, (uint32_t)n0, (const uint8_t*)m.t8.p, d_chunks,
                                       (uint32_t)chunks.size(), thr, bound, (MatchRec*)m.rec.p, cbest, csecond);
        launch::match_compact_cols(st, cbest, csecond, (const char*)d_chunks + tab_chunks, (uint32_t)n_sets, thr,
                                   lowes_ratio * lowes_ratio, d_out_cols, (unsigned long long*)d_n_cols);
    } else {
        launch::match_mfma_multi(st, (const uint8_t*)m.q8.p, qpop, (uint32_t)n0, (const uint8_t*)m.t8.p, d_chunks,
                                 (uint32_t)chunks.size(), thr, bound, (MatchRec*)m.rec.p, fp4);
    }
    launch::match_compact_sets(st, (const MatchRec*)m.rec.p, (uint32_t)n0, (uint32_t)n_sets, cps, thr,
                               lowes_ratio * lowes_ratio, d_out, (unsigned long long*)d_n_out);
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}
}  // extern "C"
// (akz_comm.cpp: the all-pairs match takes its sets where they lie in the gathered block)
int akz::match_sets_at(akz_ctx* c, const uint8_t* d_q, uint64_t n0, const uint8_t* d_rows, const uint64_t* set_first,
                       const uint64_t* set_rows, uint64_t n_sets, uint64_t distance_threshold, double lowes_ratio, akz_match* d_out,
                       uint64_t* d_n_out, akz_match* d_out_cols, uint64_t* d_n_cols, int side) {
    return match_sets_impl(c, d_q, n0, d_rows, set_rows, n_sets, distance_threshold, lowes_ratio, d_out, d_n_out, d_out_cols, d_n_cols,
                           set_first, side);
}
hipStream_t akz::match_side_stream(akz_ctx* c) {
    if (!c || c->settings.match_mode < 2 || bind(c, true, false) != AKZ_OK || ensure_aux(c) != AKZ_OK) return nullptr;
    return c->aux;
}
extern "C" {
int akz_descriptor_match_sets_device(akz_ctx* c, const uint8_t* d_q, uint64_t n0, const uint8_t* d_train,
                                     const uint64_t* set_rows, uint64_t n_sets, uint64_t distance_threshold,
                                     double lowes_ratio, akz_match* d_out, uint64_t* d_n_out) {
    return match_sets_impl(c, d_q, n0, d_train, set_rows, n_sets, distance_threshold, lowes_ratio, d_out, d_n_out, nullptr, nullptr);
}
// Both directions of every (query set, train set k) block from ONE pass over the distances (hamming is symmetric): besides
// the lists of akz_descriptor_match_sets_device, the match list of set k's rows AS QUERIES against the query set as train
// (feature_matching.rs:23-94 with the two sets exchanged) goes to d_out_cols + (rows of the sets before k), its length to
// d_n_cols[k].  Identical to two akz_descriptor_match_device calls per block, at the matrix-core work of one.
int akz_descriptor_match_sets_mutual_device(akz_ctx* c, const uint8_t* d_q, uint64_t n0, const uint8_t* d_train,
                                            const uint64_t* set_rows, uint64_t n_sets, uint64_t distance_threshold,
                                            double lowes_ratio, akz_match* d_out, uint64_t* d_n_out, akz_match* d_out_cols,
                                            uint64_t* d_n_cols) {
    if (!d_n_cols) {
        set_error("descriptor_match_sets_mutual: null count output");
        return AKZ_ERR_INVALID_ARG;
    }
    return match_sets_impl(c, d_q, n0, d_train, set_rows, n_sets, distance_threshold, lowes_ratio, d_out, d_n_out, d_out_cols, d_n_cols);
}

int akz_descriptor_match(akz_ctx* c, const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1,
                         uint64_t desc_bytes, uint64_t distance_threshold, double lowes_ratio, akz_match* out,
                         uint64_t* n_out) {
    AKZ_TRY(bind(c, true, false));
    if (!n_out || desc_bytes == 0 || desc_bytes > 64 || (n0 && (!d0 || !out)) || (n1 && !d1)) {
        set_error("descriptor_match: bad arguments (desc_bytes must be 1..64)");
        return AKZ_ERR_INVALID_ARG;
    }
    *n_out = 0;
    if (n0 == 0) return AKZ_OK;
    auto pad = [&](const uint8_t* src, uint64_t cnt, std::vector<uint8_t>& dst) {
        dst.assign((size_t)std::max<uint64_t>(1, cnt) * 64, 0);
        for (uint64_t i = 0; i < cnt; ++i) std::memcpy(&dst[(size_t)i * 64], src + i * desc_bytes, desc_bytes);
    };
    std::vector<uint8_t> p0, p1;
    pad(d0, n0, p0);
    pad(d1, n1, p1);
    AKZ_TRY(ensure(c, c->match_a, p0.size()));
    AKZ_TRY(ensure(c, c->match_b, p1.size()));
    AKZ_TRY(ensure(c, c->match_out, n0 * sizeof(akz_match) + 64));
    AKZ_HIP_TRY(hipMemcpyAsync(c->match_a.p, p0.data(), p0.size(), hipMemcpyHostToDevice, c->stream));
    AKZ_HIP_TRY(hipMemcpyAsync(c->match_b.p, p1.data(), p1.size(), hipMemcpyHostToDevice, c->stream));
    akz_match* d_m = (akz_match*)((char*)c->match_out.p + 64);
    uint64_t* d_cnt = (uint64_t*)c->match_out.p;
    AKZ_TRY(match_device_impl(c, (const uint8_t*)c->match_a.p, n0, (const uint8_t*)c->match_b.p, n1, distance_threshold,
                              lowes_ratio, d_m, d_cnt, desc_bytes <= 61));
    uint64_t cnt = 0;
    AKZ_HIP_TRY(hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    if (cnt) {
        AKZ_HIP_TRY(hipMemcpyAsync(out, d_m, cnt * sizeof(akz_match), hipMemcpyDeviceToHost, c->stream));
        AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *n_out = cnt;
    return AKZ_OK;
}

// Host keypoint logic alone (no GPU): raster-ordered NMS candidates -> keypoints without angle.
// cand: n_cand records {level, idx, v, xp, xm, yp, ym, pad} (32 bytes each, any order).
int akz_host_select_keypoints(uint32_t w, uint32_t h, const akz_config* cfg, const void* cand, uint64_t n_cand,
                              akz_keypoint* out, uint64_t cap, uint64_t* n_out, uint64_t* n_extrema) {
    if (!cfg || (n_cand && !cand) || !n_out) return AKZ_ERR_INVALID_ARG;
    std::vector<LevelPlan> plan;
    AKZ_TRY(build_plan(w, h, *cfg, plan));
    std::vector<Candidate> c((const Candidate*)cand, (const Candidate*)cand + n_cand);
    for (const Candidate& x : c)
        if (x.level >= plan.size() || x.idx >= (uint64_t)plan[x.level].w * plan[x.level].h) {
            set_error("candidate out of range");
            return AKZ_ERR_INVALID_ARG;
        }
    sort_candidates(c, plan);
    std::vector<HostKeypoint> hk;
    uint64_t ne = 0;
    select_keypoints(c.data(), c.size(), plan, *cfg, hk, &ne);
    *n_out = hk.size();
    if (n_extrema) *n_extrema = ne;
    if (out)
        for (size_t i = 0; i < hk.size() && i < cap; ++i)
            out[i] = akz_keypoint{hk[i].x, hk[i].y, hk[i].response, hk[i].size, hk[i].octave, hk[i].class_id, 0.0f, 0};
    return AKZ_OK;
}
int akz_remove_outliers(const akz_keypoint*, uint64_t, const akz_keypoint*, uint64_t, const akz_match*, uint64_t, uint64_t,
                        float, float, akz_match*, uint64_t*);
int akz_match_features(akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0,
                       const akz_keypoint* kp1, uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes,
                       double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers, akz_match* out,
                       uint64_t* n_out) {
    if (!n_out) return AKZ_ERR_INVALID_ARG;
    // a match indexes the keypoint lists with descriptor indices (lib.rs:267-274): the reference panics on a set with
    // more descriptors than keypoints as soon as such a match reaches RANSAC; here it is refused up front
    if (n_d0 > n_kp0 || n_d1 > n_kp1) {
        set_error("match_features: a feature set has more descriptors than keypoints");
        return AKZ_ERR_INVALID_ARG;
    }
    std::vector<akz_match> raw((size_t)std::max<uint64_t>(1, n_d0));
    uint64_t n_raw = 0;
    AKZ_TRY(akz_descriptor_match(c, d0, n_d0, d1, n_d1, desc_bytes, 10000, lowes_ratio, raw.data(), &n_raw));  // lib.rs:261-266
    // lib.rs:267-274.  The trials run on the device (akz_ransac_kernels.hip: the host's model source, same bits) when there is
    // enough of them to pay for a launch and a round trip (~60 us); the samples, the choice of the winner and the final
    // filter stay on the host.  A 4K pair (8 264 matches, 1 000 trials): 1.3-1.4 ms on 16 host threads -> see DESIGN 6.
    TrialsOnDevice on_device;
    if (c && ransac_trials * (n_raw + 4000) >= 400000)
        on_device = [c](const float* x0, const float* y0, const float* x1, const float* y1, uint32_t n, const uint32_t* samples,
                        uint32_t trials, float eps_model, float eps_inlier, float* models, int32_t* inliers) -> int {
            AKZ_TRY(bind(c, true, false));
            const size_t b_pts = (size_t)n * 4 * sizeof(float), b_smp = (size_t)trials * 8 * sizeof(uint32_t);
            const size_t b_mdl = (size_t)trials * 9 * sizeof(float), b_inl = (size_t)trials * sizeof(int32_t);
            const size_t in_bytes = up256(b_pts) + up256(b_smp), out_bytes = up256(b_mdl) + up256(b_inl);
            AKZ_TRY(ensure(c, c->ransac_dev, in_bytes + out_bytes));
            AKZ_TRY(ensure_pinned(c, c->ransac_pin, in_bytes + out_bytes));
            char* h = (char*)c->ransac_pin.p;
            char* d = (char*)c->ransac_dev.p;
            std::memcpy(h, x0, (size_t)n * 4); std::memcpy(h + (size_t)n * 4, y0, (size_t)n * 4);
            std::memcpy(h + (size_t)n * 8, x1, (size_t)n * 4); std::memcpy(h + (size_t)n * 12, y1, (size_t)n * 4);
            std::memcpy(h + up256(b_pts), samples, b_smp);
            hipStream_t st = c->stream;
            AKZ_HIP_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
            launch::ransac_trials(st, (const float*)d, n, (const uint32_t*)(d + up256(b_pts)), trials, eps_model, eps_inlier,
                                  (float*)(d + in_bytes), (int32_t*)(d + in_bytes + up256(b_mdl)));
            AKZ_HIP_TRY(hipGetLastError());
            AKZ_HIP_TRY(hipMemcpyAsync(h + in_bytes, d + in_bytes, out_bytes, hipMemcpyDeviceToHost, st));
            AKZ_HIP_TRY(hipStreamSynchronize(st));
            std::memcpy(models, h + in_bytes, b_mdl);
            std::memcpy(inliers, h + in_bytes + up256(b_mdl), b_inl);
            return AKZ_OK;
        };
    return remove_outliers_impl(kp0, n_kp0, kp1, n_kp1, raw.data(), n_raw, ransac_trials, 0.05f, ransac_epsilon_inliers, out, n_out,
                                on_device);
}

}  // extern "C"

const char* set_refusal(const akz_feature_set& s) {
    if (s.n_descriptors > s.n_keypoints) return "more descriptors than keypoints";
    if ((s.n_keypoints && !s.keypoints) || (s.n_descriptors && !s.descriptors)) return "null keypoints or descriptors";
    return nullptr;
}
static int pairs_refuse(const char* name, const std::string& msg) {
    set_error(name + msg);
    return AKZ_ERR_INVALID_ARG;
}
// The refusals every opening of a pairs call makes, all before any GPU work, with the one walk over pairs[]: the index bound, seen[k] = 1
// for every set a pair names, cap = the room of `out` (sum of the first sets' descriptors), and set_refusal of every set when it is
// first seen.  Over a bank desc_bytes and the sets are the bank's own and were checked when it was made: nothing of them is refused here.
static int pairs_validate(const PairsCall& q, std::vector<uint8_t>& seen, uint64_t& cap) {
    if (!q.pairs || !q.n_out) return pairs_refuse(q.name, "null pairs or n_out");
    if (q.desc_bytes == 0 || q.desc_bytes > 64) return pairs_refuse(q.name, "desc_bytes must be 1..64");
    if (q.n_sets && !q.sets) return pairs_refuse(q.name, "null sets");
    seen.assign((size_t)q.n_sets, 0);
    cap = 0;
    for (uint64_t p = 0; p < q.n_pairs; ++p)
        for (int side = 0; side < 2; ++side) {
            const uint64_t k = q.pairs[2 * p + side];
            if (k >= q.n_sets)
                return pairs_refuse(q.name, "pair " + std::to_string(p) + ": set index " + std::to_string(k) + " >= n_sets " + std::to_string(q.n_sets));
            if (side == 0) cap += q.sets[k].n_descriptors;
            if (seen[(size_t)k]) continue;
            if (const char* why = q.bank ? nullptr : set_refusal(q.sets[k]))
                return pairs_refuse(q.name, "pair " + std::to_string(p) + ", set " + std::to_string(k) + ": " + why);
            seen[(size_t)k] = 1;
        }
    if (cap && !q.out) return pairs_refuse(q.name, "null out");
    if (!q.c) return pairs_refuse(q.name, "null context");
    return AKZ_OK;
}
int pairs_upload(akz_ctx* c, const akz_feature_set* sets, uint64_t desc_bytes, const SetsBlock& b, const std::vector<uint64_t>& order) {
    hipStream_t st = c->stream;
    uint8_t* h = (uint8_t*)c->mp_pin_in.p;
    float *hx = (float*)(h + b.b_rows), *hy = (float*)(h + b.b_rows + b.b_xy);
    for (uint64_t k : order) {
        const akz_feature_set& s = sets[k];
        const uint64_t row0 = b.set_row[(size_t)k];
        uint8_t* r = h + row0 * 64;
        for (uint64_t i = 0; i < s.n_descriptors; ++i) {
            std::memcpy(r + i * 64, s.descriptors + i * desc_bytes, (size_t)desc_bytes);
            if (desc_bytes < 64) std::memset(r + i * 64 + desc_bytes, 0, (size_t)(64 - desc_bytes));
            hx[row0 + i] = s.keypoints[i].x;
            hy[row0 + i] = s.keypoints[i].y;
        }
    }
    AKZ_HIP_TRY(hipMemcpyAsync(b.d_rows, h, (size_t)b.rows * 64, hipMemcpyHostToDevice, st));
    AKZ_HIP_TRY(hipMemcpyAsync(b.d_kx, hx, (size_t)b.rows * 4, hipMemcpyHostToDevice, st));
    AKZ_HIP_TRY(hipMemcpyAsync(b.d_ky, hy, (size_t)b.rows * 4, hipMemcpyHostToDevice, st));
    return AKZ_OK;
}
// The scans of the pairs calls, enqueued on the context's stream over the sets placed in blk: pair p's raw list goes to
// d_raw + tab[p].raw_off, its count to d_cnt[tab[p].cnt_idx] (zeroed here) -- one multi-set launch per first set, or the pair
// matcher for rows of 62..64 bytes.  tab: one record per pair, raw_off, kp0_off, kp1_off and cnt_idx filled in.
// cross (optional, with d_rev and d_rcnt): the opposite direction too -- pair p's descriptor_match(second set, first set) goes to
// d_rev + (*cross)[p].rev_off (room for the second set's rows; the sum of those over the pairs is the room of d_rev), its count
// to d_rcnt[tab[p].cnt_idx] (zeroed here); (*cross)[p] is the pair's record for launch::pairs_cross_filter.  From the same
// multi-set launch on the FP4 matcher, a second scan with the sets exchanged otherwise.  distance_threshold: 10000 for match_features.
int pairs_scans(const PairsCall& q, double lowes_ratio, const SetsBlock& blk, akz_match* d_raw, uint64_t* d_cnt, std::vector<launch::PairJobHost>& tab,
                akz_match* d_rev, uint64_t* d_rcnt, std::vector<launch::CrossJobHost>* cross, uint64_t distance_threshold) {
    akz_ctx* c = q.c;
    const std::vector<uint64_t>& set_row = blk.set_row;
    uint8_t* d_rows = blk.d_rows;
    hipStream_t st = c->stream;
    tab.assign((size_t)q.n_pairs, launch::PairJobHost{});
    AKZ_HIP_TRY(hipMemsetAsync(d_cnt, 0, (size_t)q.n_pairs * 8, st));
    if (cross) {
        cross->assign((size_t)q.n_pairs, launch::CrossJobHost{});
        AKZ_HIP_TRY(hipMemsetAsync(d_rcnt, 0, (size_t)q.n_pairs * 8, st));
    }
    uint64_t raw_base = 0, rev_base = 0;
    if (q.desc_bytes > 61) {  // every byte of a row counts: the pair matcher of akz_descriptor_match
        for (uint64_t p = 0; p < q.n_pairs; ++p) {
            const uint64_t a = q.pairs[2 * p], b = q.pairs[2 * p + 1], na = q.sets[a].n_descriptors;
            tab[(size_t)p] = launch::PairJobHost{raw_base, set_row[(size_t)a], set_row[(size_t)b], 0, 0, 0, (uint32_t)p, 0};
            if (na)
                AKZ_TRY(match_device_impl(c, d_rows + set_row[(size_t)a] * 64, na, d_rows + set_row[(size_t)b] * 64, q.sets[b].n_descriptors,
                                          distance_threshold, lowes_ratio, d_raw + raw_base, d_cnt + p, false));
            if (cross) {
                const uint64_t nb = q.sets[b].n_descriptors;
                (*cross)[(size_t)p] = launch::CrossJobHost{raw_base, rev_base, (uint32_t)p, (uint32_t)p, (uint32_t)na, (uint32_t)nb};
                if (na && nb)
                    AKZ_TRY(match_device_impl(c, d_rows + set_row[(size_t)b] * 64, nb, d_rows + set_row[(size_t)a] * 64, na, distance_threshold, lowes_ratio,
                                              d_rev + rev_base, d_rcnt + p, false));
                rev_base += nb;
            }
            raw_base += na;
        }
    } else {  // one multi-set launch per first set over its second sets (split at the matcher's limits)
        std::vector<std::vector<uint64_t>> groups;
        std::vector<int64_t> group_of((size_t)q.n_sets, -1);
        for (uint64_t p = 0; p < q.n_pairs; ++p) {
            const uint64_t a = q.pairs[2 * p];
            if (group_of[(size_t)a] < 0) {
                group_of[(size_t)a] = (int64_t)groups.size();
                groups.emplace_back();
            }
            groups[(size_t)group_of[(size_t)a]].push_back(p);
        }
        uint32_t cnt_base = 0;
        std::vector<uint64_t> first, nrows;
        for (const auto& g : groups) {
            const uint64_t a = q.pairs[2 * g[0]], n0 = q.sets[a].n_descriptors;
            const uint64_t max_sets = std::max<uint64_t>(1, std::min<uint64_t>(65535, n0 ? 0x7fffffffull / launch::match_mfma_rows((uint32_t)n0, true) : 65535));
            for (size_t i = 0; i < g.size();) {
                first.clear();
                nrows.clear();
                uint64_t train = 0;
                const size_t i0 = i;
                while (i < g.size() && first.size() < max_sets) {
                    const uint64_t b = q.pairs[2 * g[i] + 1], nb = q.sets[b].n_descriptors;
                    if (!first.empty() && train + nb > 0x7fffffffull) break;
                    first.push_back(set_row[(size_t)b]);
                    nrows.push_back(nb);
                    train += nb;
                    const uint64_t p = g[i];
                    tab[(size_t)p] = launch::PairJobHost{raw_base + (i - i0) * n0, set_row[(size_t)a], set_row[(size_t)b], 0, 0, 0,
                                                                   cnt_base + (uint32_t)(i - i0), 0};
                    if (cross)  // (the launch puts set k's reverse list behind those of the sets before it)
                        (*cross)[(size_t)p] = launch::CrossJobHost{raw_base + (i - i0) * n0, rev_base + (train - nb), cnt_base + (uint32_t)(i - i0),
                                                                   cnt_base + (uint32_t)(i - i0), (uint32_t)n0, (uint32_t)nb};
                    ++i;
                }
                if (n0)
                    AKZ_TRY(match_sets_at(c, d_rows + set_row[(size_t)a] * 64, n0, d_rows, first.data(), nrows.data(), first.size(), distance_threshold,
                                          lowes_ratio, d_raw + raw_base, d_cnt + cnt_base, cross && train ? d_rev + rev_base : nullptr,
                                          cross && train ? d_rcnt + cnt_base : nullptr));  // (no train row: both directions are empty)
                rev_base += train;
                raw_base += first.size() * n0;
                cnt_base += (uint32_t)first.size();
            }
        }
    }
    return AKZ_OK;
}
// The opening every pairs call shares (akz_ctx.hpp): no GPU work before the last refusal.
int pairs_open(const PairsCall& q, bool guided, PairsFront& f) {
    akz_ctx* c = q.c;
    std::vector<uint8_t> seen;
    uint64_t cap = 0;
    AKZ_TRY(pairs_validate(q, seen, cap));
    if (guided) AKZ_TRY(guided_limits(q.name, q.sets, q.pairs, q.n_pairs, seen));
    AKZ_TRY(bind(c, true, false));
    for (uint64_t i = 0; i < 2 * q.n_pairs; ++i) {  // every distinct set once, in order of first use (seen 2: listed)
        uint8_t& s = seen[(size_t)q.pairs[i]];
        if (s == 1) f.used.push_back(q.pairs[i]);
        s = 2;
    }
    f.block.place(q.sets, q.n_sets, f.used);
    f.cap1 = std::max<uint64_t>(cap, 1);
    f.b_cnt = up256((size_t)q.n_pairs * 8);
    AKZ_TRY(ensure(c, c->mp_in, f.block.bytes(false)));
    AKZ_TRY(ensure_pinned(c, c->mp_pin_in, f.block.bytes(false)));
    f.block.bind(c->mp_in.p, false);
    return AKZ_OK;
}
// The opening of a bank call (akz_ctx.hpp): what set_refusal refuses of a set was refused when the bank was made, so the refusals
// left are the call's own -- no GPU work before the last of them -- and the block is the bank's, every set placed whether a pair
// names it or not.
int pairs_open_bank(const PairsCall& q, bool guided, PairsFront& f) {
    std::vector<uint8_t> seen;
    uint64_t cap = 0;
    AKZ_TRY(pairs_validate(q, seen, cap));
    if (q.bank->ctx != q.c) return pairs_refuse(q.name, "the bank belongs to another context");
    if (guided) {
        AKZ_TRY(guided_limits(q.name, q.sets, q.pairs, q.n_pairs, seen));
        if (q.bank->block.rows > 0xffffffffull) return pairs_refuse(q.name, "too many rows in the bank for one guided launch");  // (its records carry absolute rows)
    }
    AKZ_TRY(bind(q.c, true, false));
    f.block = q.bank->block;
    f.cap1 = std::max<uint64_t>(cap, 1);
    f.b_cnt = up256((size_t)q.n_pairs * 8);
    return AKZ_OK;
}
int pairs_table_upload(akz_ctx* c, PairsFront& f) { return table_upload(c, f.d_tab, f.h_tab, f.tab.data(), f.tab.size() * sizeof(launch::PairJobHost)); }
// The front of the RANSAC pairs calls, all on the context's stream: every distinct set's 64-byte rows and keypoint x / y through pinned
// staging; the descriptor scans (pairs_scans; cross: the opposite direction too, and the filter that rewrites raw lists and counts before
// anything reads them); the pair table; k_pair_points; the read-back of the match counts, which the caller waits for.
int pairs_front(const PairsCall& q, double lowes_ratio, bool guided, bool cross, size_t b_dev_own, size_t b_pin_own, PairsFront& f) {
    if (q.bank) AKZ_TRY(pairs_open_bank(q, guided, f));
    else AKZ_TRY(pairs_open(q, guided, f));
    akz_ctx* c = q.c;
    const uint64_t n_pairs = q.n_pairs;
    f.timed = c->mp_split_on;
    if (f.timed)
        for (Event& e : c->mp_split_ev) AKZ_TRY(e.ensure(hipEventDefault));
    hipStream_t st = c->stream;
    const size_t b_raw = up256((size_t)f.cap1 * sizeof(akz_match)), b_tab = up256((size_t)n_pairs * sizeof(launch::PairJobHost));
    AKZ_TRY(ensure(c, c->mp_raw, b_raw + f.b_cnt + (size_t)f.cap1 * 16));
    AKZ_TRY(ensure(c, c->mp_tab, b_tab + b_dev_own));
    AKZ_TRY(ensure_pinned(c, c->mp_pin_tab, b_tab + f.b_cnt + b_pin_own));
    f.d_raw = (akz_match*)c->mp_raw.p;
    f.d_cnt = (uint64_t*)((char*)c->mp_raw.p + b_raw);
    f.d_pts = (float*)((char*)c->mp_raw.p + b_raw + f.b_cnt);
    f.d_tab = (launch::PairJobHost*)c->mp_tab.p;
    f.d_own = (char*)c->mp_tab.p + b_tab;
    f.h_tab = (launch::PairJobHost*)c->mp_pin_tab.p;
    f.h_cnt = (uint64_t*)((char*)c->mp_pin_tab.p + b_tab);
    f.h_own = (char*)c->mp_pin_tab.p + b_tab + f.b_cnt;
    if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[0], st));
    if (!q.bank) AKZ_TRY(pairs_upload(c, q.sets, q.desc_bytes, f.block, f.used));  // (a bank's sets are where the scans read them)
    if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[1], st));
    if (cross) {  // the reverse lists (room: every pair's second set), their counts and the filter's records
        uint64_t cap_rev = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) cap_rev += q.sets[q.pairs[2 * p + 1]].n_descriptors;
        const size_t b_rev = up256((size_t)std::max<uint64_t>(cap_rev, 1) * sizeof(akz_match)), b_xtab = up256((size_t)n_pairs * sizeof(launch::CrossJobHost));
        AKZ_TRY(ensure(c, c->cx_rev, b_rev + f.b_cnt + b_xtab));
        AKZ_TRY(ensure_pinned(c, c->cx_pin_tab, b_xtab));
        akz_match* d_rev = (akz_match*)c->cx_rev.p;
        uint64_t* d_rcnt = (uint64_t*)((char*)c->cx_rev.p + b_rev);
        launch::CrossJobHost* d_xtab = (launch::CrossJobHost*)((char*)c->cx_rev.p + b_rev + f.b_cnt);
        std::vector<launch::CrossJobHost> xtab;
        AKZ_TRY(pairs_scans(q, lowes_ratio, f.block, f.d_raw, f.d_cnt, f.tab, d_rev, d_rcnt, &xtab));
        AKZ_TRY(table_upload(c, d_xtab, c->cx_pin_tab.p, xtab.data(), (size_t)n_pairs * sizeof(launch::CrossJobHost)));
        launch::pairs_cross_filter(st, d_xtab, (uint32_t)n_pairs, f.d_raw, f.d_cnt, d_rev, d_rcnt);
        AKZ_HIP_TRY(hipGetLastError());
    } else {
        AKZ_TRY(pairs_scans(q, lowes_ratio, f.block, f.d_raw, f.d_cnt, f.tab));
    }
    AKZ_TRY(pairs_table_upload(c, f));
    launch::pair_points(st, f.d_tab, (uint32_t)n_pairs, f.d_raw, f.d_cnt, f.block.d_kx, f.block.d_ky, f.d_pts, f.cap1);
    AKZ_HIP_TRY(hipGetLastError());
    AKZ_HIP_TRY(hipMemcpyAsync(f.h_cnt, f.d_cnt, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, st));
    return AKZ_OK;
}
// room for the head and the kept lists of n_keep matches (PairsKeep, akz_pairs_layout.hpp) on the device and in pinned memory
int pairs_keep(akz_ctx* c, const PairsFront& f, uint64_t n_keep, PairsKeep& k) {
    k.n_keep = n_keep;
    k.b_cnt = f.b_cnt;
    k.b_points = k.want_points ? up256((size_t)std::max<uint64_t>(n_keep, 1) * 12) : 0;
    const size_t b_keep = pairs_head(nullptr, k).bytes + (size_t)std::max<uint64_t>(n_keep, 1) * sizeof(akz_match);
    AKZ_TRY(ensure(c, c->mp_keep, b_keep));
    AKZ_TRY(ensure_pinned(c, c->mp_pin_out, b_keep));
    k.d = pairs_head(c->mp_keep.p, k);
    return AKZ_OK;
}
int pairs_copy_out(const PairsCall& q, const uint64_t* h_gcnt, const int32_t* h_found, const akz_match* d_gout, const uint64_t* h_kcnt,
                   const akz_match* h_keep, const launch::PairJobHost* tab) {
    akz_ctx* c = q.c;
    auto guided = [&](uint64_t p) { return h_gcnt && (!h_found || h_found[p] != 0); };
    uint64_t span = 0, off = 0;
    for (uint64_t p = 0; p < q.n_pairs; ++p) {
        if (guided(p) && h_gcnt[p]) span = off + h_gcnt[p];
        off += q.sets[q.pairs[2 * p]].n_descriptors;
    }
    if (span) {  // through pinned staging
        AKZ_TRY(ensure_pinned(c, c->gd_pin_out, (size_t)span * sizeof(akz_match)));
        AKZ_HIP_TRY(hipMemcpyAsync(c->gd_pin_out.p, d_gout, (size_t)span * sizeof(akz_match), hipMemcpyDeviceToHost, c->stream));
        AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    }
    const akz_match* h_gout = (const akz_match*)c->gd_pin_out.p;
    uint64_t at = 0;
    for (uint64_t p = 0; p < q.n_pairs; ++p) {
        const uint64_t n = guided(p) ? h_gcnt[p] : h_kcnt[p];  // found: the guided list replaces the filtered one
        if (n) std::memcpy(q.out + at, guided(p) ? h_gout + at : h_keep + tab[p].keep_off, (size_t)n * sizeof(akz_match));
        q.n_out[p] = n;
        at += q.sets[q.pairs[2 * p]].n_descriptors;
    }
    return AKZ_OK;
}
// The tail of the RANSAC pairs calls (akz_ctx.hpp).  launch::model_refit rewrites the models, the kept lists and their counts in place and
// adds every pair's number of accepted fits to the head; the guided stage then scans every pair again with the model (H or F) that is on
// the device (pairs without one give empty lists that nobody reads) over the sets the front uploaded.  Both stages need the head's models.
// launch::pairs_pose, behind the refit, shrinks the kept lists in place to the matches in front of both cameras and fills the head's poses
// and points (the seeded call alone asks for it, and refuses the guided stage with it).
int pairs_tail(const PairsCall& q, const PairsFront& f, const PairsKeep& k, launch::RansacModel kind, const float* d_mdl, const int32_t* d_inl,
               float epsilon_inliers, const RefineStage* refine, float refit_epsilon, const GuidedStage* guided, int guided_kind, double t_host,
               float* model, int* found, uint32_t* fits, uint64_t* trials_run, const PoseStage* pose) {
    akz_ctx* c = q.c;
    const uint64_t n_pairs = q.n_pairs;
    hipStream_t st = c->stream;
    launch::pairs_pick_filter(st, kind, f.d_tab, (uint32_t)n_pairs, f.d_raw, f.d_cnt, f.d_pts, f.cap1, d_mdl, d_inl, epsilon_inliers, k.d.keep, k.d.cnt,
                              k.b_model ? k.d.model : nullptr, k.b_found ? k.d.found : nullptr);
    AKZ_HIP_TRY(hipGetLastError());
    if (refine) {  // (inside the pick / filter interval of akz_debug_match_pairs_split)
        launch::model_refit(st, kind, f.d_tab, (uint32_t)n_pairs, f.d_raw, f.d_cnt, f.d_pts, f.cap1, refit_epsilon, epsilon_inliers,
                            refine->max_iterations, k.d.keep, k.d.cnt, k.d.model, k.d.found, k.d.fits);
        AKZ_HIP_TRY(hipGetLastError());
    }
    if (pose) {  // (inside the same interval; the kept lists shrink in place, so the one read-back below carries the final ones)
        launch::pairs_pose(st, f.d_tab, (uint32_t)n_pairs, pose->d_cameras, f.block.d_kx, f.block.d_ky, k.d.model, k.d.found, k.d.keep, k.d.cnt, k.d.pose,
                           pose->points ? k.d.points : nullptr);
        AKZ_HIP_TRY(hipGetLastError());
    }
    if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[5], st));
    AKZ_HIP_TRY(hipMemcpyAsync(c->mp_pin_out.p, c->mp_keep.p, k.d.bytes + (size_t)k.n_keep * sizeof(akz_match), hipMemcpyDeviceToHost, st));
    if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[6], st));
    akz_match* d_gout = nullptr;
    if (guided) {
        AKZ_TRY(ensure(c, c->gd_out, f.b_cnt + (size_t)f.cap1 * sizeof(akz_match)));
        AKZ_TRY(ensure_pinned(c, c->gd_pin_cnt, f.b_cnt));
        uint64_t* d_gcnt = (uint64_t*)c->gd_out.p;
        d_gout = (akz_match*)((char*)c->gd_out.p + f.b_cnt);
        AKZ_TRY(guided_enqueue(c, guided_specs(q, f.block), f.block, guided_kind, k.d.model, k.d.found, guided->radius, 10000, guided->ratio, d_gout, d_gcnt));
        AKZ_HIP_TRY(hipMemcpyAsync(c->gd_pin_cnt.p, d_gcnt, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, st));
    }
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    const PairsHead h = pairs_head(c->mp_pin_out.p, k);  // the head's pinned image
    AKZ_TRY(pairs_copy_out(q, guided ? (const uint64_t*)c->gd_pin_cnt.p : nullptr, h.found, d_gout, h.cnt, h.keep, f.tab.data()));
    if (model) std::memcpy(model, h.model, (size_t)n_pairs * 36);
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (found) found[p] = h.found[p];
        if (fits) fits[p] = h.fits[p];
        if (trials_run) trials_run[p] = h.trials[p];
    }
    if (pose) {
        std::memcpy(pose->poses, h.pose, (size_t)n_pairs * sizeof(akz_pose));
        if (pose->points) {  // (3 floats per kept record at the place of its list, to the place of that list in `out`)
            uint64_t at = 0;
            for (uint64_t p = 0; p < n_pairs; ++p) {
                if (q.n_out[p] && pose->poses[p].found) std::memcpy(pose->points + 3 * at, h.points + 3 * f.tab[(size_t)p].keep_off, (size_t)q.n_out[p] * 12);
                at += q.sets[q.pairs[2 * p]].n_descriptors;
            }
        }
    }
    if (f.timed) {  // akz_debug_match_pairs_split: [3] is the trials or the rounds, between the caller's events 3 and 4
        float ms[6] = {};
        AKZ_HIP_TRY(hipEventElapsedTime(&ms[0], c->mp_split_ev[0], c->mp_split_ev[1]));
        AKZ_HIP_TRY(hipEventElapsedTime(&ms[1], c->mp_split_ev[1], c->mp_split_ev[2]));
        AKZ_HIP_TRY(hipEventElapsedTime(&ms[3], c->mp_split_ev[3], c->mp_split_ev[4]));
        AKZ_HIP_TRY(hipEventElapsedTime(&ms[4], c->mp_split_ev[4], c->mp_split_ev[5]));
        AKZ_HIP_TRY(hipEventElapsedTime(&ms[5], c->mp_split_ev[5], c->mp_split_ev[6]));
        for (int i = 0; i < 6; ++i) c->mp_split_ms[i] = ms[i];
        c->mp_split_ms[2] = t_host;
    }
    return AKZ_OK;
}
// The geometric model of the pairs orchestration below: the kernels' model kind, K match indices per sample, and whether the
// call hands back a model per pair (H, found).
namespace {
struct FundamentalModel {  // akz_match_features_pairs
    static constexpr launch::RansacModel kKind = launch::RansacModel::Fundamental;
    static constexpr int K = 8;
    static constexpr bool kModelOut = false;
    static constexpr float kEpsilonModel = 0.05f;
    static constexpr float kRefitEpsilon = AKZ_FUNDAMENTAL_REFIT_EPSILON;  // the rank rule of the refit stage
    static constexpr int kGuidedKind = AKZ_GUIDED_FUNDAMENTAL;            // the gate of the guided stage
    static constexpr const char* kName = "match_features_pairs: ";
};
struct FundamentalModelOut : FundamentalModel {  // akz_match_features_fundamental*(_pairs): F and found are read back too
    static constexpr bool kModelOut = true;
    static constexpr const char* kName = "match_features_fundamental_pairs: ";
};
struct HomographyModel {  // akz_match_features_homography(_pairs)
    static constexpr launch::RansacModel kKind = launch::RansacModel::Homography;
    static constexpr int K = 4;
    static constexpr bool kModelOut = true;
    static constexpr float kEpsilonModel = AKZ_HOMOGRAPHY_EPSILON_MODEL;
    static constexpr float kRefitEpsilon = AKZ_HOMOGRAPHY_EPSILON_MODEL;
    static constexpr int kGuidedKind = AKZ_GUIDED_HOMOGRAPHY;
    static constexpr const char* kName = "match_features_homography_pairs: ";
};

// match_features over many pairs (see the header), the samples drawn on the host: between pairs_front and pairs_tail the samples
// of every pair with K matches or more are drawn on the calling thread in pair order, in chunks whose trials (launch::pairs_trials)
// run while the next chunk is drawn.  A RefineStage or a GuidedStage needs a model that is handed back (kModelOut).
template <class Model>
int match_pairs_impl(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs, uint64_t n_pairs, uint64_t desc_bytes,
                     double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers, akz_match* out, uint64_t* n_out, float* model_out,
                     int* found_out, const GuidedStage* guided = nullptr, const RefineStage* refine = nullptr,
                     const char* name = Model::kName) {  // name: the prefix of the entry point's error texts
    constexpr int K = Model::K;
    if (n_pairs == 0) return AKZ_OK;
    if (guided && !(guided->radius >= 0.0f && std::isfinite(guided->radius))) {
        set_error(std::string(name) + "guided_radius must be finite and >= 0");
        return AKZ_ERR_INVALID_ARG;
    }
    if (!Model::kModelOut) refine = nullptr;
    constexpr uint32_t kChunk = 16384;  // trials per launch of k_pairs_trials (and per pinned sample slot)
    const size_t b_smp = (size_t)kChunk * 9 * sizeof(uint32_t);
    const PairsCall q{name, c, sets, n_sets, pairs, n_pairs, desc_bytes, out, n_out, nullptr};
    PairsFront f;
    AKZ_TRY(pairs_front(q, lowes_ratio, guided != nullptr, false, 2 * b_smp, 0, f));
    hipStream_t st = c->stream;
    uint32_t* d_smp[2] = {(uint32_t*)f.d_own, (uint32_t*)(f.d_own + b_smp)};
    if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[2], st));
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    // the trials of every pair with 8 matches or more, in pair order; the kept lists side by side
    uint64_t n_trials = 0, n_keep = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        launch::PairJobHost& j = f.tab[(size_t)p];
        const uint64_t n = f.h_cnt[j.cnt_idx];
        j.trial_off = n_trials;
        j.n_trials = n >= (uint64_t)K ? ransac_trials : 0;  // (the pair's trials, for the pick)
        j.keep_off = n_keep;
        n_keep += n;
        n_trials += j.n_trials;
    }
    const size_t b_mdl = up256((size_t)std::max<uint64_t>(n_trials, 1) * 36), b_inl = up256((size_t)std::max<uint64_t>(n_trials, 1) * 4);
    // (a model handed back: every pair's 9 floats and found flag between the counts and the kept lists)
    PairsKeep keep{Model::kModelOut ? up256((size_t)n_pairs * 36) : 0, Model::kModelOut ? up256((size_t)n_pairs * 4) : 0,
                   refine ? up256((size_t)n_pairs * 4) : 0, 0};
    AKZ_TRY(ensure(c, c->mp_trials, b_mdl + b_inl));
    AKZ_TRY(pairs_keep(c, f, n_keep, keep));
    for (int i = 0; i < 2; ++i) {
        AKZ_TRY(ensure_pinned(c, c->mp_pin_smp[i], b_smp));
        AKZ_TRY(c->mp_smp_ev[i].ensure());
    }
    float* d_mdl = (float*)c->mp_trials.p;
    int32_t* d_inl = (int32_t*)((char*)c->mp_trials.p + b_mdl);
    AKZ_TRY(pairs_table_upload(c, f));
    // draws on this thread, in pair order; a full slot goes to the device and its trials start while the next one fills
    double t_draw = 0.0;
    DefaultSource& src = default_source();
    int slot = 0;
    uint32_t fill = 0;
    uint64_t chunk_first = 0;
    bool launched = false;
    uint32_t* hs = nullptr;
    auto flush = [&]() -> int {
        if (fill == 0) return AKZ_OK;
        // (the slot's samples of fill trials sit at the front, then their pairs: close the gap)
        std::memmove(hs + (size_t)fill * K, hs + (size_t)kChunk * K, (size_t)fill * 4);
        AKZ_HIP_TRY(hipMemcpyAsync(d_smp[slot], hs, (size_t)fill * (K + 1) * 4, hipMemcpyHostToDevice, st));
        AKZ_HIP_TRY(hipEventRecord(c->mp_smp_ev[slot], st));
        if (f.timed && !launched) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[3], st));
        launched = true;
        launch::pairs_trials(st, Model::kKind, f.d_tab, d_smp[slot], chunk_first, fill, f.d_cnt, f.d_pts, f.cap1, Model::kEpsilonModel,
                             ransac_epsilon_inliers, d_mdl, d_inl);
        AKZ_HIP_TRY(hipGetLastError());
        chunk_first += fill;
        fill = 0;
        slot ^= 1;
        hs = nullptr;
        return AKZ_OK;
    };
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const uint64_t n = f.h_cnt[f.tab[(size_t)p].cnt_idx];
        if (n < (uint64_t)K) continue;
        for (uint64_t left = ransac_trials; left;) {
            if (!hs) {  // the slot's previous copy must be done before it is written again
                AKZ_HIP_TRY(hipEventSynchronize(c->mp_smp_ev[slot]));
                hs = (uint32_t*)c->mp_pin_smp[slot].p;
            }
            const uint32_t take = (uint32_t)std::min<uint64_t>(left, kChunk - fill);
            const double t0 = now_ms();
            draw_samples<K>(src, n, take, hs + (size_t)fill * K);
            t_draw += now_ms() - t0;
            for (uint32_t t = 0; t < take; ++t) hs[(size_t)kChunk * K + fill + t] = (uint32_t)p;
            fill += take;
            left -= take;
            if (fill == kChunk) AKZ_TRY(flush());
        }
    }
    AKZ_TRY(flush());
    if (f.timed) {
        if (!launched) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[3], st));
        AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[4], st));
    }
    return pairs_tail(q, f, keep, Model::kKind, d_mdl, d_inl, ransac_epsilon_inliers, refine, Model::kRefitEpsilon, guided, Model::kGuidedKind, t_draw,
                      model_out, found_out, refine ? refine->iterations : nullptr, nullptr);
}
// One pair: the pairs call with sets {0, 1} and the pair (0, 1).  refine_iterations / g: null without that stage.  H is copied out only
// when found; F always (zeros without a winner, as akz_remove_outliers_fundamental), and its refusals inside the pairs call carry `name`.
template <class Model>
int match_single(const char* name, akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0, const akz_keypoint* kp1,
                 uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                 float ransac_epsilon_inliers, const uint32_t* refine_iterations, const GuidedStage* g, akz_match* out, uint64_t* n_out, float* m,
                 int* found, uint32_t* iterations) {
    constexpr bool homography = Model::kKind == launch::RansacModel::Homography;
    if (!n_out) {
        set_error(std::string(name) + "null n_out");
        return AKZ_ERR_INVALID_ARG;
    }
    if (n_d0 > n_kp0 || n_d1 > n_kp1) {
        set_error(std::string(name) + "a feature set has more descriptors than keypoints");
        return AKZ_ERR_INVALID_ARG;
    }
    const akz_feature_set sets[2] = {{kp0, n_kp0, d0, n_d0}, {kp1, n_kp1, d1, n_d1}};
    const uint64_t pair[2] = {0, 1};
    int fnd = 0;
    float mdl[9] = {};
    uint32_t it = 0;
    const RefineStage r{refine_iterations ? *refine_iterations : 0u, &it};
    AKZ_TRY(match_pairs_impl<Model>(c, sets, 2, pair, 1, desc_bytes, lowes_ratio, ransac_trials, ransac_epsilon_inliers, out, n_out, mdl, &fnd, g,
                                    refine_iterations ? &r : nullptr, homography ? Model::kName : name));
    if (found) *found = fnd;
    if (m && (fnd || !homography)) std::memcpy(m, mdl, sizeof(mdl));
    if (iterations) *iterations = it;
    return AKZ_OK;
}
}  // namespace

extern "C" {
int akz_match_features_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs, uint64_t n_pairs,
                             uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers,
                             akz_match* out, uint64_t* n_out) {
    return match_pairs_impl<FundamentalModel>(c, sets, n_sets, pairs, n_pairs, desc_bytes, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                              out, n_out, nullptr, nullptr);
}

int akz_debug_match_pairs_split(akz_ctx* c, int enable, double* ms) {
    if (!c) {
        set_error("null context");
        return AKZ_ERR_INVALID_ARG;
    }
    c->mp_split_on = enable != 0;
    if (ms)
        for (int k = 0; k < 6; ++k) ms[k] = c->mp_split_ms[k];
    return AKZ_OK;
}

// ---- the homography RANSAC (see the header): 4-point samples; with the guided scan as the last stage; with the refit stage ----
int akz_match_features_homography_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs, uint64_t n_pairs,
                                        uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers,
                                        akz_match* out, uint64_t* n_out, float* h, int* found) {
    return match_pairs_impl<HomographyModel>(c, sets, n_sets, pairs, n_pairs, desc_bytes, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                             out, n_out, h, found);
}
int akz_match_features_homography_guided_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                               uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                               float ransac_epsilon_inliers, float guided_radius, double guided_lowes_ratio, akz_match* out,
                                               uint64_t* n_out, float* h, int* found) {
    const GuidedStage g{guided_radius, guided_lowes_ratio};
    return match_pairs_impl<HomographyModel>(c, sets, n_sets, pairs, n_pairs, desc_bytes, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                             out, n_out, h, found, &g);
}
int akz_match_features_homography_refined_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                                uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                                float ransac_epsilon_inliers, uint32_t refine_iterations, akz_match* out, uint64_t* n_out,
                                                float* h, int* found, uint32_t* iterations) {
    const RefineStage r{refine_iterations, iterations};
    return match_pairs_impl<HomographyModel>(c, sets, n_sets, pairs, n_pairs, desc_bytes, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                             out, n_out, h, found, nullptr, &r);
}
int akz_match_features_homography_refined_guided_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                                       uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                                       float ransac_epsilon_inliers, uint32_t refine_iterations, float guided_radius,
                                                       double guided_lowes_ratio, akz_match* out, uint64_t* n_out, float* h, int* found,
                                                       uint32_t* iterations) {
    const GuidedStage g{guided_radius, guided_lowes_ratio};
    const RefineStage r{refine_iterations, iterations};
    return match_pairs_impl<HomographyModel>(c, sets, n_sets, pairs, n_pairs, desc_bytes, lowes_ratio, ransac_trials, ransac_epsilon_inliers,
                                             out, n_out, h, found, &g, &r);
}
// (refusals are those of akz_match_features: a null n_out sets no text)
int akz_match_features_homography(akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0,
                                  const akz_keypoint* kp1, uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes,
                                  double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers, akz_match* out,
                                  uint64_t* n_out, float* h, int* found) {
    if (!n_out) return AKZ_ERR_INVALID_ARG;
    return match_single<HomographyModel>("match_features_homography: ", c, kp0, n_kp0, d0, n_d0, kp1, n_kp1, d1, n_d1, desc_bytes, lowes_ratio,
                                         ransac_trials, ransac_epsilon_inliers, nullptr, nullptr, out, n_out, h, found, nullptr);
}
int akz_match_features_homography_guided(akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0,
                                         const akz_keypoint* kp1, uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes,
                                         double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers, float guided_radius,
                                         double guided_lowes_ratio, akz_match* out, uint64_t* n_out, float* h, int* found) {
    const GuidedStage g{guided_radius, guided_lowes_ratio};
    return match_single<HomographyModel>("match_features_homography_guided: ", c, kp0, n_kp0, d0, n_d0, kp1, n_kp1, d1, n_d1, desc_bytes,
                                         lowes_ratio, ransac_trials, ransac_epsilon_inliers, nullptr, &g, out, n_out, h, found, nullptr);
}
int akz_match_features_homography_refined(akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0,
                                          const akz_keypoint* kp1, uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes,
                                          double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers,
                                          uint32_t refine_iterations, akz_match* out, uint64_t* n_out, float* h, int* found,
                                          uint32_t* iterations) {
    return match_single<HomographyModel>("match_features_homography_refined: ", c, kp0, n_kp0, d0, n_d0, kp1, n_kp1, d1, n_d1, desc_bytes,
                                         lowes_ratio, ransac_trials, ransac_epsilon_inliers, &refine_iterations, nullptr, out, n_out, h, found,
                                         iterations);
}
int akz_match_features_homography_refined_guided(akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0,
                                                 const akz_keypoint* kp1, uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1,
                                                 uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                                 float ransac_epsilon_inliers, uint32_t refine_iterations, float guided_radius,
                                                 double guided_lowes_ratio, akz_match* out, uint64_t* n_out, float* h, int* found,
                                                 uint32_t* iterations) {
    const GuidedStage g{guided_radius, guided_lowes_ratio};
    return match_single<HomographyModel>("match_features_homography_refined_guided: ", c, kp0, n_kp0, d0, n_d0, kp1, n_kp1, d1, n_d1, desc_bytes,
                                         lowes_ratio, ransac_trials, ransac_epsilon_inliers, &refine_iterations, &g, out, n_out, h, found,
                                         iterations);
}

// ---- the fundamental matrix handed back, refitted, and guiding (see the header) ---------------------------------------------
int akz_match_features_fundamental_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs, uint64_t n_pairs,
                                         uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers,
                                         akz_match* out, uint64_t* n_out, float* f, int* found) {
    return match_pairs_impl<FundamentalModelOut>(c, sets, n_sets, pairs, n_pairs, desc_bytes, lowes_ratio, ransac_trials,
                                                 ransac_epsilon_inliers, out, n_out, f, found);
}
int akz_match_features_fundamental_refined_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                                 uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                                 float ransac_epsilon_inliers, uint32_t refine_iterations, akz_match* out, uint64_t* n_out,
                                                 float* f, int* found, uint32_t* iterations) {
    const RefineStage r{refine_iterations, iterations};
    return match_pairs_impl<FundamentalModelOut>(c, sets, n_sets, pairs, n_pairs, desc_bytes, lowes_ratio, ransac_trials,
                                                 ransac_epsilon_inliers, out, n_out, f, found, nullptr, &r,
                                                 "match_features_fundamental_refined_pairs: ");
}
int akz_match_features_fundamental_guided_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                                uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                                float ransac_epsilon_inliers, float guided_radius, double guided_lowes_ratio, akz_match* out,
                                                uint64_t* n_out, float* f, int* found) {
    const GuidedStage g{guided_radius, guided_lowes_ratio};
    return match_pairs_impl<FundamentalModelOut>(c, sets, n_sets, pairs, n_pairs, desc_bytes, lowes_ratio, ransac_trials,
                                                 ransac_epsilon_inliers, out, n_out, f, found, &g, nullptr,
                                                 "match_features_fundamental_guided_pairs: ");
}
int akz_match_features_fundamental_refined_guided_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                                        uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                                        float ransac_epsilon_inliers, uint32_t refine_iterations, float guided_radius,
                                                        double guided_lowes_ratio, akz_match* out, uint64_t* n_out, float* f, int* found,
                                                        uint32_t* iterations) {
    const GuidedStage g{guided_radius, guided_lowes_ratio};
    const RefineStage r{refine_iterations, iterations};
    return match_pairs_impl<FundamentalModelOut>(c, sets, n_sets, pairs, n_pairs, desc_bytes, lowes_ratio, ransac_trials,
                                                 ransac_epsilon_inliers, out, n_out, f, found, &g, &r,
                                                 "match_features_fundamental_refined_guided_pairs: ");
}
int akz_match_features_fundamental(akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0,
                                   const akz_keypoint* kp1, uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes,
                                   double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers, akz_match* out, uint64_t* n_out,
                                   float* f, int* found) {
    return match_single<FundamentalModelOut>("match_features_fundamental: ", c, kp0, n_kp0, d0, n_d0, kp1, n_kp1, d1, n_d1, desc_bytes,
                                             lowes_ratio, ransac_trials, ransac_epsilon_inliers, nullptr, nullptr, out, n_out, f, found, nullptr);
}
int akz_match_features_fundamental_refined(akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0,
                                           const akz_keypoint* kp1, uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes,
                                           double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers,
                                           uint32_t refine_iterations, akz_match* out, uint64_t* n_out, float* f, int* found,
                                           uint32_t* iterations) {
    return match_single<FundamentalModelOut>("match_features_fundamental_refined: ", c, kp0, n_kp0, d0, n_d0, kp1, n_kp1, d1, n_d1, desc_bytes,
                                             lowes_ratio, ransac_trials, ransac_epsilon_inliers, &refine_iterations, nullptr, out, n_out, f, found, iterations);
}
int akz_match_features_fundamental_guided(akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0,
                                          const akz_keypoint* kp1, uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes,
                                          double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers, float guided_radius,
                                          double guided_lowes_ratio, akz_match* out, uint64_t* n_out, float* f, int* found) {
    const GuidedStage g{guided_radius, guided_lowes_ratio};
    return match_single<FundamentalModelOut>("match_features_fundamental_guided: ", c, kp0, n_kp0, d0, n_d0, kp1, n_kp1, d1, n_d1, desc_bytes,
                                             lowes_ratio, ransac_trials, ransac_epsilon_inliers, nullptr, &g, out, n_out, f, found, nullptr);
}
int akz_match_features_fundamental_refined_guided(akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0,
                                                  const akz_keypoint* kp1, uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1,
                                                  uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                                  float ransac_epsilon_inliers, uint32_t refine_iterations, float guided_radius,
                                                  double guided_lowes_ratio, akz_match* out, uint64_t* n_out, float* f, int* found,
                                                  uint32_t* iterations) {
    const GuidedStage g{guided_radius, guided_lowes_ratio};
    return match_single<FundamentalModelOut>("match_features_fundamental_refined_guided: ", c, kp0, n_kp0, d0, n_d0, kp1, n_kp1, d1, n_d1, desc_bytes,
                                             lowes_ratio, ransac_trials, ransac_epsilon_inliers, &refine_iterations, &g, out, n_out, f, found, iterations);
}
}  // extern "C"
