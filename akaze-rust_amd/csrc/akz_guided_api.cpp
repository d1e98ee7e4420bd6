// C ABI of libakaze_hip.so, part 5: guided matching -- the host statement, the pair call and the pairs call, which opens as every
// pairs call does (pairs_open) and closes with the copy-out they share (pairs_copy_out); guided_specs and guided_enqueue are also
// the guided stage of the RANSAC pairs calls (pairs_tail, akz_match_api.cpp).
#include "akz_ctx.hpp"
#include "akz_homography.hpp"
#include "akz_match_rule.hpp"

namespace {
// the refusals every guided call shares; false: refused (message set)
bool guided_args_ok(const char* name, int model_kind, const float* model, float radius) {
    if (model_kind != AKZ_GUIDED_HOMOGRAPHY && model_kind != AKZ_GUIDED_FUNDAMENTAL) {
        set_error(std::string(name) + "model_kind must be AKZ_GUIDED_HOMOGRAPHY (0) or AKZ_GUIDED_FUNDAMENTAL (1)");
        return false;
    }
    if (!model) {
        set_error(std::string(name) + "null model");
        return false;
    }
    if (!(radius >= 0.0f && std::isfinite(radius))) {
        set_error(std::string(name) + "radius must be finite and >= 0");
        return false;
    }
    return true;
}
bool pair_args_ok(const char* name, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0, const akz_keypoint* kp1,
                  uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes, const akz_match* out, const uint64_t* n_out) {
    const char* why = nullptr;
    if (!n_out) why = "null n_out";
    else if (desc_bytes == 0 || desc_bytes > 64) why = "desc_bytes must be 1..64";
    else if (n_d0 > n_kp0 || n_d1 > n_kp1) why = "a feature set has more descriptors than keypoints";
    else if (!(why = set_refusal({kp0, n_kp0, d0, n_d0})) && !(why = set_refusal({kp1, n_kp1, d1, n_d1})) && n_d0 && !out)
        why = "null out";  // (the counts have passed: set_refusal can only name the pointers, of set 0 first as before)
    if (why) set_error(std::string(name) + why);
    return why == nullptr;
}
}  // namespace

// The sizes one launch of the guided scan takes, checked with the other refusals before any GPU work: rows of a set below
// 2^31, rows of all sets of the call below 2^32, workgroups (query blocks x at most 64 chunks) below 2^31.
int guided_limits(const char* name, const akz_feature_set* sets, const uint64_t* pairs, uint64_t n_pairs, const std::vector<uint8_t>& seen) {
    uint64_t rows = 0, wg = 0;
    bool ok = true;
    for (size_t k = 0; k < seen.size(); ++k)
        if (seen[k]) {
            ok = ok && sets[k].n_descriptors <= 0x7fffffffull;
            rows += std::min<uint64_t>(sets[k].n_descriptors, 0x100000000ull);
        }
    for (uint64_t p = 0; p < n_pairs && ok; ++p) {
        wg += (sets[pairs[2 * p]].n_descriptors + launch::match_guided_block() - 1) / launch::match_guided_block() * 64;
        ok = wg <= 0x7fffffffull;
    }
    if (!ok || rows > 0xffffffffull) {
        set_error(std::string(name) + "too many rows or pairs for one guided launch");
        return AKZ_ERR_INVALID_ARG;
    }
    return AKZ_OK;
}

std::vector<GuidedPairSpec> guided_specs(const PairsCall& q, const SetsBlock& blk) {
    std::vector<GuidedPairSpec> spec((size_t)q.n_pairs);
    uint64_t off = 0;
    for (uint64_t p = 0; p < q.n_pairs; ++p) {
        const uint64_t a = q.pairs[2 * p], b = q.pairs[2 * p + 1];
        spec[(size_t)p] = GuidedPairSpec{blk.set_row[(size_t)a], q.sets[a].n_descriptors, blk.set_row[(size_t)b], q.sets[b].n_descriptors, off};
        off += q.sets[a].n_descriptors;
    }
    return spec;
}

int guided_enqueue(akz_ctx* c, const std::vector<GuidedPairSpec>& spec, const SetsBlock& b, int kind, const float* d_models, const int32_t* d_found,
                   float radius, uint64_t distance_threshold, double lowes_ratio, akz_match* d_out, uint64_t* d_cnt) {
    hipStream_t st = c->stream;
    const uint32_t thr = akz::clamp_threshold(distance_threshold), block = launch::match_guided_block();
    AKZ_HIP_TRY(hipMemsetAsync(d_cnt, 0, spec.size() * sizeof(uint64_t), st));
    // A pair's train rows are cut into chunks so that the launch fills the chip: 256 compute units take eight workgroups of
    // four waves each, and a chunk should still be a few LDS tiles long (akz_debug_set_match_chunks forces the pair count).
    // (sizes: guided_limits has passed)
    uint64_t qblocks = 0;
    for (const GuidedPairSpec& s : spec)
        if (s.n0 && s.n1) qblocks += (s.n0 + block - 1) / block;
    if (qblocks == 0) return AKZ_OK;
    const uint64_t want = std::max<uint64_t>(1, (2048 + qblocks - 1) / qblocks);
    std::vector<launch::GuidedPairHost> tab;
    uint64_t rec_total = 0, wg = 0;
    for (size_t p = 0; p < spec.size(); ++p) {
        const GuidedPairSpec& s = spec[p];
        if (!s.n0 || !s.n1) continue;
        const uint32_t tiles = (uint32_t)((s.n1 + block - 1) / block);
        uint32_t chunks = c->settings.dbg_pair_chunks ? c->settings.dbg_pair_chunks : (uint32_t)std::min<uint64_t>(want, std::max<uint32_t>(1, tiles / 2));
        chunks = std::max(1u, std::min(std::min(chunks, tiles), 64u));
        const uint32_t chunk_rows = (uint32_t)((s.n1 + chunks - 1) / chunks);
        tab.push_back(launch::GuidedPairHost{rec_total, (uint32_t)s.q_row0, (uint32_t)s.n0, (uint32_t)s.t_row0, (uint32_t)s.n1, (uint32_t)wg,
                                             chunks, chunk_rows, (uint32_t)p});
        rec_total += s.n0 * (chunks + 1);  // (+ 1: the merged records of a pair with many chunks)
        wg += (s.n0 + block - 1) / block * chunks;
    }
    const size_t b_tab = tab.size() * sizeof(launch::GuidedPairHost);
    AKZ_TRY(ensure(c, c->gd_tab, b_tab));
    AKZ_TRY(ensure(c, c->gd_rec, rec_total * sizeof(MatchRec)));
    AKZ_TRY(ensure_pinned(c, c->gd_pin_tab, b_tab));
    AKZ_TRY(table_upload(c, c->gd_tab.p, c->gd_pin_tab.p, tab.data(), b_tab));
    MatchRec* rec = (MatchRec*)c->gd_rec.p;
    launch::match_guided(st, kind, b.d_rows, b.d_kx, b.d_ky, (const launch::GuidedPairHost*)c->gd_tab.p, (uint32_t)tab.size(), (uint32_t)wg, d_models,
                         d_found, radius, thr, rec);
    AKZ_HIP_TRY(hipGetLastError());
    for (const launch::GuidedPairHost& g : tab)
        AKZ_TRY(match_finish(c, rec + g.rec_off, g.n0, g.chunks, thr, lowes_ratio, d_out + spec[g.model].out_off, d_cnt + g.model));
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}

extern "C" {

int akz_descriptor_match_guided_host(const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0, const akz_keypoint* kp1,
                                     uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes, int model_kind,
                                     const float* model, float radius, uint64_t distance_threshold, double lowes_ratio, akz_match* out,
                                     uint64_t* n_out) {
    const char* name = "descriptor_match_guided_host: ";
    if (!pair_args_ok(name, kp0, n_kp0, d0, n_d0, kp1, n_kp1, d1, n_d1, desc_bytes, out, n_out) ||
        !guided_args_ok(name, model_kind, model, radius))
        return AKZ_ERR_INVALID_ARG;
    float m[9];
    std::memcpy(m, model, sizeof(m));
    // feature_matching.rs:37-81 with the gate at the top of the inner loop
    const auto gate = [&](uint64_t i, uint64_t j) {
        return model_kind == AKZ_GUIDED_HOMOGRAPHY ? akz::homography_inlier(m, kp0[i].x, kp0[i].y, kp1[j].x, kp1[j].y, radius)
                                                   : akz::fundamental_near_line(m, kp0[i].x, kp0[i].y, kp1[j].x, kp1[j].y, radius);
    };
    uint64_t cnt = 0;
    akz::host_match_scan(d0, n_d0, d1, n_d1, desc_bytes, akz::clamp_threshold(distance_threshold), lowes_ratio * lowes_ratio, gate,
                         [&](const akz_match& r) { out[cnt++] = r; });
    *n_out = cnt;
    return AKZ_OK;
}

int akz_descriptor_match_guided_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs, uint64_t n_pairs,
                                      uint64_t desc_bytes, int model_kind, const float* models, float radius, uint64_t distance_threshold,
                                      double lowes_ratio, akz_match* out, uint64_t* n_out) {
    const char* name = "descriptor_match_guided_pairs: ";
    if (n_pairs == 0) return AKZ_OK;
    if (!guided_args_ok(name, model_kind, models, radius)) return AKZ_ERR_INVALID_ARG;
    const PairsCall q{name, c, sets, n_sets, pairs, n_pairs, desc_bytes, out, n_out, nullptr};
    PairsFront f;
    AKZ_TRY(pairs_open(q, true, f));
    hipStream_t st = c->stream;
    const size_t b_mdl = up256((size_t)n_pairs * 36);
    AKZ_TRY(ensure(c, c->gd_out, f.b_cnt + b_mdl + (size_t)f.cap1 * sizeof(akz_match)));
    AKZ_TRY(ensure_pinned(c, c->gd_pin_cnt, f.b_cnt + b_mdl));
    uint64_t* d_cnt = (uint64_t*)c->gd_out.p;
    float* d_models = (float*)((char*)c->gd_out.p + f.b_cnt);
    akz_match* d_out = (akz_match*)((char*)c->gd_out.p + f.b_cnt + b_mdl);
    uint64_t* h_cnt = (uint64_t*)c->gd_pin_cnt.p;
    float* h_models = (float*)((char*)c->gd_pin_cnt.p + f.b_cnt);
    AKZ_TRY(pairs_upload(c, sets, desc_bytes, f.block, f.used));
    AKZ_TRY(table_upload(c, d_models, h_models, models, (size_t)n_pairs * 36));
    AKZ_TRY(guided_enqueue(c, guided_specs(q, f.block), f.block, model_kind, d_models, nullptr, radius, distance_threshold, lowes_ratio, d_out, d_cnt));
    AKZ_HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, st));
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    return pairs_copy_out(q, h_cnt, nullptr, d_out, nullptr, nullptr, nullptr);  // every pair's guided list
}

// one pair: the pairs call with sets {0, 1} and the pair (0, 1)
int akz_descriptor_match_guided(akz_ctx* c, const akz_keypoint* kp0, uint64_t n_kp0, const uint8_t* d0, uint64_t n_d0, const akz_keypoint* kp1,
                                uint64_t n_kp1, const uint8_t* d1, uint64_t n_d1, uint64_t desc_bytes, int model_kind, const float* model,
                                float radius, uint64_t distance_threshold, double lowes_ratio, akz_match* out, uint64_t* n_out) {
    const char* name = "descriptor_match_guided: ";
    if (!pair_args_ok(name, kp0, n_kp0, d0, n_d0, kp1, n_kp1, d1, n_d1, desc_bytes, out, n_out) ||
        !guided_args_ok(name, model_kind, model, radius))
        return AKZ_ERR_INVALID_ARG;
    if (!c) {
        set_error(std::string(name) + "null context");
        return AKZ_ERR_INVALID_ARG;
    }
    const akz_feature_set sets[2] = {{kp0, n_kp0, d0, n_d0}, {kp1, n_kp1, d1, n_d1}};
    const uint64_t pair[2] = {0, 1};
    uint64_t cnt = 0;
    AKZ_TRY(akz_descriptor_match_guided_pairs(c, sets, 2, pair, 1, desc_bytes, model_kind, model, radius, distance_threshold, lowes_ratio, out,
                                              &cnt));
    *n_out = cnt;
    return AKZ_OK;
}

}  // extern "C"
