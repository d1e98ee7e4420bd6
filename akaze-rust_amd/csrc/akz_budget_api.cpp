// The keypoint budget (additions; include/akaze_hip.h): at most N keypoints of a set, the strongest or -- adaptive
// non-maximal suppression -- the best spread.  akz_keypoint_budget_host is the statement: plain f32 loops and a sort.
// akz_keypoint_budget_sets runs it over many sets on the GPU (akz_budget.hip): one upload, the radius and rank passes of
// k_budget_walk, one compaction per set, one download.  Nothing here touches an extraction or a matching call.  The call is two
// halves: budget_enqueue (plan, upload, kernels), which the budgeted bank (akz_bank_api.cpp) shares and stops after, and the download.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "akz_ctx.hpp"

// every refusal that does not depend on a set's keypoints; `name` ends in ": "
bool budget_options_ok(const char* name, const akz_keypoint_budget* opt, const void* indices, const void* n_out, const void* radius2) {
    if (!opt || !indices || !n_out) {
        set_error(std::string(name) + "null options, indices or n_out");
        return false;
    }
    if (opt->mode != AKZ_BUDGET_STRONGEST && opt->mode != AKZ_BUDGET_SPREAD) {
        set_error(std::string(name) + "unknown mode " + std::to_string(opt->mode));
        return false;
    }
    if (opt->mode == AKZ_BUDGET_SPREAD && !(opt->robust > 0.0f && opt->robust <= 1.0f)) {
        set_error(std::string(name) + "robust must lie in (0, 1]");
        return false;
    }
    if (opt->mode == AKZ_BUDGET_STRONGEST && radius2) {
        set_error(std::string(name) + "radius2 is an output of the SPREAD mode only");
        return false;
    }
    return true;
}

// ... and those of one set; `what` names it ("" or "set 3: ")
bool budget_set_ok(const char* name, const std::string& what, const akz_keypoint* k, uint64_t n) {
    if (n > kBudgetMaxKeypoints) {
        set_error(std::string(name) + what + "more than 2^31 - 1 keypoints");
        return false;
    }
    if (n && !k) {
        set_error(std::string(name) + what + "null keypoints");
        return false;
    }
    for (uint64_t i = 0; i < n; ++i)
        if (!std::isfinite(k[i].x) || !std::isfinite(k[i].y) || !std::isfinite(k[i].response)) {
            set_error(std::string(name) + what + "keypoint " + std::to_string(i) + " has an x, y or response that is not finite");
            return false;
        }
    return true;
}

namespace {

// the statement for one checked set
void budget_statement(const akz_keypoint* k, uint64_t n64, const akz_keypoint_budget& o, uint64_t* indices, uint64_t* n_out, float* radius2) {
    const size_t n = (size_t)n64;
    const size_t keep = (size_t)std::min<uint64_t>(o.max_keypoints, n64);
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> x(n), y(n), r(n), rad(n, inf);
    for (size_t i = 0; i < n; ++i) x[i] = k[i].x, y[i] = k[i].y, r[i] = k[i].response;
    if (o.mode == AKZ_BUDGET_SPREAD) {
        std::vector<float> rr(n);
        for (size_t j = 0; j < n; ++j) rr[j] = o.robust * r[j];
        for (size_t i = 0; i < n; ++i) {
            const float xi = x[i], yi = y[i], ri = r[i];
            float m = inf;
            for (size_t j = 0; j < n; ++j) {
                const float dx = xi - x[j], dy = yi - y[j];
                const float xx = dx * dx, yy = dy * dy;
                const float d2 = xx + yy;
                m = (ri < rr[j] && d2 < m) ? d2 : m;
            }
            rad[i] = m;
        }
        if (radius2) std::copy(rad.begin(), rad.end(), radius2);
    }
    std::vector<uint32_t> ord(n);
    std::iota(ord.begin(), ord.end(), 0u);
    std::partial_sort(ord.begin(), ord.begin() + (ptrdiff_t)keep, ord.end(), [&](uint32_t a, uint32_t b) {
        if (rad[a] != rad[b]) return rad[a] > rad[b];
        if (r[a] != r[b]) return r[a] > r[b];
        return a < b;
    });
    std::sort(ord.begin(), ord.begin() + (ptrdiff_t)keep);
    for (size_t t = 0; t < keep; ++t) indices[t] = ord[t];
    *n_out = keep;
}

}  // namespace

// The plan / enqueue half of akz_keypoint_budget_sets (akz_ctx.hpp), which the budgeted bank stops after
int budget_enqueue(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const akz_keypoint_budget& o, BudgetPlan& p) {
    const bool spread = o.mode == AKZ_BUDGET_SPREAD;
    // the set table, and the walk's workgroups: every query tile of a set against train chunks of one length for the whole call, as
    // short as fills the chip (about 2 048 workgroups) and a multiple of the LDS stage
    std::vector<launch::BudgetSet>& tab = p.tab;
    tab.assign((size_t)n_sets, launch::BudgetSet{});
    const uint32_t qt = launch::budget_query_tile(), tt = launch::budget_train_tile();
    double work = 0.0;
    uint32_t base = 0, kept = 0;
    for (uint64_t s = 0; s < n_sets; ++s) {
        const uint32_t n = (uint32_t)sets[s].n_keypoints;
        const uint32_t keep = (uint32_t)std::min<uint64_t>(o.max_keypoints, n);
        tab[(size_t)s] = launch::BudgetSet{base, n, keep, kept};
        base += n;
        kept += keep;
        work += (double)n * (double)n;
    }
    const uint32_t total = base;
    p.total = total, p.kept = kept;
    if (total == 0) return AKZ_OK;
    const double per_block = std::max((double)qt * tt, work / 2048.0);
    const uint32_t chunk = (uint32_t)std::min<double>(std::ceil(per_block / qt / tt) * tt, 1u << 30);
    std::vector<launch::BudgetBlock> blocks;
    for (uint64_t s = 0; s < n_sets; ++s) {
        const uint32_t n = tab[(size_t)s].n;
        for (uint32_t q0 = 0; q0 < n; q0 += qt)
            for (uint32_t t0 = 0; t0 < n; t0 += chunk) blocks.push_back(launch::BudgetBlock{(uint32_t)s, q0, t0, (uint32_t)std::min<uint64_t>((uint64_t)t0 + chunk, n)});
    }
    // device: x | y | r | set table | block table (the upload), rank, then kept indices | radius2 (the download)
    const size_t b_f = up256((size_t)total * 4), b_tab = up256(tab.size() * sizeof(launch::BudgetSet)),
                 b_blk = up256(blocks.size() * sizeof(launch::BudgetBlock)), b_idx = up256((size_t)kept * 4);
    const size_t b_up = 3 * b_f + b_tab + b_blk;
    AKZ_TRY(ensure(c, c->kb_dev, b_up + b_f + b_idx + b_f));
    AKZ_TRY(ensure_pinned(c, c->kb_pin, b_up + b_idx + b_f));
    const bool timed = c->kb_split_on;
    if (timed)
        for (Event& e : c->kb_split_ev) AKZ_TRY(e.ensure(hipEventDefault));
    char *d = (char*)c->kb_dev.p, *h = (char*)c->kb_pin.p;
    float *hx = (float*)h, *hy = (float*)(h + b_f), *hr = (float*)(h + 2 * b_f);
    for (uint64_t s = 0; s < n_sets; ++s) {
        const akz_keypoint* k = sets[s].keypoints;
        const size_t at = tab[(size_t)s].base;
        for (size_t i = 0; i < tab[(size_t)s].n; ++i) hx[at + i] = k[i].x, hy[at + i] = k[i].y, hr[at + i] = k[i].response;
    }
    std::memcpy(h + 3 * b_f, tab.data(), tab.size() * sizeof(launch::BudgetSet));
    std::memcpy(h + 3 * b_f + b_tab, blocks.data(), blocks.size() * sizeof(launch::BudgetBlock));
    hipStream_t st = c->stream;
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->kb_split_ev[0], st));
    AKZ_HIP_TRY(hipMemcpyAsync(d, h, b_up, hipMemcpyHostToDevice, st));
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->kb_split_ev[1], st));
    uint32_t* d_rank = (uint32_t*)(d + b_up);
    uint32_t* d_idx = (uint32_t*)(d + b_up + b_f);
    float* d_rad = (float*)(d + b_up + b_f + b_idx);
    launch::budget(st, spread, o.robust, (const float*)d, (const float*)(d + b_f), (const float*)(d + 2 * b_f), total,
                   (const launch::BudgetSet*)(d + 3 * b_f), (uint32_t)n_sets, (const launch::BudgetBlock*)(d + 3 * b_f + b_tab),
                   (uint32_t)blocks.size(), d_rad, d_rank, d_idx);
    AKZ_HIP_TRY(hipGetLastError());
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->kb_split_ev[2], st));
    p.d_x = (const float*)d, p.d_y = (const float*)(d + b_f), p.d_r = (const float*)(d + 2 * b_f);
    p.d_idx = d_idx, p.b_idx = b_idx;
    p.h_down = h + b_up;
    return AKZ_OK;
}

extern "C" {

int akz_keypoint_budget_host(const akz_keypoint* keypoints, uint64_t n, const akz_keypoint_budget* options, uint64_t* indices,
                             uint64_t* n_out, float* radius2) {
    const char* name = "keypoint_budget_host: ";
    if (!budget_options_ok(name, options, indices, n_out, radius2) || !budget_set_ok(name, "", keypoints, n)) return AKZ_ERR_INVALID_ARG;
    budget_statement(keypoints, n, *options, indices, n_out, radius2);
    return AKZ_OK;
}

int akz_keypoint_budget_sets(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const akz_keypoint_budget* options, uint64_t* indices,
                             uint64_t* n_out, float* radius2) {
    const char* name = "keypoint_budget_sets: ";
    if (n_sets == 0) return AKZ_OK;
    if (!c || !sets) {
        set_error(std::string(name) + (c ? "null sets" : "null context"));
        return AKZ_ERR_INVALID_ARG;
    }
    if (!budget_options_ok(name, options, indices, n_out, radius2)) return AKZ_ERR_INVALID_ARG;
    uint64_t total64 = 0;
    for (uint64_t s = 0; s < n_sets; ++s) {
        if (!budget_set_ok(name, "set " + std::to_string(s) + ": ", sets[s].keypoints, sets[s].n_keypoints)) return AKZ_ERR_INVALID_ARG;
        total64 += sets[s].n_keypoints;
        if (total64 > kBudgetMaxKeypoints) {
            set_error(std::string(name) + "set " + std::to_string(s) + ": the sets of one call hold more than 2^31 - 1 keypoints together");
            return AKZ_ERR_INVALID_ARG;
        }
    }
    AKZ_TRY(bind(c, true, false));
    BudgetPlan p;
    AKZ_TRY(budget_enqueue(c, sets, n_sets, *options, p));
    for (uint64_t s = 0; s < n_sets; ++s) n_out[s] = p.tab[(size_t)s].keep;
    if (p.total == 0) return AKZ_OK;
    // the download: kept indices | radius2
    const bool timed = c->kb_split_on;
    hipStream_t st = c->stream;
    const size_t b_down = p.b_idx + (radius2 ? (size_t)p.total * 4 : 0);
    if (b_down) AKZ_HIP_TRY(hipMemcpyAsync(p.h_down, p.d_idx, b_down, hipMemcpyDeviceToHost, st));
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->kb_split_ev[3], st));
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    const uint32_t* h_idx = (const uint32_t*)p.h_down;
    for (uint64_t s = 0; s < n_sets; ++s) {
        const launch::BudgetSet& b = p.tab[(size_t)s];
        for (uint32_t t = 0; t < b.keep; ++t) indices[(size_t)b.base + t] = h_idx[(size_t)b.out_off + t];
    }
    if (radius2) std::memcpy(radius2, p.h_down + p.b_idx, (size_t)p.total * 4);
    if (timed) {
        float ms[3] = {0.0f, 0.0f, 0.0f};
        for (int i = 0; i < 3; ++i) AKZ_HIP_TRY(hipEventElapsedTime(&ms[i], c->kb_split_ev[i], c->kb_split_ev[i + 1]));
        for (int i = 0; i < 3; ++i) c->kb_split_ms[i] = ms[i];
    }
    return AKZ_OK;
}

int akz_debug_keypoint_budget_split(akz_ctx* c, int enable, double* ms) {  // include/akaze_hip_debug.h
    if (!c) {
        set_error("null context");
        return AKZ_ERR_INVALID_ARG;
    }
    c->kb_split_on = enable != 0;
    if (ms)
        for (int k = 0; k < 3; ++k) ms[k] = c->kb_split_ms[k];
    return AKZ_OK;
}

int akz_debug_keypoint_budget_tiles(uint32_t* query_tile, uint32_t* train_tile) {  // include/akaze_hip_debug.h
    if (!query_tile || !train_tile) return AKZ_ERR_INVALID_ARG;
    *query_tile = launch::budget_query_tile();
    *train_tile = launch::budget_train_tile();
    return AKZ_OK;
}

}  // extern "C"
