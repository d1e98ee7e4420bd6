// Host post-filter of match_features: 8-point fundamental matrix + RANSAC
// (akaze/src/ops/estimate_fundamental_matrix.rs:17-165, called from akaze/src/lib.rs:267-274).
// a tiny host step after the GPU matcher, outside the GPU path.
//
// Reference behaviour reproduced here, quirks included:
//   * fewer than 8 matches: returned unchanged (:107-110);
//   * the design matrix row is [x0*x1, x0*y1, x0, y0*x1, y0*y1, y0, x1, y1, 1] (:26-40) with (x0, y0)
//     from keypoints_0 and (x1, y1) from keypoints_1;
//   * nalgebra's SVD of the 8x9 matrix yields 8 singular values / right vectors; the model is the
//     right singular vector of the SMALLEST OF THOSE 8 (:46-53) — not the null vector of the 9x9
//     problem — accepted only if all 8 singular values exceed epsilon_model (rank == 8, :44);
//   * F = [[v0, v3, v6], [v1, v4, v7], [v2, v5, v8]] (:55-66); error = |p_r^T F p_l| (:79-83);
//   * a model replaces the best one only with strictly more inliers; if no trial yields a model the
//     final model is the zero matrix, whose error is 0, so every match is kept (:112-113, :152-163);
//   * every trial takes `random::default()` (:118).  In the `random` crate 0.12 that is a handle to a
//     THREAD-LOCAL Xorshift128+ source seeded [42, 69], not a fresh generator: successive trials (and later
//     calls, and the debug drawings' random_color) continue one stream.  The crate is not in the reference
//     tree; generator, seed and the persistence are pinned by the reference's own published output
//     test-data/keypoints-1.jpg, whose i-th keypoint disc has the colour of stream values 3i..3i+2
//     (tests/test_reference_outputs.py).  akz_random_seed reseeds the calling thread's source.
// Not reproducible bit for bit (and not a parity target): the HashSet iteration order of the
// 8 sampled indices (random per process) and nalgebra's f32 SVD.  Here the sample is taken in ascending
// index order and the decomposition is a one-sided Jacobi SVD of the 8x9 matrix in f64.
#include <unistd.h>

#include <algorithm>
#include <thread>
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

#include "akz_fmatrix.hpp"
#include "akz_fmatrix_normalised.hpp"
#include "akz_homography.hpp"
#include "akz_fundamental_refit.hpp"
#include "akz_homography_refit.hpp"
#include "akz_internal.hpp"
#include "akz_pool.hpp"

namespace akz {

// `random::default()` of the `random` crate 0.12: one Xorshift128+ source per thread, seeded [42, 69]
DefaultSource& default_source() {
    static thread_local DefaultSource src;
    return src;
}

// the refusals every call over a list of matches shares; `name` is the call's
int refuse_bad_matches(const char* name, const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                       const akz_match* matches, uint64_t n_matches, const akz_match* out, const uint64_t* n_out) {
    if (!n_out || (n_matches && (!matches || !out))) {
        set_error(std::string(name) + ": null pointer");
        return AKZ_ERR_INVALID_ARG;
    }
    for (uint64_t i = 0; i < n_matches; ++i)
        if (matches[i].index_0 >= n0 || matches[i].index_1 >= n1 || !keypoints_0 || !keypoints_1) {
            set_error(std::string(name) + ": match index out of range");
            return AKZ_ERR_INVALID_ARG;
        }
    return AKZ_OK;
}

namespace {

struct Model {
    float f[9];  // row-major 3 x 3
};

// the model of exactly M::K matches (estimate_fundamental_matrix :17-69 for K = 8): *found = 0 is the reference's `None`
template <class M>
int estimate_model(const char* name, const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                   const akz_match* sample, float epsilon, float* model, int* found) {
    if (!keypoints_0 || !keypoints_1 || !sample || !model || !found) {
        set_error(std::string(name) + ": null pointer");
        return AKZ_ERR_INVALID_ARG;
    }
    for (int i = 0; i < M::K; ++i)
        if (sample[i].index_0 >= n0 || sample[i].index_1 >= n1) {
            set_error(std::string(name) + ": match index out of range");
            return AKZ_ERR_INVALID_ARG;
        }
    float x0[M::K], y0[M::K], x1[M::K], y1[M::K], m[9];
    for (int i = 0; i < M::K; ++i) {
        x0[i] = keypoints_0[sample[i].index_0].x; y0[i] = keypoints_0[sample[i].index_0].y;
        x1[i] = keypoints_1[sample[i].index_1].x; y1[i] = keypoints_1[sample[i].index_1].y;
    }
    *found = M::from_sample(x0, y0, x1, y1, epsilon, m) ? 1 : 0;
    if (*found) std::memcpy(model, m, sizeof(m));
    return AKZ_OK;
}

// run_trials(lo, hi) over trials 0 .. num_trials on nthreads host threads (one pool for both RANSAC models)
void run_trials_pooled(uint64_t num_trials, unsigned nthreads, const std::function<void(uint64_t, uint64_t)>& run_trials) {
    if (nthreads <= 1) {
        run_trials(0, num_trials);
        return;
    }
    // the trials go to a pool of host threads that lives as long as the process (starting 16 threads per call was a
    // third of a 1 000-trial call's 1.3 ms); a second caller at the same time starts its own threads, as before
    // The pool is never destroyed (its threads end with the process) and belongs to the process that made it: after a
    // fork() the child inherits the object but none of its threads, so a pid that differs drops it (leaked: joining
    // threads that do not exist would hang) and starts a new one.  A child forked while another thread held pool_m
    // never gets the lock and takes the per-call threads below.
    static std::mutex pool_m;
    static WorkerPool* pool = nullptr;
    static pid_t pool_pid = 0;
    std::unique_lock<std::mutex> lk(pool_m, std::try_to_lock);
    if (lk.owns_lock()) {
        const pid_t me = getpid();
        if (pool && pool_pid != me) pool = nullptr;
        if (!pool || pool->size() < nthreads) {
            if (pool && pool_pid == me) delete pool;
            pool = new WorkerPool(nthreads - 1);
            pool_pid = me;
        }
        // handed out dynamically, four pieces per thread -- unless the pool is wider than this call wants (it was grown by
        // a larger one): then exactly nthreads pieces, so that a small call does not wake sixteen threads
        const uint64_t per = std::max<uint64_t>(1, num_trials / ((pool->size() > nthreads ? 1ull : 4ull) * nthreads));
        const size_t pieces = (size_t)((num_trials + per - 1) / per);
        pool->run(pieces, [&](size_t i) { run_trials((uint64_t)i * per, std::min<uint64_t>(num_trials, ((uint64_t)i + 1) * per)); });
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nthreads; ++t)
            th.emplace_back(run_trials, num_trials * t / nthreads, num_trials * (t + 1) / nthreads);
        for (auto& t : th) t.join();
    }
}

}  // namespace

// The samples of `trials` RANSAC trials over n_matches >= K matches, K ascending indices per trial (8: the fundamental matrix,
// 4: the homography), from `src` in trial order: per trial `set.insert(source.read::<usize>() % matches.len())` until the
// set holds K distinct indices (:117-121), sorted (the reference iterates its HashSet: arbitrary order).  The remainder is the exact `%`: q = mulhi(v, m) with
// m = floor((2^64 - 1) / n) undershoots v / n by at most 2 (q <= v / n < q + 3), so r = v - q n < 3 n needs at most two
// corrections -- one multiplication in place of a 64-bit division per draw.  Both match_features paths draw here.
template <int K, class T>
void draw_samples(DefaultSource& src, uint64_t n_matches, uint64_t trials, T* out) {
    const uint64_t m = ~0ull / n_matches;
    for (uint64_t trial = 0; trial < trials; ++trial) {
        uint64_t picked[K];
        int k = 0;
        while (k < K) {
            const uint64_t v = src.next();
            uint64_t r = v - (uint64_t)(((unsigned __int128)v * m) >> 64) * n_matches;
            if (r >= n_matches) r -= n_matches;
            if (r >= n_matches) r -= n_matches;
            int at = k;  // insertion into the ascending list, unless already drawn
            bool dup = false;
            while (at > 0 && picked[at - 1] >= r) {
                if (picked[at - 1] == r) {
                    dup = true;
                    break;
                }
                --at;
            }
            if (dup) continue;
            for (int j = k; j > at; --j) picked[j] = picked[j - 1];
            picked[at] = r;
            ++k;
        }
        for (int i = 0; i < K; ++i) out[trial * K + i] = (T)picked[i];
    }
}
template void draw_samples<8, uint64_t>(DefaultSource&, uint64_t, uint64_t, uint64_t*);
template void draw_samples<8, uint32_t>(DefaultSource&, uint64_t, uint64_t, uint32_t*);
template void draw_samples<4, uint64_t>(DefaultSource&, uint64_t, uint64_t, uint64_t*);
template void draw_samples<4, uint32_t>(DefaultSource&, uint64_t, uint64_t, uint32_t*);
}  // namespace akz

using namespace akz;

// draw_samples from a source of its own seeded [s0, s1] (tests hold it to the plain `%` loop)
extern "C" int akz_debug_ransac_samples(uint64_t s0, uint64_t s1, uint64_t n_matches, uint64_t trials, uint64_t* out) {
    if (n_matches == 0 || (trials && !out)) {
        set_error("debug_ransac_samples: bad arguments");
        return AKZ_ERR_INVALID_ARG;
    }
    DefaultSource src;
    src.s0 = s0;
    src.s1 = s1;
    draw_samples<8>(src, n_matches, trials, out);
    return AKZ_OK;
}

// the same for k = 8 or 4 indices per trial (the homography draws 4); n_matches < k is refused (the loop could not end)
extern "C" int akz_debug_ransac_samples_k(uint64_t s0, uint64_t s1, uint64_t n_matches, uint64_t trials, int k, uint64_t* out) {
    if ((k != 4 && k != 8) || n_matches < (uint64_t)k || (trials && !out)) {
        set_error("debug_ransac_samples_k: bad arguments (k must be 4 or 8, n_matches >= k)");
        return AKZ_ERR_INVALID_ARG;
    }
    DefaultSource src;
    src.s0 = s0;
    src.s1 = s1;
    if (k == 8) draw_samples<8>(src, n_matches, trials, out);
    else draw_samples<4>(src, n_matches, trials, out);
    return AKZ_OK;
}

// RANSAC on the host for either model (M: FundamentalRansac of akz_fmatrix.hpp, HomographyRansac of akz_homography.hpp).
// The trials are independent once their samples are drawn: the samples come from the thread's random source in trial order
// (as the sequential loop of :111-147 draws them), the models and inlier counts are computed on a few host threads, the
// winner is picked in trial order with the reference's strict `>` from 0 -- the same model as the sequential loop returns
// (12 ms -> 1.5 ms for the 8 000 matches of a 4K pair at 1 000 trials) -- and the final filter runs in match order.  Fewer
// than M::K matches ("Not enough points to do RANSAC."): returned unchanged, nothing drawn.  No trial with an inlier: the zero
// model filters, or (M::kKeepAllWithoutWinner) every match is kept; h and found are written for M::kModelOut only.  Without a
// winner (and with fewer than K matches) the two models that hand a model back differ, by M::kZeroModelOut: the homography
// leaves h untouched (found = 0 says so), the fundamental matrix writes the zero model that it evaluated (found = 0 as well).
// trials_on_device (match_features with a context, the fundamental matrix only): runs the trials elsewhere -- x0 .. y1
// (n_matches floats each), the samples (8 per trial), -> models (9 floats per trial), inliers (-1: no model); AKZ_OK or an
// error (the host path then takes over)
namespace {
template <class M>
int ransac_host(const char* name, const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                const akz_match* matches, uint64_t n_matches, uint64_t num_trials, float epsilon_model, float epsilon_inlier, akz_match* out,
                uint64_t* n_out, float* h, int* found, const TrialsOnDevice& trials_on_device) {
    constexpr int K = M::K;
    AKZ_TRY(refuse_bad_matches(name, keypoints_0, n0, keypoints_1, n1, matches, n_matches, out, n_out));
    if (found) *found = 0;
    if (M::kModelOut && M::kZeroModelOut && h) std::memset(h, 0, 9 * sizeof(float));
    if (n_matches < (uint64_t)K) {
        if (n_matches) std::memcpy(out, matches, n_matches * sizeof(akz_match));
        *n_out = n_matches;
        return AKZ_OK;
    }
    std::vector<uint64_t> samples((size_t)num_trials * K);
    draw_samples<K>(default_source(), n_matches, num_trials, samples.data());
    std::vector<Model> models((size_t)num_trials);
    std::vector<int64_t> inliers((size_t)num_trials, -1);  // -1: no model (rank-deficient or degenerate sample)
    const MatchPoints pt(keypoints_0, keypoints_1, matches, n_matches);
    const float *x0 = pt.x0, *y0 = pt.y0, *x1 = pt.x1, *y1 = pt.y1;
    auto run_trials = [&](uint64_t lo, uint64_t hi) {
        for (uint64_t trial = lo; trial < hi; ++trial) {
            float sx0[K], sy0[K], sx1[K], sy1[K];
            for (int i = 0; i < K; ++i) {
                const uint64_t j = samples[(size_t)trial * K + i];
                sx0[i] = x0[j]; sy0[i] = y0[j]; sx1[i] = x1[j]; sy1[i] = y1[j];
            }
            Model model;
            if (!M::from_sample(sx0, sy0, sx1, sy1, epsilon_model, model.f)) continue;
            int64_t inl = 0;
            for (uint64_t i = 0; i < n_matches; ++i) inl += M::inlier(model.f, x0[i], y0[i], x1[i], y1[i], epsilon_inlier) ? 1 : 0;
            models[(size_t)trial] = model;
            inliers[(size_t)trial] = inl;
        }
    };
    bool on_device = false;
    if (trials_on_device && num_trials <= 0x7fffffffull && n_matches <= 0x7fffffffull) {
        std::vector<uint32_t> smp(samples.begin(), samples.end());
        std::vector<float> mdl((size_t)num_trials * 9);
        std::vector<int32_t> inl((size_t)num_trials);
        if (trials_on_device(x0, y0, x1, y1, (uint32_t)n_matches, smp.data(), (uint32_t)num_trials, epsilon_model, epsilon_inlier, mdl.data(),
                             inl.data()) == AKZ_OK) {
            for (uint64_t t = 0; t < num_trials; ++t) {
                inliers[(size_t)t] = inl[(size_t)t];
                if (inl[(size_t)t] >= 0) std::memcpy(models[(size_t)t].f, &mdl[(size_t)t * 9], sizeof(float) * 9);
            }
            on_device = true;
        }
    }
    // (a model costs ~5-9 us -- the 8 x 9 singular value decomposition -- and an inlier count ~0.3-1 ns per match)
    const unsigned nthreads = (unsigned)std::min<uint64_t>(std::min(host_cpu_share(), 16u),
                                                          std::max<uint64_t>(1, num_trials * (n_matches + 9000) / 2000000));  // ~0.1 ms of work per thread at least
    if (!on_device) run_trials_pooled(num_trials, nthreads, run_trials);
    int64_t max_inliers = 0;
    Model final_model;
    std::memset(&final_model, 0, sizeof(final_model));
    for (uint64_t trial = 0; trial < num_trials; ++trial)
        if (inliers[(size_t)trial] > max_inliers) {
            max_inliers = inliers[(size_t)trial];
            final_model = models[(size_t)trial];
        }
    uint64_t k = 0;
    for (uint64_t i = 0; i < n_matches; ++i)
        if ((M::kKeepAllWithoutWinner && max_inliers == 0) || M::inlier(final_model.f, x0[i], y0[i], x1[i], y1[i], epsilon_inlier))
            out[k++] = matches[i];
    *n_out = k;
    if (M::kModelOut && (max_inliers > 0 || M::kZeroModelOut)) {  // (no winner: final_model is the zero model)
        if (h) std::memcpy(h, final_model.f, sizeof(final_model.f));
        if (found) *found = max_inliers > 0 ? 1 : 0;
    }
    return AKZ_OK;
}
}  // namespace

int akz::remove_outliers_impl(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                              const akz_match* matches, uint64_t n_matches, uint64_t num_trials, float epsilon_model,
                              float epsilon_inlier, akz_match* out, uint64_t* n_out, const TrialsOnDevice& trials_on_device) {
    return ransac_host<FundamentalRansac>("remove_outliers", keypoints_0, n0, keypoints_1, n1, matches, n_matches, num_trials, epsilon_model,
                                          epsilon_inlier, out, n_out, nullptr, nullptr, trials_on_device);
}

extern "C" int akz_remove_outliers(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1,
                                   uint64_t n1, const akz_match* matches, uint64_t n_matches, uint64_t num_trials,
                                   float epsilon_model, float epsilon_inlier, akz_match* out, uint64_t* n_out) {
    return akz::remove_outliers_impl(keypoints_0, n0, keypoints_1, n1, matches, n_matches, num_trials, epsilon_model, epsilon_inlier, out,
                                     n_out, akz::TrialsOnDevice());
}

// ops::estimate_fundamental_matrix::estimate_fundamental_matrix (:17-69) for exactly 8 matches; f = the 3x3 matrix, row-major
extern "C" int akz_estimate_fundamental_matrix(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1,
                                               uint64_t n1, const akz_match* matches8, float epsilon, float* f, int* found) {
    return estimate_model<FundamentalRansac>("estimate_fundamental_matrix", keypoints_0, n0, keypoints_1, n1, matches8, epsilon, f, found);
}

// akz_remove_outliers with the winner handed back (see the header): the same skeleton, the same draws, the same list
extern "C" int akz_remove_outliers_fundamental(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                               const akz_match* matches, uint64_t n_matches, uint64_t num_trials, float epsilon_model,
                                               float epsilon_inlier, akz_match* out, uint64_t* n_out, float* f, int* found) {
    return ransac_host<FundamentalRansacModelOut>("remove_outliers_fundamental", keypoints_0, n0, keypoints_1, n1, matches, n_matches,
                                                  num_trials, epsilon_model, epsilon_inlier, out, n_out, f, found, TrialsOnDevice());
}

// ---- the homography (no reference counterpart; akz_homography.hpp) ------------------------------------------
extern "C" int akz_estimate_homography(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                       const akz_match* matches4, float epsilon, float* h, int* found) {
    return estimate_model<HomographyRansac>("estimate_homography", keypoints_0, n0, keypoints_1, n1, matches4, epsilon, h, found);
}

extern "C" int akz_remove_outliers_homography(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                              const akz_match* matches, uint64_t n_matches, uint64_t num_trials, float epsilon_model,
                                              float epsilon_inlier, akz_match* out, uint64_t* n_out, float* h, int* found) {
    return ransac_host<HomographyRansac>("remove_outliers_homography", keypoints_0, n0, keypoints_1, n1, matches, n_matches, num_trials,
                                         epsilon_model, epsilon_inlier, out, n_out, h, found, TrialsOnDevice());
}

// ---- the refit of a model on its inliers (akz_homography_refit.hpp, akz_fundamental_refit.hpp) -----------------
namespace {
// the loop of the statement (refit_loop_host) over a list of matches; `name` is the call's, `what` its model argument
template <class R>
int refine_host(const char* name, const char* what, const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                const akz_match* matches, uint64_t n_matches, const float* h_in, float epsilon_model, float epsilon_inlier,
                uint32_t max_iterations, akz_match* out, uint64_t* n_out, float* h_out, uint32_t* iterations) {
    AKZ_TRY(refuse_bad_matches(name, keypoints_0, n0, keypoints_1, n1, matches, n_matches, out, n_out));
    if (!h_in) {
        set_error(std::string(name) + ": null " + what);
        return AKZ_ERR_INVALID_ARG;
    }
    if (!(epsilon_inlier > 0.0f && std::isfinite(epsilon_inlier))) {
        set_error(std::string(name) + ": epsilon_inlier must be finite and > 0");
        return AKZ_ERR_INVALID_ARG;
    }
    const MatchPoints pt(keypoints_0, keypoints_1, matches, n_matches);
    float h[9];
    std::memcpy(h, h_in, sizeof(h));
    std::vector<uint8_t> member((size_t)n_matches);
    const uint32_t done = refit_loop_host<R>(pt, n_matches, h, epsilon_model, epsilon_inlier, max_iterations, member);
    uint64_t k = 0;
    for (uint64_t i = 0; i < n_matches; ++i)
        if (member[(size_t)i]) out[k++] = matches[i];
    *n_out = k;
    if (h_out) std::memcpy(h_out, h, sizeof(h));
    if (iterations) *iterations = done;
    return AKZ_OK;
}
}  // namespace

extern "C" int akz_refine_homography(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                     const akz_match* matches, uint64_t n_matches, const float* h_in, float epsilon_inlier,
                                     uint32_t max_iterations, akz_match* out, uint64_t* n_out, float* h_out, uint32_t* iterations) {
    return refine_host<HomographyRefit>("refine_homography", "h_in", keypoints_0, n0, keypoints_1, n1, matches, n_matches, h_in,
                                        AKZ_HOMOGRAPHY_EPSILON_MODEL, epsilon_inlier, max_iterations, out, n_out, h_out, iterations);
}

extern "C" int akz_refine_fundamental_matrix(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                             const akz_match* matches, uint64_t n_matches, const float* f_in, float epsilon_inlier,
                                             uint32_t max_iterations, akz_match* out, uint64_t* n_out, float* f_out, uint32_t* iterations) {
    return refine_host<FundamentalRefit>("refine_fundamental_matrix", "f_in", keypoints_0, n0, keypoints_1, n1, matches, n_matches, f_in,
                                         AKZ_FUNDAMENTAL_REFIT_EPSILON, epsilon_inlier, max_iterations, out, n_out, f_out, iterations);
}

// ---- the normalised 8-point model of the seeded family (akz_fmatrix_normalised.hpp) -----------------------------
// one sample: fit(S) of the refit over exactly eight matches, in ascending order
extern "C" int akz_estimate_fundamental_normalised(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                                   const akz_match* matches8, float* f, int* found) {
    return estimate_model<FundamentalNormalisedRansac>("estimate_fundamental_normalised", keypoints_0, n0, keypoints_1, n1, matches8,
                                                       AKZ_FUNDAMENTAL_REFIT_EPSILON, f, found);
}

// akz_refine_fundamental_matrix with the Sampson rule of that model
extern "C" int akz_refine_fundamental_normalised(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                                 const akz_match* matches, uint64_t n_matches, const float* f_in, float epsilon_inlier,
                                                 uint32_t max_iterations, akz_match* out, uint64_t* n_out, float* f_out, uint32_t* iterations) {
    return refine_host<FundamentalNormalisedRefit>("refine_fundamental_normalised", "f_in", keypoints_0, n0, keypoints_1, n1, matches,
                                                   n_matches, f_in, AKZ_FUNDAMENTAL_REFIT_EPSILON, epsilon_inlier, max_iterations, out, n_out,
                                                   f_out, iterations);
}

// random::default().seed([s0, s1]) for the calling thread
extern "C" int akz_random_seed(uint64_t s0, uint64_t s1) {
    DefaultSource& src = default_source();
    src.s0 = s0;
    src.s1 = s1;
    return AKZ_OK;
}
