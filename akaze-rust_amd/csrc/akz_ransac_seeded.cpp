// The seeded RANSAC on the host (an addition; include/akaze_hip.h): the statement that
// akz_match_features_seeded_pairs equals bit for bit.  Samples are a pure function of (seed, stream, trial)
// (akz_ransac_seeded.hpp), trials run in rounds of AKZ_RANSAC_ROUND, and a pair stops after the round in which its best inlier
// count reaches need(n, K, trials so far, confidence).  Models and inlier counts are those of akz_ransac.cpp (from_sample and
// inlier of akz_fmatrix.hpp / akz_homography.hpp); the refit is akz_refine_homography / akz_refine_fundamental_matrix.  The
// third kind, AKZ_RANSAC_FUNDAMENTAL_NORMALISED, is this family's alone: the normalised 8-point model and the Sampson rule of
// akz_fmatrix_normalised.hpp, refitted by akz_refine_fundamental_normalised.  One thread, in trial order: this is the
// definition, not a fast path.  The calling thread's default random source is not touched.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "akz_fmatrix.hpp"
#include "akz_fmatrix_normalised.hpp"
#include "akz_homography.hpp"
#include "akz_internal.hpp"
#include "akz_ransac_seeded.hpp"

namespace akz {

// the refusals that the host statement and the GPU call share: the options alone (see the header)
// resection: the calls of akz_resection_api.cpp, whose one kind is AKZ_RANSAC_RESECTION; every other call keeps refusing it
int seeded_refuse_options_of(const char* name, const akz_ransac_options* opt, bool resection) {
    auto refuse = [name](const char* msg) {
        set_error(std::string(name) + msg);
        return AKZ_ERR_INVALID_ARG;
    };
    if (!opt) return refuse("null options");
    if (opt->struct_size != sizeof(akz_ransac_options)) return refuse("options.struct_size is not sizeof(akz_ransac_options)");
    if (resection ? opt->model_kind != AKZ_RANSAC_RESECTION
                  : opt->model_kind != AKZ_GUIDED_HOMOGRAPHY && opt->model_kind != AKZ_GUIDED_FUNDAMENTAL &&
                        opt->model_kind != AKZ_RANSAC_FUNDAMENTAL_NORMALISED)
        return refuse(resection ? "options.model_kind must be AKZ_RANSAC_RESECTION" : "unknown options.model_kind");
    if (opt->max_trials > kSeededMaxTrials) return refuse("options.max_trials must be <= 1 << 24");
    if (!(opt->confidence >= 0.0 && opt->confidence < 1.0)) return refuse("options.confidence must be 0 (off) or 0 < c < 1");
    return AKZ_OK;
}
int seeded_refuse_options(const char* name, const akz_ransac_options* opt) { return seeded_refuse_options_of(name, opt, false); }

namespace {

// `refine`: the refit of the model kind (akz_refine_homography and its kin)
template <class M, class Refine>
int seeded_host(Refine refine, const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1, const akz_match* matches,
                uint64_t n_matches, const akz_ransac_options& opt, uint64_t stream, float epsilon_model, akz_match* out, uint64_t* n_out,
                float* model_out, int* found_out, uint32_t* iterations_out, uint64_t* trials_out) {
    constexpr int K = M::K;
    float best_model[9] = {};
    int64_t best = 0;
    uint64_t trials_run = 0;
    uint32_t iterations = 0;
    uint64_t kept = 0;
    if (n_matches < (uint64_t)K) {
        if (n_matches) std::memcpy(out, matches, n_matches * sizeof(akz_match));
        kept = n_matches;
    } else {
        const MatchPoints pt(keypoints_0, keypoints_1, matches, n_matches);
        const float *x0 = pt.x0, *y0 = pt.y0, *x1 = pt.x1, *y1 = pt.y1;
        float m[9];  // the model of the trial at hand
        seeded_rounds<K>(
            n_matches, opt.seed[0], opt.seed[1], stream, opt.max_trials, opt.confidence,
            [&](const uint64_t(&smp)[K]) -> int64_t {
                float sx0[K], sy0[K], sx1[K], sy1[K];
                for (int i = 0; i < K; ++i) {
                    sx0[i] = x0[smp[i]]; sy0[i] = y0[smp[i]]; sx1[i] = x1[smp[i]]; sy1[i] = y1[smp[i]];
                }
                if (!M::from_sample(sx0, sy0, sx1, sy1, epsilon_model, m)) return -1;
                int64_t inl = 0;
                for (uint64_t i = 0; i < n_matches; ++i) inl += M::inlier(m, x0[i], y0[i], x1[i], y1[i], opt.epsilon_inliers) ? 1 : 0;
                return inl;
            },
            [&] { std::memcpy(best_model, m, sizeof(m)); }, best, trials_run);
        for (uint64_t i = 0; i < n_matches; ++i)
            if ((M::kKeepAllWithoutWinner && best == 0) || M::inlier(best_model, x0[i], y0[i], x1[i], y1[i], opt.epsilon_inliers))
                out[kept++] = matches[i];
        if (best > 0 && opt.refine_iterations > 0) {  // the list, the model and the accepted fits are the refit's
            const float winner[9] = {best_model[0], best_model[1], best_model[2], best_model[3], best_model[4],
                                     best_model[5], best_model[6], best_model[7], best_model[8]};
            AKZ_TRY(refine(keypoints_0, n0, keypoints_1, n1, matches, n_matches, winner, opt.epsilon_inliers, opt.refine_iterations, out, &kept,
                           best_model, &iterations));
        }
    }
    *n_out = kept;
    if (model_out) std::memcpy(model_out, best_model, sizeof(best_model));  // (zeros without a winner, for both models)
    if (found_out) *found_out = best > 0 ? 1 : 0;
    if (iterations_out) *iterations_out = iterations;
    if (trials_out) *trials_out = trials_run;
    return AKZ_OK;
}

}  // namespace
}  // namespace akz

using namespace akz;

extern "C" {

void akz_ransac_options_default(akz_ransac_options* opt) {
    if (!opt) return;
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (uint32_t)sizeof(*opt);
    opt->model_kind = AKZ_GUIDED_FUNDAMENTAL;
    opt->lowes_ratio = 0.86;
    opt->max_trials = 1000;
    opt->epsilon_inliers = 0.02f;
    opt->confidence = 0.99;
    opt->seed[0] = 42;
    opt->seed[1] = 69;
    opt->guided_radius = 3.0f;
    opt->guided_lowes_ratio = 0.86;
}

int akz_draw_sample_seeded(uint64_t seed0, uint64_t seed1, uint64_t stream, uint64_t trial, uint64_t n_matches, int k, uint64_t* out) {
    if ((k != 4 && k != 6 && k != 8) || n_matches < (uint64_t)k || !out) {
        set_error("draw_sample_seeded: bad arguments (k must be 4, 6 or 8, n_matches >= k, out not null)");
        return AKZ_ERR_INVALID_ARG;
    }
    const uint64_t ks = seeded_stream_key(seeded_seed_key(seed0, seed1), stream);
    if (k == 8) {
        uint64_t s[8];
        seeded_sample<8>(ks, trial, n_matches, s);
        std::memcpy(out, s, sizeof(s));
    } else if (k == 6) {
        uint64_t s[6];
        seeded_sample<6>(ks, trial, n_matches, s);
        std::memcpy(out, s, sizeof(s));
    } else {
        uint64_t s[4];
        seeded_sample<4>(ks, trial, n_matches, s);
        std::memcpy(out, s, sizeof(s));
    }
    return AKZ_OK;
}

int akz_ransac_required_inliers(uint64_t n_matches, int k, uint64_t trials, double confidence, uint64_t* need) {
    if ((k != 4 && k != 6 && k != 8) || n_matches == 0 || trials == 0 || !(confidence > 0.0 && confidence < 1.0) || !need) {
        set_error("ransac_required_inliers: bad arguments (k must be 4, 6 or 8, n_matches and trials >= 1, 0 < confidence < 1, need not null)");
        return AKZ_ERR_INVALID_ARG;
    }
    *need = seeded_need(n_matches, k, trials, confidence);
    return AKZ_OK;
}

int akz_remove_outliers_seeded(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                               const akz_match* matches, uint64_t n_matches, const akz_ransac_options* options, uint64_t stream,
                               akz_match* out, uint64_t* n_out, float* model, int* found, uint32_t* iterations, uint64_t* trials_run) {
    const char* name = "remove_outliers_seeded";
    AKZ_TRY(refuse_bad_matches(name, keypoints_0, n0, keypoints_1, n1, matches, n_matches, out, n_out));
    AKZ_TRY(seeded_refuse_options("remove_outliers_seeded: ", options));
    // (the refit's own refusal, up front: nothing is written after one)
    if (options->refine_iterations > 0 && !(options->epsilon_inliers > 0.0f && std::isfinite(options->epsilon_inliers))) {
        set_error("remove_outliers_seeded: with refine_iterations > 0, epsilon_inliers must be finite and > 0");
        return AKZ_ERR_INVALID_ARG;
    }
    if (options->model_kind == AKZ_RANSAC_FUNDAMENTAL_NORMALISED)
        return seeded_host<FundamentalNormalisedRansac>(akz_refine_fundamental_normalised, keypoints_0, n0, keypoints_1, n1, matches, n_matches,
                                                        *options, stream, AKZ_FUNDAMENTAL_REFIT_EPSILON, out, n_out, model, found, iterations,
                                                        trials_run);
    if (options->model_kind == AKZ_GUIDED_FUNDAMENTAL)
        return seeded_host<FundamentalRansac>(akz_refine_fundamental_matrix, keypoints_0, n0, keypoints_1, n1, matches, n_matches, *options,
                                              stream, 0.05f, out, n_out, model, found, iterations, trials_run);
    return seeded_host<HomographyRansac>(akz_refine_homography, keypoints_0, n0, keypoints_1, n1, matches, n_matches, *options, stream,
                                         AKZ_HOMOGRAPHY_EPSILON_MODEL, out, n_out, model, found, iterations, trials_run);
}

}  // extern "C"
