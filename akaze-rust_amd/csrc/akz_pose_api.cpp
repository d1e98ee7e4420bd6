// Relative pose (additions; include/akaze_hip.h): akz_recover_pose_host is the statement of akz_pose.hpp run on the
// host -- no GPU call, no context --, and akz_match_features_seeded_pose_pairs is the seeded pairs call (akz_match_seeded_api.cpp)
// with launch::pairs_pose (akz_pose.hip: the same source on the device) in front of its one read-back.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "akz_ctx.hpp"
#include "akz_pose.hpp"

namespace akz {
int seeded_refuse_options(const char* name, const akz_ransac_options* opt);  // akz_ransac_seeded.cpp
}
using namespace akz;

bool camera_ok(const akz_camera& k) {
    return std::isfinite(k.fx) && std::isfinite(k.fy) && std::isfinite(k.cx) && std::isfinite(k.cy) && k.fx != 0.0 && k.fy != 0.0;
}
namespace {
int refuse(const std::string& what) {
    set_error(what);
    return AKZ_ERR_INVALID_ARG;
}
}  // namespace

extern "C" int akz_recover_pose_host(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                     const akz_match* matches, uint64_t n_matches, const float* f, const akz_camera* camera_0,
                                     const akz_camera* camera_1, akz_match* out, uint64_t* n_out, akz_pose* pose, float* points) {
    AKZ_TRY(refuse_bad_matches("recover_pose_host", keypoints_0, n0, keypoints_1, n1, matches, n_matches, out, n_out));
    if (!f || !camera_0 || !camera_1 || !pose) return refuse("recover_pose_host: null f, camera or pose");
    if (!camera_ok(*camera_0) || !camera_ok(*camera_1)) return refuse("recover_pose_host: a camera needs finite fields and fx, fy != 0");
    const akz_camera k0 = *camera_0, k1 = *camera_1;
    Mat3x9 m;
    PoseCandidates pc;
    float sigma[3];
    const bool ok = pose_decompose(m, f, k0, k1, pc, sigma);
    uint32_t in_front[4] = {0, 0, 0, 0};
    std::vector<uint8_t> bits((size_t)n_matches);
    if (ok)
        for (uint64_t i = 0; i < n_matches; ++i) {
            const akz_keypoint &p = keypoints_0[matches[i].index_0], &q = keypoints_1[matches[i].index_1];
            double a[3], b[3];
            pose_rays(p.x, p.y, q.x, q.y, k0, k1, a, b);
            bits[(size_t)i] = (uint8_t)pose_front(pc, a, b);
            for (int k = 0; k < 4; ++k) in_front[k] += (bits[(size_t)i] >> k) & 1u;
        }
    akz_pose res;
    pose_result(ok, pc, sigma, in_front, res);
    uint64_t kept = 0;
    if (res.found) {
        double r[9], ts[3];
        pose_of_candidate(pc, res.winner, r, ts);
        for (uint64_t i = 0; i < n_matches; ++i) {
            if (!((bits[(size_t)i] >> res.winner) & 1u)) continue;
            if (points) {
                const akz_keypoint &p = keypoints_0[matches[i].index_0], &q = keypoints_1[matches[i].index_1];
                double a[3], b[3];
                float x[3];
                pose_rays(p.x, p.y, q.x, q.y, k0, k1, a, b);
                pose_point(r, ts, a, b, x);
                std::memcpy(points + 3 * kept, x, sizeof(x));
            }
            out[kept++] = matches[i];
        }
    } else {
        for (uint64_t i = 0; i < n_matches; ++i) out[i] = matches[i];
        kept = n_matches;
    }
    *n_out = kept;
    *pose = res;
    return AKZ_OK;
}

// what the pose forms of the seeded pairs calls refuse of their own, in front of the seeded call's refusals (the bank form too: akz_bank_api.cpp)
int pose_pairs_refusals(const char* name, const akz_ransac_options* options, const akz_camera* cameras, uint64_t n_sets, const akz_pose* poses) {
    AKZ_TRY(seeded_refuse_options(name, options));
    if (options->model_kind == AKZ_GUIDED_HOMOGRAPHY) return refuse(std::string(name) + "a pose needs a fundamental matrix (model_kind 1 or 3)");
    if (options->guided != 0) return refuse(std::string(name) + "the guided stage behind a pose is not there yet: guided must be 0");
    if (!cameras || !poses) return refuse(std::string(name) + "null cameras or poses");
    for (uint64_t s = 0; s < n_sets; ++s)
        if (!camera_ok(cameras[s])) return refuse(std::string(name) + "camera " + std::to_string(s) + " needs finite fields and fx, fy != 0");
    return AKZ_OK;
}

extern "C" int akz_match_features_seeded_pose_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const akz_camera* cameras,
                                                    const uint64_t* pairs, uint64_t n_pairs, uint64_t desc_bytes,
                                                    const akz_ransac_options* options, int cross_check, akz_match* out, uint64_t* n_out,
                                                    float* model, int* found, uint32_t* iterations, uint64_t* trials_run, akz_pose* poses,
                                                    float* points) {
    const char* name = "match_features_seeded_pose_pairs: ";
    AKZ_TRY(pose_pairs_refusals(name, options, cameras, n_sets, poses));
    const SeededPose pose{cameras, poses, points};
    return match_seeded_pairs_impl({name, c, sets, n_sets, pairs, n_pairs, desc_bytes, out, n_out, nullptr}, cross_check != 0, options, model, found,
                                   iterations, trials_run, &pose);
}
