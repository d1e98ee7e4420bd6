// Absolute pose by the seeded resection RANSAC (additions; include/akaze_hip.h).  akz_estimate_resection,
// akz_refine_resection and akz_resection_seeded_host are the statement of akz_resection.hpp run on the host -- one thread, in
// trial order, no GPU call, no context: the definition, not a fast path; their refit is refit_loop_host<ResectionRefit>, the loop of
// every model.  akz_resection_seeded_problems runs it over many problems on the GPU (akz_resection.hip: the same source on the
// device): one upload, the rounds by seeded_rounds_device (akz_match_seeded_api.cpp: the driver of every seeded call, which launches this
// model's round through launch::resection_round), one launch for filter and refit, one read-back.  The winner and the stopping rule
// are seeded_rounds<K> / seeded_need in the host statement and k_seeded_update on the device: the family's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "akz_ctx.hpp"
#include "akz_ransac_seeded.hpp"
#include "akz_resection.hpp"

namespace akz {
int seeded_refuse_options_of(const char* name, const akz_ransac_options* opt, bool resection);  // akz_ransac_seeded.cpp
}

namespace {

constexpr int MF = kResModelFloats;

int refuse(const std::string& what) {
    set_error(what);
    return AKZ_ERR_INVALID_ARG;
}

// one problem as the statement reads it (the host's view of ResectionRefit): X[i] .. v[i] out of the interleaved arrays
struct Strided {
    const float* p;
    int step;
    float operator[](uint64_t i) const { return p[step * i]; }
};
struct Problem {
    Strided X, Y, Z, u, v;
    uint64_t n;
    ResCamera cam;
};
Problem problem_of(const akz_resection_problem& q) {
    return Problem{{q.points, 3}, {q.points + 1, 3}, {q.points + 2, 3}, {q.pixels, 2}, {q.pixels + 1, 2}, q.n, res_camera(q.camera)};
}

// what every call refuses of a problem; `name` ends in ": ", `what` names the problem ("" or "problem 3: ")
int refuse_problem(const char* name, const std::string& what, const akz_resection_problem& q) {
    if (q.n >= (1ull << 32)) return refuse(std::string(name) + what + "n must be < 1 << 32");
    if (q.n && (!q.points || !q.pixels)) return refuse(std::string(name) + what + "null points or pixels");
    if (!camera_ok(q.camera)) return refuse(std::string(name) + what + "the camera needs finite fields and fx, fy != 0");
    return AKZ_OK;
}
bool epsilon_ok(float eps) { return eps > 0.0f && std::isfinite(eps); }
// the refusals that the host statement and the GPU call share: the options alone
int refuse_options(const char* name, const akz_ransac_options* opt) {
    AKZ_TRY(seeded_refuse_options_of(name, opt, true));
    if (opt->guided != 0) return refuse(std::string(name) + "there is no guided stage behind a resection: guided must be 0");
    if (opt->refine_iterations > 0 && !epsilon_ok(opt->epsilon_inliers))
        return refuse(std::string(name) + "with refine_iterations > 0, epsilon_inliers must be finite and > 0");
    return AKZ_OK;
}

void pose_out(const float (&m)[MF], bool found, akz_resection& out) {
    for (int k = 0; k < 9; ++k) out.r[k] = found ? m[k] : 0.0f;
    for (int k = 0; k < 3; ++k) out.t[k] = found ? m[9 + k] : 0.0f, out.sigma[k] = found ? m[12 + k] : 0.0f;
    out.found = found ? 1 : 0;
}

uint64_t write_kept(const std::vector<uint8_t>& member, uint32_t* kept) {
    uint64_t k = 0;
    for (size_t i = 0; i < member.size(); ++i)
        if (member[i]) kept[k++] = (uint32_t)i;
    return k;
}

// the statement for one checked problem
void seeded_statement(const Problem& q, const akz_ransac_options& opt, uint64_t stream, uint32_t* kept, uint64_t* n_kept, akz_resection* pose,
                      uint32_t* iterations, uint64_t* trials_run) {
    float best_model[MF] = {};
    int64_t best = 0;
    uint64_t run = 0, k = 0;
    uint32_t fits = 0;
    if (q.n >= (uint64_t)kResK) {
        float m[MF];  // the model of the trial at hand
        seeded_rounds<kResK>(
            q.n, opt.seed[0], opt.seed[1], stream, opt.max_trials, opt.confidence,
            [&](const uint64_t(&smp)[kResK]) -> int64_t {
                float X[kResK], Y[kResK], Z[kResK], u[kResK], v[kResK];
                for (int i = 0; i < kResK; ++i) X[i] = q.X[smp[i]], Y[i] = q.Y[smp[i]], Z[i] = q.Z[smp[i]], u[i] = q.u[smp[i]], v[i] = q.v[smp[i]];
                if (!resection_from_6(X, Y, Z, u, v, q.cam, AKZ_FUNDAMENTAL_REFIT_EPSILON, m)) return -1;
                int64_t inl = 0;
                for (uint64_t i = 0; i < q.n; ++i) inl += ResectionRefit::inlier(m, q, i, opt.epsilon_inliers) ? 1 : 0;
                return inl;
            },
            [&] { std::memcpy(best_model, m, sizeof(m)); }, best, run);
        if (best > 0) {
            std::vector<uint8_t> member((size_t)q.n);
            fits = refit_loop_host<ResectionRefit>(q, q.n, best_model, AKZ_FUNDAMENTAL_REFIT_EPSILON, opt.epsilon_inliers, opt.refine_iterations, member);  // (no iteration: the classification alone)
            k = write_kept(member, kept);
        }
    }
    *n_kept = k;
    pose_out(best_model, best > 0, *pose);
    if (iterations) *iterations = fits;
    if (trials_run) *trials_run = run;
}

}  // namespace

extern "C" {

int akz_estimate_resection(const float* points6, const float* pixels6, const akz_camera* camera, akz_resection* pose, int* found) {
    const char* name = "estimate_resection: ";
    if (!points6 || !pixels6 || !camera || !pose) return refuse(std::string(name) + "null points6, pixels6, camera or pose");
    if (!camera_ok(*camera)) return refuse(std::string(name) + "the camera needs finite fields and fx, fy != 0");
    float X[kResK], Y[kResK], Z[kResK], u[kResK], v[kResK], m[MF] = {};
    for (int i = 0; i < kResK; ++i) X[i] = points6[3 * i], Y[i] = points6[3 * i + 1], Z[i] = points6[3 * i + 2], u[i] = pixels6[2 * i], v[i] = pixels6[2 * i + 1];
    const bool ok = resection_from_6(X, Y, Z, u, v, res_camera(*camera), AKZ_FUNDAMENTAL_REFIT_EPSILON, m);
    pose_out(m, ok, *pose);
    if (found) *found = ok ? 1 : 0;
    return AKZ_OK;
}

int akz_refine_resection(const akz_resection_problem* problem, const akz_resection* pose_in, float epsilon, uint32_t max_iterations, uint32_t* kept,
                         uint64_t* n_kept, akz_resection* pose_out_, uint32_t* iterations) {
    const char* name = "refine_resection: ";
    if (!problem || !pose_in || !n_kept) return refuse(std::string(name) + "null problem, pose_in or n_kept");
    AKZ_TRY(refuse_problem(name, "", *problem));
    if (problem->n && !kept) return refuse(std::string(name) + "null kept");
    if (!epsilon_ok(epsilon)) return refuse(std::string(name) + "epsilon must be finite and > 0");
    const Problem q = problem_of(*problem);
    float h[MF];
    for (int k = 0; k < 9; ++k) h[k] = pose_in->r[k];
    for (int k = 0; k < 3; ++k) h[9 + k] = pose_in->t[k], h[12 + k] = pose_in->sigma[k];
    std::vector<uint8_t> member((size_t)q.n);
    const uint32_t done = refit_loop_host<ResectionRefit>(q, q.n, h, AKZ_FUNDAMENTAL_REFIT_EPSILON, epsilon, max_iterations, member);
    *n_kept = write_kept(member, kept);
    if (pose_out_) {
        if (done > 0) pose_out(h, true, *pose_out_);
        else *pose_out_ = *pose_in;
    }
    if (iterations) *iterations = done;
    return AKZ_OK;
}

int akz_resection_seeded_host(const akz_resection_problem* problem, const akz_ransac_options* options, uint64_t stream, uint32_t* kept,
                              uint64_t* n_kept, akz_resection* pose, uint32_t* iterations, uint64_t* trials_run) {
    const char* name = "resection_seeded_host: ";
    AKZ_TRY(refuse_options(name, options));
    if (!problem || !n_kept || !pose) return refuse(std::string(name) + "null problem, n_kept or pose");
    AKZ_TRY(refuse_problem(name, "", *problem));
    if (problem->n && !kept) return refuse(std::string(name) + "null kept");
    seeded_statement(problem_of(*problem), *options, stream, kept, n_kept, pose, iterations, trials_run);
    return AKZ_OK;
}

int akz_resection_seeded_problems(akz_ctx* c, const akz_resection_problem* problems, uint64_t n_problems, const akz_ransac_options* options,
                                  uint32_t* kept, uint64_t* n_kept, akz_resection* poses, uint32_t* iterations, uint64_t* trials_run) {
    const char* name = "resection_seeded_problems: ";
    if (!c) return refuse(std::string(name) + "null context");
    AKZ_TRY(refuse_options(name, options));
    if (n_problems >= (1ull << 28)) return refuse(std::string(name) + "n_problems must be < 1 << 28");  // (a round is 8 workgroups per problem in one launch)
    if (n_problems == 0) return AKZ_OK;
    if (!problems || !n_kept || !poses) return refuse(std::string(name) + "null problems, n_kept or poses");
    uint64_t total = 0;
    for (uint64_t p = 0; p < n_problems; ++p) {
        AKZ_TRY(refuse_problem(name, "problem " + std::to_string(p) + ": ", problems[p]));
        total += problems[p].n;
        if (total >= (1ull << 32)) return refuse(std::string(name) + "the problems of one call hold 1 << 32 correspondences or more together");
    }
    if (total && !kept) return refuse(std::string(name) + "null kept");
    const akz_ransac_options& opt = *options;
    const uint32_t max_trials = (uint32_t)opt.max_trials;
    uint64_t n_running = 0;
    for (uint64_t p = 0; p < n_problems; ++p) n_running += problems[p].n >= (uint64_t)kResK && max_trials > 0 ? 1 : 0;
    if (n_running == 0) {  // nothing to try anywhere: the statement's zeros, and no GPU work
        for (uint64_t p = 0; p < n_problems; ++p) {
            n_kept[p] = 0;
            std::memset(&poses[p], 0, sizeof(akz_resection));
            if (iterations) iterations[p] = 0;
            if (trials_run) trials_run[p] = 0;
        }
        return AKZ_OK;
    }
    AKZ_TRY(bind(c, true, false));
    hipStream_t st = c->stream;
    // the upload: problem table | done | need (one window of rounds per problem) | X | Y | Z | u | v
    const size_t np = (size_t)n_problems;
    const uint64_t stride = (total + 63) / 64 * 64;
    SeededState s(n_problems, MF, opt);
    const size_t b_job = up256(np * sizeof(launch::ResJobHost)), b_done = s.b_done, b_need = s.b_need;
    const size_t b_pl = up256((size_t)stride * 4 * 5), b_up = b_job + b_done + b_need + b_pl;
    const size_t b_state = s.bytes();  // the rounds' state, behind the upload
    // the read-back: kept counts | fits | trials | poses | kept indices
    const size_t b_w = up256(np * 4), b_pose = up256(np * sizeof(akz_resection)), b_down = 3 * b_w + b_pose + up256((size_t)total * 4);
    AKZ_TRY(ensure(c, c->rs_dev, b_up + b_state + b_down));
    AKZ_TRY(ensure_pinned(c, c->rs_pin, b_up + 256 + b_down));
    char *d = (char*)c->rs_dev.p, *h = (char*)c->rs_pin.p;
    launch::ResJobHost* h_job = (launch::ResJobHost*)h;
    s.tables(d + b_job, h + b_job, h + b_up);
    uint32_t* h_done = s.h_done;
    float* h_pl = (float*)(h + b_job + b_done + b_need);
    uint64_t off = 0;
    for (size_t p = 0; p < np; ++p) {
        const akz_resection_problem& q = problems[p];
        const ResCamera cam = res_camera(q.camera);
        h_job[p] = launch::ResJobHost{off, (uint32_t)q.n, 0u, cam.fx, cam.fy, cam.cx, cam.cy};
        h_done[p] = q.n >= (uint64_t)kResK && max_trials > 0 ? 0u : 1u;
        for (uint64_t i = 0; i < q.n; ++i) {
            h_pl[off + i] = q.points[3 * i];
            h_pl[stride + off + i] = q.points[3 * i + 1];
            h_pl[2 * stride + off + i] = q.points[3 * i + 2];
            h_pl[3 * stride + off + i] = q.pixels[2 * i];
            h_pl[4 * stride + off + i] = q.pixels[2 * i + 1];
        }
        off += q.n;
    }
    for (int k = 0; k < 5; ++k)  // (the padding goes up too)
        for (uint64_t i = total; i < stride; ++i) h_pl[k * stride + i] = 0.0f;
    const launch::ResJobHost* d_job = (const launch::ResJobHost*)d;
    const float* d_pl = (const float*)(d + b_job + b_done + b_need);
    s.place(d + b_up);
    char* d_down = d + b_up + b_state;
    uint32_t *d_nk = (uint32_t*)d_down, *d_fits = (uint32_t*)(d_down + b_w), *d_trials = (uint32_t*)(d_down + 2 * b_w);
    s.d_trials = d_trials;
    akz_resection* d_pose = (akz_resection*)(d_down + 3 * b_w);
    uint32_t* d_kept = (uint32_t*)(d_down + 3 * b_w + b_pose);
    const bool timed = c->rs_split_on;
    const uint64_t k1 = seeded_seed_key(opt.seed[0], opt.seed[1]);
    AKZ_TRY(seeded_rounds_device(
        st, s, kResK, n_running, [&](uint64_t p) { return problems[p].n; },
        [&]() -> int {
            if (timed) {
                for (Event& e : c->mp_split_ev) AKZ_TRY(e.ensure(hipEventDefault));
                AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[0], st));
            }
            AKZ_HIP_TRY(hipMemcpyAsync(d, h, b_up, hipMemcpyHostToDevice, st));
            AKZ_TRY(s.clear(st));
            AKZ_HIP_TRY(hipMemsetAsync(d_trials, 0, b_w, st));  // (a problem that never runs: 0 trials)
            if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[1], st));
            return AKZ_OK;
        },
        [&](uint32_t r) {
            launch::resection_round(st, d_job, (uint32_t)np, s.d_done, k1, opt.stream_base, r, max_trials, d_pl, stride,
                                    AKZ_FUNDAMENTAL_REFIT_EPSILON, opt.epsilon_inliers, s.d_rm, s.d_ri);
        }));
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[2], st));
    launch::resection_finish(st, d_job, (uint32_t)np, d_pl, stride, s.d_bm, s.d_bi, AKZ_FUNDAMENTAL_REFIT_EPSILON, opt.epsilon_inliers,
                             opt.refine_iterations, d_kept, d_nk, d_fits, d_pose);
    AKZ_HIP_TRY(hipGetLastError());
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[3], st));
    char* h_down = h + b_up + 256;
    AKZ_HIP_TRY(hipMemcpyAsync(h_down, d_down, 3 * b_w + b_pose + (size_t)total * 4, hipMemcpyDeviceToHost, st));
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[4], st));
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    if (timed)
        for (int i = 0; i < 4; ++i) {
            float ms = 0.0f;
            AKZ_HIP_TRY(hipEventElapsedTime(&ms, c->mp_split_ev[i], c->mp_split_ev[i + 1]));
            c->rs_split_ms[i] = ms;
        }
    const uint32_t *r_nk = (const uint32_t*)h_down, *r_fits = (const uint32_t*)(h_down + b_w), *r_trials = (const uint32_t*)(h_down + 2 * b_w);
    const akz_resection* r_pose = (const akz_resection*)(h_down + 3 * b_w);
    const uint32_t* r_kept = (const uint32_t*)(h_down + 3 * b_w + b_pose);
    for (size_t p = 0; p < np; ++p) {
        n_kept[p] = r_nk[p];
        poses[p] = r_pose[p];
        if (iterations) iterations[p] = r_fits[p];
        if (trials_run) trials_run[p] = r_trials[p];
        if (r_nk[p]) std::memcpy(kept + h_job[p].off, r_kept + h_job[p].off, (size_t)r_nk[p] * 4);
    }
    return AKZ_OK;
}

int akz_debug_resection_split(akz_ctx* c, int enable, double* ms) {  // include/akaze_hip_debug.h
    if (!c) return refuse("null context");
    c->rs_split_on = enable != 0;
    if (ms)
        for (int k = 0; k < 4; ++k) ms[k] = c->rs_split_ms[k];
    return AKZ_OK;
}

}  // extern "C"
