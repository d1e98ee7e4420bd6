// Internal declarations shared by the host-side translation units of libakaze_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/akaze_hip.h"
#include "../../include/akaze_hip_debug.h"

namespace akz {

void set_error(const std::string& msg);
// host cores this process can count on: affinity mask, cgroup CPU quota, ranks per host (akz_api.cpp)
unsigned host_cpu_share();

// remove_outliers (estimate_fundamental_matrix.rs:99-165) with the trials optionally run by the caller's hook (akz_ransac.cpp;
// match_features hands in the device kernel of akz_ransac_kernels.hip): (x0, y0, x1, y1 of every match, n, 8 sample indices per
// trial, trials, epsilon_model, epsilon_inlier) -> 9 model floats and the inlier count (-1: no model) per trial
using TrialsOnDevice = std::function<int(const float*, const float*, const float*, const float*, uint32_t, const uint32_t*, uint32_t,
                                         float, float, float*, int32_t*)>;
int remove_outliers_impl(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                         const akz_match* matches, uint64_t n_matches, uint64_t num_trials, float epsilon_model,
                         float epsilon_inlier, akz_match* out, uint64_t* n_out, const TrialsOnDevice& trials_on_device);

#define AKZ_HIP_TRY(expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            ::akz::set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e));            \
            return AKZ_ERR_HIP;                                                                    \
        }                                                                                          \
    } while (0)

// The `random` crate's default source (Xorshift128+), one per thread, seeded [42, 69] (akz_ransac.cpp)
struct DefaultSource {
    uint64_t s0 = 42, s1 = 69;
    uint64_t next() {
        uint64_t x = s0;
        const uint64_t y = s1;
        s0 = y;
        x ^= x << 23;
        x ^= x >> 17;
        x ^= y ^ (y >> 26);
        s1 = x;
        return x + y;
    }
};
DefaultSource& default_source();
// the samples of `trials` RANSAC trials over n_matches >= K matches: K ascending indices per trial into out (akz_ransac.cpp;
// K = 8 or 4, T = uint64_t or uint32_t)
template <int K, class T>
void draw_samples(DefaultSource& src, uint64_t n_matches, uint64_t trials, T* out);

// the refusals every call over a list of matches shares (akz_ransac.cpp); `name` is the call's
int refuse_bad_matches(const char* name, const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                       const akz_match* matches, uint64_t n_matches, const akz_match* out, const uint64_t* n_out);
// The matched point pairs side by side, x0 | y0 | x1 | y1 with n_matches floats each: the inlier count of a trial -- 8 M
// evaluations for the 8 000 matches of a 4K pair at 1 000 trials -- is then a streaming loop the compiler vectorises instead
// of two gathers of 32-byte keypoints per evaluation.
struct MatchPoints {
    std::vector<float> v;
    const float *x0, *y0, *x1, *y1;
    MatchPoints(const akz_keypoint* keypoints_0, const akz_keypoint* keypoints_1, const akz_match* matches, uint64_t n) : v((size_t)n * 4) {
        float* p = v.data();
        x0 = p; y0 = p + n; x1 = p + 2 * n; y1 = p + 3 * n;
        for (uint64_t i = 0; i < n; ++i) {
            p[i] = keypoints_0[matches[i].index_0].x; p[n + i] = keypoints_0[matches[i].index_0].y;
            p[2 * n + i] = keypoints_1[matches[i].index_1].x; p[3 * n + i] = keypoints_1[matches[i].index_1].y;
        }
    }
};


#define AKZ_TRY(expr)            \
    do {                         \
        int _s = (expr);         \
        if (_s != AKZ_OK) return _s; \
    } while (0)

// one query set against sets that lie anywhere in one block of 64-byte rows (set k: rows set_first[k] .. + set_rows[k]);
// with d_n_cols also the opposite direction of every block (akz_descriptor_match_sets_mutual_device) -- akz_api.cpp
int match_sets_at(akz_ctx* c, const uint8_t* d_q, uint64_t n0, const uint8_t* d_rows, const uint64_t* set_first,
                  const uint64_t* set_rows, uint64_t n_sets, uint64_t distance_threshold, double lowes_ratio, akz_match* d_out,
                  uint64_t* d_n_out, akz_match* d_out_cols, uint64_t* d_n_cols, int side = 0);
// side 1 of match_sets_at enqueues on this stream with its own scratch (nullptr: the matcher mode has one side only); the
// caller orders it after its inputs and joins it before its outputs are read
hipStream_t match_side_stream(akz_ctx* c);

// streams of another component that run beside a context's: each slot ends up on a hardware queue and a pipe that the
// context's caller, coarse and finish streams do not use (a colliding stream is destroyed and replaced) -- akz_api.cpp
int place_streams_beside(akz_ctx* c, hipStream_t* slots, int n_slots, int* still_shared);
// what the stream-placement probe concludes from its timings (akz_api.cpp; akz_debug_placement_verdict for the tests):
// spin_pair_ms = two spins of spin_ms on two streams, first start to second end; tiny_pair_ms = 24 + 24 interleaved tiny
// kernels on two streams (negative: not measured); tiny_alone_ms = 24 of them on one stream
enum { kPlaceQueue = 1, kPlacePipe = 2, kPlaceAmbiguous = 4 };
int placement_verdict(float spin_pair_ms, float tiny_pair_ms, float tiny_alone_ms, float spin_ms);

// ---- host-side planning (akz_plan.cpp) ---------------------------------------------------
struct LevelPlan {
    double etime = 0, esigma = 0;
    uint32_t octave = 0, sublevel = 0, sigma_size = 0;  // EvolutionStep scalars
    uint32_t w = 0, h = 0;                               // plane size of the level
    uint32_t det_sigma = 0;                              // round(esigma*derivative_factor/2^octave)
    std::vector<double> tau;                             // fed_tau_steps
};
int config_validate(const akz_config& c);
int fed_tau_by_process_time(double T, int M, double tau_max, bool reordering, std::vector<double>& tau);
std::vector<float> gaussian_kernel(float sigma, size_t kernel_size);
size_t gaussian_kernel_size(float sigma);
void scharr_kernels(uint32_t scale, std::vector<float>& main_axis, std::vector<float>& off_axis);
int build_plan(uint32_t w, uint32_t h, const akz_config& cfg, std::vector<LevelPlan>& plan);

// A separable-filter pass as a sparse tap list: out = sum_i wgt[i] * in(.. + off[i]) evaluated
// left to right starting from 0.0f.  Dense Gaussian: 2hw+1 taps; Scharr: taps at -s, 0, +s.
constexpr int kMaxTaps = 13;
struct Taps {
    int n = 0;
    int hw = 0;  // half width of the full kernel (border clamp distance)
    int off[kMaxTaps] = {0};
    float wgt[kMaxTaps] = {0};
};
int taps_from_dense(const float* k, uint32_t ntaps, Taps& t);
Taps taps_scharr_main(uint32_t scale);
Taps taps_scharr_off(uint32_t scale);

// ---- device kernels' launch wrappers (akz_kernels.hip) -----------------------------------
struct Candidate {  // one NMS survivor (scale_space_extrema.rs:32-42 + bounds :80-87)
    uint32_t level;
    uint32_t idx;  // flat index w*y + x in the level
    float v, xp, xm, yp, ym;
    uint32_t img;  // image of the batch
};
struct KpParam {  // per-keypoint input of the orientation / descriptor kernels
    float xf, yf;     // point / ratio
    float scale;      // round(0.5*size/ratio)
    uint32_t level;
    uint32_t img;     // image of the batch
    uint32_t _pad[3];
};
struct OrientOut {
    float sum_x, sum_y;
    uint32_t found;
    uint32_t angle_bits;  // the angle as f32 bits where the device formed it (k_mldb with DeviceAngles); unused otherwise
};
struct MatchRec {  // per query descriptor
    uint32_t min_d, second_d, min_j, _pad;
};
struct LevelPtrs {  // device addresses of the planes one kernel needs, image 0 of the batch
    const float* lt;
    const float* lx;
    const float* ly;
    uint32_t w, h;
    uint64_t stride;  // elements between consecutive images
};
constexpr int kMaxLevels = 64;
constexpr int kRel1 = 12, kRel2 = 6;  // neighbour lists of the keypoint selection (akz_sort.hip, k_relations): 36-byte rows (four next-level places overflowed on enough candidates of a 4K frame for k_select's second pass to spend half its time scanning for them).  Six earlier neighbours overflowed on a third of a 4K frame's fine-level candidates -- the host then scans the partner levels itself -- : host selection 0.79 -> 0.45 ms per 4K frame with twelve (nine suffice; sixteen give nothing more)
struct LevelTable {
    LevelPtrs lv[kMaxLevels];
};

namespace launch {
void filter_h_f32(hipStream_t s, const float* in, float* out, uint32_t w, uint32_t h, uint32_t n, const Taps& t);
void filter_h_u8(hipStream_t s, const uint8_t* in, float* out, uint32_t w, uint32_t h, uint32_t n, const Taps& t);
void filter_v_f32(hipStream_t s, const float* in, float* out, uint32_t w, uint32_t h, uint32_t n, const Taps& t);
void delay(hipStream_t s, uint32_t microseconds);  // one wave spinning on the 100 MHz counter (stream-placement probe)
void half_size(hipStream_t s, const float* in, float* out, uint32_t w, uint32_t h, uint32_t n);
void pm_g2(hipStream_t s, const float* lx, const float* ly, float* out, uint32_t w, uint32_t h, uint32_t n,
           const double* d_k, uint32_t k_scale_pow);
void flow(hipStream_t s, const float* lsmooth, float* lflow, uint32_t w, uint32_t h, uint32_t n, const double* d_k,
          uint32_t k_scale_pow);
void fed_step(hipStream_t s, const float* lt_in, const float* lflow, float* lt_out, float* lstep, uint32_t w,
              uint32_t h, uint32_t n, float half_tau);
// n_steps <= 16 explicit steps in one launch of k_fed_own (LDS tile + register ownership, temporally fused)
// next != NULL: the launch also writes the NEXT level's Lsmooth and Lflow from this level's final Lt (k_fed_own's epilogue;
// only where fed_epilogue_supported says so)
struct FedNextPrep {
    float* lsmooth;
    float* lflow;
    const float* g3;     // gaussian_kernel(1.0, 3)
    const double* d_k;
    uint32_t k_pow;
};
bool fed_epilogue_supported(uint32_t w, uint32_t h, uint32_t n_steps);
void fed_fused(hipStream_t s, const float* lt_in, const float* lflow, float* lt_out, float* lstep, uint32_t w, uint32_t h,
               uint32_t n, const float* half_taus, uint32_t n_steps, const FedNextPrep* next = nullptr);
// workgroups of a 9..16-step launch (64 x 10 tiles)
uint64_t fed_deep_workgroups(uint32_t w, uint32_t h, uint32_t n);
void contrast_max(hipStream_t s, const float* blurred, uint32_t w, uint32_t h, uint32_t n,
                  unsigned long long* d_hmax_bits);
void contrast_hist(hipStream_t s, const float* blurred, uint32_t w, uint32_t h, uint32_t n,
                   const unsigned long long* d_hmax_bits, uint32_t nbins, uint32_t* d_hist);
void contrast_final(hipStream_t s, const unsigned long long* d_hmax_bits, const uint32_t* d_hist, uint32_t nbins,
                    double percentile, uint32_t n, double* d_k);
// ---- fused LDS stencil chains (akz_stencil.hip) ----
bool blur_fused_supported(uint32_t ntaps);
void blur_fused_f32(hipStream_t s, const float* in, float* out, uint32_t w, uint32_t h, uint32_t n, const float* k,
                    uint32_t ntaps);
void blur_fused_u8(hipStream_t s, const uint8_t* in, float* out, uint32_t w, uint32_t h, uint32_t n, const float* k,
                   uint32_t ntaps);
// prev: the previous level's final Lt (pw x ph).  half: this level starts a new octave; then the 2x2
// mean is written to lt_out as well.  g3: the 3 Gaussian taps of sigma 1.
void prep_fused(hipStream_t s, const float* prev, bool half, float* lt_out, float* lsmooth, float* lflow, uint32_t w,
                uint32_t h, uint32_t pw, uint32_t ph, uint32_t n, const float* g3, const double* d_k, uint32_t k_pow);
bool detector_fused_supported(uint32_t sigma);
void detector_fused(hipStream_t s, const float* lsmooth, uint32_t sigma, float* lx, float* ly, float* lxx, float* lyy,
                    float* lxy, float* ldet_out, uint32_t w, uint32_t h, uint32_t n);
// first + second derivatives, Ldet and the extrema candidates of one level in two launches
bool detector_tiled_fused_supported(uint32_t sigma);
// the same kernel over a set of levels that share sigma_size (one launch for several small levels)
struct DetLevelDesc {
    const float* lsmooth;
    float *lx, *ly, *lxx, *lyy, *lxy, *ldet;
    uint32_t w, h, level;
    float border_m;
};
uint32_t detector_tiled_set_max();
void detector_tiled_set(hipStream_t s, uint32_t sigma, const DetLevelDesc* levels, uint32_t nlevels, uint32_t n, float thr,
                        Candidate* d_cand, uint32_t cap, uint32_t* d_count);
void detector_tiled_fused(hipStream_t s, const float* lsmooth, uint32_t sigma, float* lx, float* ly, float* lxx,
                          float* lyy, float* lxy, float* ldet_out, uint32_t w, uint32_t h, uint32_t n, uint32_t level,
                          float thr, float border_m, Candidate* d_cand, uint32_t cap, uint32_t* d_count);
// streaming 5-tap gaussian_blur (akz_stream.hip)
bool blur5_stream_supported(uint32_t w, uint32_t h, uint32_t ntaps, bool is_u8);
void blur5_stream_u8(hipStream_t s, const uint8_t* in, float* out, uint32_t w, uint32_t h, uint32_t n, const float* k);
void blur5_stream_f32(hipStream_t s, const float* in, float* out, uint32_t w, uint32_t h, uint32_t n, const float* k);
// streaming contrast-factor passes (akz_stream.hip): max and histogram of the gradient of blur(in) in two launches
uint32_t march_band_rows(int kind, uint32_t w, uint32_t h, uint32_t n, int S, int32_t* cs_ce, uint32_t cap);  // test hook
bool blur5_march_supported(uint32_t w, uint32_t h, uint32_t ntaps);  // akz_march.hip: the same blur as a column march
void blur5_march_u8(hipStream_t s, const uint8_t* in, float* out, uint32_t w, uint32_t h, uint32_t n, const float* k);
void blur5_march_f32(hipStream_t s, const float* in, float* out, uint32_t w, uint32_t h, uint32_t n, const float* k);
// the same two passes as column marches (akz_march.hip: two columns per thread, bound by the plane read, not by arithmetic)
bool contrast_march_supported(uint32_t w, uint32_t h, uint32_t ntaps, uint32_t nbins);
void contrast_march(hipStream_t s, const float* in, uint32_t w, uint32_t h, uint32_t n, const float* g3,
                    unsigned long long* d_hmax_bits, uint32_t nbins, uint32_t* d_hist, double* d_thr);
void contrast_thresholds(hipStream_t s, const unsigned long long* d_hmax_bits, uint32_t nbins, uint32_t n, double* d_thr);
bool contrast_stream_supported(uint32_t w, uint32_t h, uint32_t ntaps, uint32_t nbins);
void contrast_stream(hipStream_t s, const float* in, uint32_t w, uint32_t h, uint32_t n, const float* g3,
                     unsigned long long* d_hmax_bits, uint32_t nbins, uint32_t* d_hist, double* d_thr);
// streaming form of prep_fused (akz_stream.hip)
bool prep_stream_supported(uint32_t w, uint32_t h);
void prep_stream(hipStream_t s, const float* prev, bool half, float* lt_out, float* lsmooth, float* lflow, uint32_t w,
                 uint32_t h, uint32_t pw, uint32_t ph, uint32_t n, const float* g3, const double* d_k, uint32_t k_pow);
// one-pass column march (akz_march.hip): 256-thread workgroups own 512-column strips, two columns per thread
bool detector_march_supported(uint32_t sigma, uint32_t w, uint32_t h, float border_m, bool nms);
void detector_march(hipStream_t s, const float* lsmooth, uint32_t sigma, float* lx, float* ly, float* lxx, float* lyy,
                    float* lxy, float* ldet_out, uint32_t w, uint32_t h, uint32_t n, uint32_t level, float thr,
                    float border_m, Candidate* d_cand, uint32_t cap, uint32_t* d_count);
// the same kernel over a set of levels that share sigma_size, the width's parity and the kept planes: one launch whose cells
// are shared among the levels in proportion to their strip-rows (largest level first)
uint32_t detector_march_set_max();
void detector_march_set(hipStream_t s, uint32_t sigma, const DetLevelDesc* levels, uint32_t nlevels, uint32_t n, float thr,
                        Candidate* d_cand, uint32_t cap, uint32_t* d_count);
void detector_set_waves(int waves);  // measurement hook (process-wide): 0 = kDetSetWaves
uint32_t detector_set_cells(int S, const uint32_t* w, const uint32_t* h, uint32_t nlv, uint32_t n, int32_t* cells, uint32_t cap,
                            int32_t* grids);  // test hook
// level preparation + the first n_steps <= 4 diffusion steps of a level in one launch (akz_march.hip, k_level_march)
bool head_fused_supported(uint32_t w, uint32_t h, uint32_t ntaps0, uint32_t ntaps1);
// (d_zero_word: a 32-bit word the kernel clears -- the job's candidate counter -- or NULL)
void head_fused_u8(hipStream_t s, const uint8_t* in, float* lt0, float* blurred, float* gx, float* gy, uint32_t w, uint32_t h, uint32_t n,
                   const float* k5, const float* g3, unsigned long long* d_smax_bits, uint32_t* d_zero_word = nullptr);
void head_fused_f32(hipStream_t s, const float* in, float* lt0, float* blurred, float* gx, float* gy, uint32_t w, uint32_t h, uint32_t n,
                    const float* k5, const float* g3, unsigned long long* d_smax_bits, uint32_t* d_zero_word = nullptr);
// the histogram + percentile pass over the stored Scharr pair (gx, gy: k_head's), and Lflow = pm_g2 of the same pair
void contrast_hist_final(hipStream_t s, const float* gx, const float* gy, uint32_t w, uint32_t h, uint32_t n, unsigned long long* d_smax_bits,
                         uint32_t nbins, uint32_t* d_hist, uint32_t* d_done, double percentile, double* d_k);
void flow_from_pair(hipStream_t s, const float* gx, const float* gy, float* lflow, uint32_t w, uint32_t h, uint32_t n, const double* d_k,
                    uint32_t k_pow);
void march_min_band_rows(int detector, int level);  // measurement hook (process-wide): 0 = the planners' own rules
bool level_march_supported(uint32_t w, uint32_t h);
// pw, ph != 0: `prev` is the previous octave's last Lt (pw x ph) and the level starts from its 2x2 mean, formed inside the
// kernel (level_march_half_supported)
bool level_march_half_supported(uint32_t w, uint32_t h, uint32_t pw, uint32_t ph, uint32_t n_steps);
void level_march(hipStream_t s, const float* prev, float* lsmooth, float* lflow, float* lt_out, float* lstep, uint32_t w,
                 uint32_t h, uint32_t n, const float* g3, const double* d_k, uint32_t k_pow, const float* half_taus,
                 uint32_t n_steps, uint32_t pw = 0, uint32_t ph = 0);
// the remaining levels of the pyramid, from the first one whose image fits a compute unit, in ONE launch with one
// workgroup per image (akz_resident.hip, k_octave_resident): preparation and every diffusion step of every level
struct ResidentLevel {
    float *lt, *lsmooth, *lflow, *lstep;  // image 0 of the batch; lstep may be null
    uint32_t w, h;
    bool half;              // the level opens an octave (2x2 mean of the previous level's final Lt)
    uint32_t n_tau;         // >= 1
    const float* half_tau;  // 0.5f * (tau as f32) per step
    uint32_t k_pow;         // octave
};
constexpr int kResidentMaxLevels = 10;
constexpr int kResidentMaxSteps = 448;
bool octave_resident_supported(uint32_t w, uint32_t h);
void octave_resident(hipStream_t s, const float* prev, uint32_t pw, uint32_t ph, uint32_t n, const ResidentLevel* levels,
                     uint32_t n_levels, const float* g3, const double* d_k);
bool detector_nms_fused_supported(uint32_t sigma);
void detector_nms_fused(hipStream_t s, const float* lsmooth, uint32_t sigma, float* lx, float* ly, float* lxx,
                        float* lyy, float* lxy, float* ldet_out, uint32_t w, uint32_t h, uint32_t n, uint32_t level,
                        float thr, float border_m, Candidate* d_cand, uint32_t cap, uint32_t* d_count);
void rcp_f64_to_f32(hipStream_t s, const double* x, float* out, uint64_t n);  // test hook (akz_pm_g2.hpp)
void accumulate(hipStream_t s, float* a, const float* b, uint64_t count);  // a += b (image.rs:218-231); a may equal b
void ldet(hipStream_t s, const float* lxx, const float* lyy, const float* lxy, float* out, uint64_t count,
          float sigma_quat);
// the candidate list into scan order on the device (akz_sort.hip): by image, level, flat pixel index.  false: the
// batch needs more key bits than the sort takes (the host then sorts)
size_t sort_candidates_scratch(uint32_t cap, uint64_t max_px, uint32_t n_levels, uint32_t n_images);
uint32_t sort_small_capacity();  // one image's list up to this capacity is sorted by one launch of one workgroup:
// false: not this list (too long, too many rows) -- the caller takes sort_candidates_device
// Lists of any length, several images, up to 65 536 (image, level, row) buckets: the same counting sort in four launches
// (scratch: sort_candidates_buckets_scratch(cap) bytes, the first sort_candidates_buckets_counters() of them its counters;
// *counters_zero: the context's claim -- how many bytes of `scratch` are known to be zero.  The sort clears the counters unless the
// claim covers them, drops the claim before its first launch and raises it to the counters' size behind its last).  false: too
// many buckets -- nothing was enqueued, the claim is as it was, the caller takes sort_candidates_device.  rel_scratch as for
// sort_candidates_rows.
size_t sort_candidates_buckets_scratch(uint32_t cap);
size_t sort_candidates_buckets_counters();
bool sort_candidates_buckets(hipStream_t s, const Candidate* d_cand, uint32_t cap, const uint32_t* d_count, const uint32_t* level_w,
                             const uint32_t* level_h, uint32_t n_levels, uint32_t n_images, void* scratch, size_t* counters_zero,
                             Candidate* d_sorted, uint32_t* d_zero, void* rel_scratch);
// rel_scratch (candidate_relations_bytes for ONE image, or null): the sort leaves candidate_relations' level / row tables there
// (its bucket starts are those tables) -- pass tables_ready to candidate_relations
bool sort_candidates_rows(hipStream_t s, const Candidate* d_cand, uint32_t cap, const uint32_t* d_count, const uint32_t* level_w,
                          const uint32_t* level_h, uint32_t n_levels, Candidate* d_sorted, uint32_t* d_zero, void* rel_scratch);
bool sort_candidates_device(hipStream_t s, const Candidate* d_cand, uint32_t cap, const uint32_t* d_count, uint64_t max_px,
                            uint32_t n_levels, uint32_t n_images, void* scratch, Candidate* d_sorted, uint32_t* d_zero = nullptr);
// who can be within `size` of whom (akz_sort.hip, k_relations): per candidate of the SORTED list kRel1 indices of earlier
// candidates of its own / the previous level and kRel2 of the next level, relative to its image's first candidate
size_t candidate_relations_bytes(uint32_t cap, const uint32_t* level_h, uint32_t n_levels, uint32_t n_images);
void candidate_relations(hipStream_t s, const Candidate* d_sorted, uint32_t cap, const uint32_t* d_count, const float* size, const float* ratio,
                         const uint32_t* level_w, const uint32_t* level_h, uint32_t n_levels, uint32_t n_images, void* scratch,
                         uint16_t** d_rel_out, uint32_t** d_flags_out, void* sel_scratch = nullptr, bool tables_ready = false);
// The selection itself on the device (akz_sort.hip: k_sel_prepare, k_select, k_sel_pack; akz_select.hpp): dependency rounds
// over the neighbour lists, one workgroup per image.  sel_scratch (select_device_bytes) must have been handed to
// sort_candidates_device (d_zero = select_device_revcnt(...)) and to candidate_relations of the same list.  Leaves, in image
// order, the selected keypoints (d_recs: 32-byte records -- x, y, response, level, then room for the keypoint's OrientOut,
// which orientation_counted(..., out_stride 2) fills in: one copy brings both to the host) and the parameters of the keypoint
// kernels (d_pars), room for `cap` of each; *d_hdr_out: per image 16 words {keypoints, extrema, status, looks, four phase
// times, the list's length, the image's flags, its contrast factor (2 words), 4 unused} -- status != 0: the image is for the
// host's selection (an overflowed list, too many candidates) and the whole job should take that path --; *d_total_out: the
// keypoint count of the job
size_t select_device_bytes(uint32_t cap, uint32_t n_images);
uint32_t* select_device_revcnt(void* sel_scratch, uint32_t cap, uint32_t n_images);
void select_device(hipStream_t s, const Candidate* d_sorted, uint32_t cap, const uint32_t* d_count, const float* size, const float* ratio,
                   const uint32_t* level_w, const uint32_t* level_h, uint32_t n_levels, uint32_t n_images, const void* rel_scratch,
                   void* sel_scratch, const double* d_k, void* d_recs, KpParam* d_pars, uint32_t** d_hdr_out, uint32_t** d_total_out);
// candidates of all images are appended to ONE list (d_count is a single counter, cap the list capacity)
void nms(hipStream_t s, const float* ldet, uint32_t w, uint32_t h, uint32_t n, uint64_t img_stride, uint32_t level,
         float thr, float border_m, Candidate* d_cand, uint32_t cap, uint32_t* d_count);
// The detection mask (akz_mask.hip): d_out = the records of d_in whose mask byte is nonzero, in any order.  d_cnt: four words, 8-byte aligned --
// [0] the list's length on entry, the kept count on return (untouched if it exceeds cap: the first cap records are then copied
// through), [1] the length on entry, [2], [3] the kernel's own (cleared here, in front of the launch).  row_pitch, frame_stride:
// bytes of the mask; frame_stride 0 = one mask for all images.  d_out holds cap records and is not d_in.
void mask_candidates(hipStream_t s, const Candidate* d_in, Candidate* d_out, uint32_t cap, uint32_t* d_cnt, const uint8_t* d_mask,
                     uint64_t row_pitch, uint64_t frame_stride, const uint32_t* level_w, const uint32_t* level_h,
                     const uint32_t* level_octave, uint32_t n_levels, uint32_t n_images);
void orientation(hipStream_t s, const LevelTable& lt, const KpParam* d_kp, uint32_t nkp,
                 unsigned long long window_mask, uint32_t n_windows, OrientOut* d_out);
// the same with the keypoint count still on the device (*d_nkp <= max_kp: the grid is sized for max_kp)
void orientation_counted(hipStream_t s, const LevelTable& lt, const KpParam* d_kp, const uint32_t* d_nkp, uint32_t max_kp,
                         unsigned long long window_mask, uint32_t n_windows, OrientOut* d_out, uint32_t out_stride);
// d_cosi: (cosf(angle), sinf(angle)) per keypoint from the host libm (descriptors.rs:55-56)
void mldb(hipStream_t s, const LevelTable& lt, const KpParam* d_kp, const float* d_cosi, uint32_t nkp,
          uint32_t channels, uint8_t* d_desc64);
// the same with the keypoint count still on the device and the angle, cosf, sinf of every keypoint formed ON the device from
// its orientation sums (akz_libm.hpp; d_sums[i * sums_stride]): the angle is left in d_sums[..].angle_bits, *d_flag is raised
// if an argument is outside what the device forms cover
// (keypoints [first, min(last, *d_nkp)): the grid covers first .. last; first is rounded down to the kernel's group of four)
// `mirror`: the kernel also stores every keypoint's 32-byte record and descriptor row, and the selection's headers, into the
// host's (pinned, device-visible) buffers -- the waited-for job's results without copies behind the kernel
struct MldbMirror {
    void* host_recs;        // 32 bytes per keypoint
    const void* d_hdr;      // the selection's headers on the device, hdr_bytes (a multiple of 16) ...
    void* host_hdr;         // ... and where the host wants them
    uint32_t hdr_bytes;
    uint8_t* host_desc;     // 64 bytes per keypoint, or NULL
};
void mldb_counted(hipStream_t s, const LevelTable& lt, const KpParam* d_kp, const uint32_t* d_nkp, uint32_t first, uint32_t last, OrientOut* d_sums,
                  uint32_t sums_stride, bool libm_fma, uint32_t* d_flag, uint32_t channels, uint8_t* d_desc64, const MldbMirror* mirror = nullptr);
void libm_eval(hipStream_t s, const float* a, const float* b, float* out3, uint64_t n, bool fma, uint32_t* d_flag);
// the popcount scan and the kernels that turn chunk records into lists (akz_kernels.hip; the rule: akz_match_rule.hpp)
uint32_t match_num_chunks(uint32_t n0, uint32_t n1);
// Both scans write one record per (chunk of the train set, query): d_rec[chunk * n0 + query]; match_compact merges a
// query's chunk records (ascending rows: the lowest row wins among equal minima) and applies the ratio test.
// rows_le_61: rows are M-LDB descriptors (at most 61 bytes): bytes 61..63 are padding and not compared
void match(hipStream_t s, const uint8_t* d0, uint32_t n0, const uint8_t* d1, uint32_t n1, uint32_t threshold,
           bool rows_le_61, uint32_t chunks, MatchRec* d_rec);
// the same scan on the matrix cores (akz_match.hip): descriptor bits unpacked to int8, distances from one integer
// GEMM; identical records.  Rows of the unpacked images are padded (match_mfma_rows).
uint32_t match_mfma_rows(uint32_t n, bool queries);
uint32_t match_mfma_chunks(uint32_t n0, uint32_t n1, uint32_t forced = 0);
uint32_t match_mfma_multi_chunks(uint32_t n0, uint32_t n_sets, uint32_t avg_tiles, uint32_t forced = 0);  // chunks per set of a multi-set launch
// bound (queries only): n_bound arrays of n_pad per-query pruning bounds, set to threshold; d_tiles (train images of
// several sets): per LDS tile {first source row, valid rows}
void unpack_bits(hipStream_t s, const uint8_t* d, uint32_t n, uint32_t n_pad, bool query, uint8_t* out8, uint32_t* pop,
                 uint32_t* bound, uint32_t threshold, uint32_t n_bound, const uint32_t* d_tiles, bool fp4 = false);
// both sets of a pair call in one launch (query form with one bound array, train form)
// one workgroup per RANSAC trial: model of its eight samples (akz_fmatrix.hpp) + inlier count over all matches
// (akz_ransac_kernels.hip)
void ransac_trials(hipStream_t s, const float* d_pts, uint32_t n_matches, const uint32_t* d_samples, uint32_t trials, float epsilon_model,
                   float epsilon_inlier, float* d_models, int32_t* d_inliers);
// The pairs calls of both models (akz_ransac_kernels.hip).  Per pair p: its matches at d_raw + raw_off, their count at
// d_raw_cnt[cnt_idx]; its x0 | y0 | x1 | y1 at d_pts + {0, 1, 2, 3} * pts_stride + raw_off; its trials at trial_off .. + n_trials
// of the call
struct PairJobHost {
    uint64_t raw_off, kp0_off, kp1_off, trial_off, keep_off, n_trials;
    uint32_t cnt_idx, pad;
};
static_assert(sizeof(PairJobHost) == 56, "the device reads 56-byte pair records");
// 8 / 4 / 8 matches per sample (FundamentalRansac, HomographyRansac, FundamentalNormalisedRansac: the seeded calls only --
// seeded_round, pairs_pick_filter over the best slots, model_refit)
enum class RansacModel { Fundamental, Homography, FundamentalNormalised };
// gathers the keypoint coordinates of every pair's matches (kx / ky: x / y of every uploaded set's keypoints)
void pair_points(hipStream_t s, const PairJobHost* d_pairs, uint32_t n_pairs, const void* d_raw, const uint64_t* d_raw_cnt,
                 const float* d_kx, const float* d_ky, float* d_pts, uint64_t pts_stride);
// trials first_trial .. + n_trials of the call: d_trials holds this chunk's K sample indices per trial (relative to the
// pair's first match), then the pair of every trial; models / inliers are indexed by the call's trial number
void pairs_trials(hipStream_t s, RansacModel model, const PairJobHost* d_pairs, const uint32_t* d_trials, uint64_t first_trial,
                  uint32_t n_trials, const uint64_t* d_raw_cnt, const float* d_pts, uint64_t pts_stride, float epsilon_model,
                  float epsilon_inlier, float* d_models, int32_t* d_inliers);
// per pair: the first trial with the most inliers (strict `>` from 0 in trial order), then the matches it keeps, compacted in
// order at d_keep + keep_off, their count at d_keep_cnt[pair] (fewer than K matches: all of them).  No trial above 0 -- the
// fundamental matrix: the zero model filters; the homography: every match kept.  A call that hands the model back also gets the
// winner's model at d_h + 9 pair (none: zeros) and found at d_found[pair]; both are null for akz_match_features_pairs.
void pairs_pick_filter(hipStream_t s, RansacModel model, const PairJobHost* d_pairs, uint32_t n_pairs, const void* d_raw,
                       const uint64_t* d_raw_cnt, const float* d_pts, uint64_t pts_stride, const float* d_models, const int32_t* d_inliers,
                       float epsilon_inlier, void* d_keep, uint64_t* d_keep_cnt, float* d_h, int32_t* d_found);
// the refit stage after pairs_pick_filter (akz_homography_refit.hip), for a model that was handed back: per pair with found = 1
// and 4 (the fundamental matrix: 8) matches or more, the loop of akz_homography_refit.hpp (akz_fundamental_refit.hpp) on the raw
// list from the model at d_h + 9 pair; after an accepted fit the model, the kept list and its count are rewritten;
// d_iterations[pair] = accepted fits (0 for the pairs left alone).  epsilon_model: that of the model's rank rule
void model_refit(hipStream_t s, RansacModel model, const PairJobHost* d_pairs, uint32_t n_pairs, const void* d_raw, const uint64_t* d_raw_cnt,
                      const float* d_pts, uint64_t pts_stride, float epsilon_model, float epsilon_inlier, uint32_t max_iterations,
                      void* d_keep, uint64_t* d_keep_cnt, float* d_h, const int32_t* d_found, uint32_t* d_iterations);
// the pose stage after model_refit (akz_pose.hip; the statement: akz_pose.hpp), for a fundamental matrix that was handed back: per
// pair with found = 1 the decomposition of E = K1^T F K0 from the model at d_f + 9 pair and the cameras d_cameras[2 pair] (image 0)
// and d_cameras[2 pair + 1] (image 1), the cheirality counts of the four candidates over the KEPT list (coordinates from d_kx / d_ky
// at kp0_off / kp1_off + the records' indices), the pose at d_poses[pair]; with a pose the kept list compacted in place to the matches
// in front, its count rewritten, and (d_points != null) 3 floats per kept record at d_points + 3 keep_off.  A pair with found = 0
// is left alone: its pose must be zero already.
void pairs_pose(hipStream_t s, const PairJobHost* d_pairs, uint32_t n_pairs, const akz_camera* d_cameras,
                const float* d_kx, const float* d_ky, const float* d_f, const int32_t* d_found, void* d_keep, uint64_t* d_keep_cnt,
                akz_pose* d_poses, float* d_points);
// The seeded pairs call (akz_match_seeded_api.cpp; the statement: akz_ransac_seeded.hpp).  seeded_round: round `round` of every pair
// with d_done[pair] == 0 -- its trials draw their own samples from (k1, stream_base + pair, trial) -- into the pair's ring of
// 128 models and counts.  seeded_update: per running pair the round's first maximum against d_best_inl / d_best_mdl (strictly
// greater replaces), d_trials_run, d_done from d_need[pair * need_stride + need_index] (null: no stopping rule) or the last round, and
// the pairs that go on counted in d_running[round].
void seeded_round(hipStream_t s, RansacModel model, const PairJobHost* d_pairs, uint32_t n_pairs, const uint32_t* d_done, uint64_t k1,
                  uint64_t stream_base, uint32_t round, uint32_t max_trials, const uint64_t* d_raw_cnt, const float* d_pts, uint64_t pts_stride,
                  float epsilon_model, float epsilon_inlier, float* d_ring_mdl, int32_t* d_ring_inl);
void seeded_update(hipStream_t s, uint32_t n_pairs, uint32_t round, uint32_t max_trials, const uint32_t* d_need, uint32_t need_stride,
                   uint32_t need_index, const float* d_ring_mdl, const int32_t* d_ring_inl, uint32_t* d_done, int32_t* d_best_inl, float* d_best_mdl,
                   uint32_t* d_trials_run, uint32_t* d_running, uint32_t model_floats = 9 /* or 15: the resection's r | t | sigma */);
// The resection call (akz_resection.hip; the statement: akz_resection.hpp).  Problem p: its n correspondences at d_planes +
// {0 .. 4} * stride + off (X | Y | Z | u | v), its camera as the statement's f32 casts, its kept indices at d_kept + off.
struct ResJobHost {
    uint64_t off;
    uint32_t n, pad;
    float fx, fy, cx, cy;
};
static_assert(sizeof(ResJobHost) == 32, "the device reads 32-byte problem records");
// resection_round: seeded_round for this model -- a ring of 128 models of 15 floats and counts per problem; seeded_update(.., 15)
// follows it.  resection_finish, after the last round: per problem found = best count > 0, the refit loop from the best model
// (max_iterations > 0 and found), the kept indices compacted in order, their count, the accepted fits and the akz_resection (zeros
// where found is 0).
void resection_round(hipStream_t s, const ResJobHost* d_jobs, uint32_t n_problems, const uint32_t* d_done, uint64_t k1, uint64_t stream_base,
                     uint32_t round, uint32_t max_trials, const float* d_planes, uint64_t stride, float epsilon_model, float epsilon_inlier,
                     float* d_ring_mdl, int32_t* d_ring_inl);
void resection_finish(hipStream_t s, const ResJobHost* d_jobs, uint32_t n_problems, const float* d_planes, uint64_t stride,
                      const float* d_best_mdl, const int32_t* d_best_inl, float epsilon_model, float epsilon_inlier, uint32_t max_iterations,
                      uint32_t* d_kept, uint32_t* d_n_kept, uint32_t* d_fits, akz_resection* d_poses);
void unpack_pair(hipStream_t s, const uint8_t* dq, uint32_t nq, uint32_t q_pad, uint8_t* outq, uint32_t* popq, uint32_t* bound, uint32_t threshold,
                 const uint8_t* dt, uint32_t nt, uint32_t t_pad, uint8_t* outt, uint32_t* popt, bool fp4);
uint32_t match_mfma_tile_rows();
uint32_t match_mfma_query_block();
struct MatchChunkHost {  // = MatchChunk of akz_match.hip
    uint32_t t_begin, t_end, row0, n_rows, bound_off, record;
};
void match_mfma_multi(hipStream_t s, const uint8_t* q8, const uint32_t* qpop, uint32_t n0, const uint8_t* t8,
                      const void* d_table, uint32_t n_chunks, uint32_t threshold, uint32_t* bound, MatchRec* d_out, bool fp4 = false);
void match_mfma(hipStream_t s, const uint8_t* q8, const uint32_t* qpop, uint32_t n0, const uint8_t* t8, uint32_t n1,
                uint32_t threshold, uint32_t* bound, uint32_t chunks, MatchRec* d_rec, bool fp4 = false);
// both directions of a multi-set launch (FP4 form): see k_match_fp4<COLS> in akz_match.hip
struct MatchColSetHost {  // = ColSet of akz_match.hip
    uint32_t row0, rows, out0;
};
uint32_t match_cols_seed_rows(uint32_t n0);
void match_cols_seed(hipStream_t s, const uint8_t* q4, uint32_t n0, const uint8_t* t4, uint32_t t_rows, uint32_t threshold,
                     uint32_t* d_bound, MatchRec* d_seed, unsigned long long* cbest, uint32_t* csecond);
void match_fp4_multi_mutual(hipStream_t s, const uint8_t* q4, uint32_t n0, const uint8_t* t4, const void* d_table, uint32_t n_chunks,
                            uint32_t threshold, uint32_t* bound, MatchRec* d_out, unsigned long long* cbest, uint32_t* csecond);
void match_compact_cols(hipStream_t s, const unsigned long long* cbest, const uint32_t* csecond, const void* d_sets, uint32_t n_sets,
                        uint32_t threshold, double ratio2, akz_match* d_out, unsigned long long* d_n_out);
// set k's `chunks` chunk records at d_rec + k * chunks * n0, its matches at d_out + k * n0, its count at d_n_out[k]
void match_compact_sets(hipStream_t s, const MatchRec* d_rec, uint32_t n0, uint32_t n_sets, uint32_t chunks, uint32_t threshold,
                        double ratio2, akz_match* d_out, unsigned long long* d_n_out);
void match_compact(hipStream_t s, const MatchRec* d_rec, uint32_t n0, uint32_t chunks, uint32_t threshold, double ratio2,
                   akz_match* d_out, unsigned long long* d_n_out);
// the same merge as a kernel of its own, one thread per query (many chunks): d_out[query]
void match_merge(hipStream_t s, const MatchRec* d_part, uint32_t n0, uint32_t chunks, uint32_t threshold, MatchRec* d_out);
// merge + ratio test + ordered compaction of one set in one launch; d_state: match_merge_compact_state_bytes(n0) bytes that
// were zero when allocated and are only ever written by this kernel; epoch: different for every call on that buffer, never 0
size_t match_merge_compact_state_bytes(uint32_t n0);
void match_merge_compact(hipStream_t s, const MatchRec* d_part, uint32_t n0, uint32_t chunks, uint32_t threshold, double ratio2,
                         akz_match* d_out, unsigned long long* d_n_out, void* d_state, uint32_t epoch);
// guided matching (akz_guided.hip): the scan of `match` over many pairs at once, in which a train row competes for a query
// only if the pair's model (kind 0: homography, 1: fundamental matrix; d_models + 9 * model) sends the query within
// `radius` pixels of it.  d_rows / d_kx / d_ky: 64-byte rows and keypoint coordinates of every set; a table entry per
// pair WITH rows on both sides, its workgroups wg0 .. wg0 + ceil(n0 / match_guided_block()) * chunks - 1; records as
// `match` writes them, at d_rec[rec_off + chunk * n0 + query].  d_found (optional): pairs with found[model] == 0 get the
// records of an empty scan.
struct GuidedPairHost {  // = GuidedPair of akz_guided.hip
    uint64_t rec_off;
    uint32_t q_row0, n0, t_row0, n1, wg0, chunks, chunk_rows, model;
};
uint32_t match_guided_block();
void match_guided(hipStream_t s, int kind, const uint8_t* d_rows, const float* d_kx, const float* d_ky, const GuidedPairHost* d_tab,
                  uint32_t n_tab, uint32_t n_workgroups, const float* d_models, const int32_t* d_found, float radius,
                  uint32_t threshold, MatchRec* d_rec);
// the cross-check (akz_cross.hip, k_pairs_cross_filter): per pair the forward list at d_fwd + fwd_off (its count at
// d_fwd_cnt[fwd_cnt_idx]) is rewritten in place, in order, to the records m for which the reverse list at d_rev + rev_off (count
// at d_rev_cnt[rev_cnt_idx], ascending index_0) holds r with r.index_0 == m.index_1 and r.index_1 == m.index_0; the count follows.
// fwd_cap / rev_cap: the room of the two lists (a count above it is cut to it).  One workgroup per pair.
struct CrossJobHost {
    uint64_t fwd_off, rev_off;
    uint32_t fwd_cnt_idx, rev_cnt_idx, fwd_cap, rev_cap;
};
static_assert(sizeof(CrossJobHost) == 32, "the device reads 32-byte cross records");
void pairs_cross_filter(hipStream_t s, const CrossJobHost* d_tab, uint32_t n_pairs, akz_match* d_fwd, uint64_t* d_fwd_cnt,
                        const akz_match* d_rev, const uint64_t* d_rev_cnt);
// the same for one pair whose record travels with the launch (no table on the device)
void pair_cross_filter(hipStream_t s, const CrossJobHost& job, akz_match* d_fwd, uint64_t* d_fwd_cnt, const akz_match* d_rev,
                       const uint64_t* d_rev_cnt);
// the feature bank's gather (akz_bank.hip, k_bank_gather): n_seg segments of 64-byte rows -- n_rows rows at src_rows to the rows
// from dst_row0 on of d_dst -- in ONE launch; dst_row0 ascends, segment s + 1 starts where s ends (0-row segments included),
// total_rows is their sum.  Bytes of a row at or beyond desc_bytes are stored as zero.
struct BankSeg {
    const uint8_t* src_rows;
    uint64_t n_rows, dst_row0;
};
static_assert(sizeof(BankSeg) == 24, "the device reads 24-byte segment records");
constexpr uint64_t kBankMaxRows = 0x7fffffffull * 64;  // (a launch's workgroups, at no fewer than 64 rows each)
void bank_gather(hipStream_t s, const BankSeg* d_tab, uint32_t n_seg, uint64_t total_rows, uint32_t desc_bytes, uint8_t* d_dst);
// the budgeted bank's gather (akz_bank.hip, k_bank_select): set s sends `keep` of its rows -- those that d_idx[idx_off + t],
// t < keep, names, ascending and below the set's row count -- to the rows from dst_row0 on, in ONE launch over n_set records laid
// out as the segments above (dst_row0 ascends, record s + 1 starts where s ends, total_rows is the sum of keep).  Destination row
// r = dst_row0 + t, with i the index it names, receives row i of src_rows (bytes at or beyond desc_bytes as zero),
// d_sx / d_sy[src_base + i], and i itself in d_dst_src.
struct BankSel {
    const uint8_t* src_rows;
    uint64_t src_base, keep, dst_row0, idx_off;
};
static_assert(sizeof(BankSel) == 40, "the device reads 40-byte selection records");
void bank_select(hipStream_t s, const BankSel* d_tab, uint32_t n_set, uint64_t total_rows, uint32_t desc_bytes, const uint32_t* d_idx,
                 const float* d_sx, const float* d_sy, uint8_t* d_dst, float* d_dx, float* d_dy, uint32_t* d_dst_src);
// k-nearest-neighbour matching (akz_knn.hip): q4 / t4 are the FP4 images of unpack_pair(fp4); `chunks` from knn_chunks (forced: the
// test hook, 0 = automatic; never fewer than the row field of a key allows); d_part: knn_part_bytes bytes of partial lists.
// Writes k records per query and its count (all padding for n1 == 0); false: arguments or a retuned tile the kernel was not built for.
uint32_t knn_list_len(uint32_t k);  // k rounded up to the list length the kernel is built for (1, 2, 4, 8)
uint32_t knn_chunks(uint32_t n0, uint32_t n1, uint32_t forced = 0);
size_t knn_part_bytes(uint32_t n0, uint32_t chunks, uint32_t k);
bool knn(hipStream_t s, const uint8_t* q4, uint32_t n0, const uint8_t* t4, uint32_t n1, uint32_t threshold, uint32_t chunks, uint32_t k,
         uint32_t* d_part, akz_match* d_out, uint32_t* d_counts);
// The keypoint budget (akz_budget.hip; include/akaze_hip.h).  All sets of a call lie packed one after the other: d_x, d_y, d_r hold
// `total` floats each, set s at [base, base + n).  keep = min(max_keypoints, n); out_off: where the set's kept indices start in d_idx
// (the sets' lists lie densely one after the other: their lengths are known before the launch).
struct BudgetSet {
    uint32_t base, n, keep, out_off;
};
// One workgroup of k_budget_walk: queries [q0, q0 + budget_query_tile()) of set `set` against its keypoints [t0, t1)
struct BudgetBlock {
    uint32_t set, q0, t0, t1;
};
static_assert(sizeof(BudgetSet) == 16 && sizeof(BudgetBlock) == 16, "the device reads 16-byte budget records");
uint32_t budget_query_tile();   // queries of a workgroup (1024)
uint32_t budget_train_tile();   // keypoints of one LDS stage (256); a block's [t0, t1) starts on a multiple of it
// radius2 := +inf, rank := 0 for `total` keypoints; then (spread) the radius pass and the rank pass over the n_blocks records of
// d_blocks, and the ordered compaction, one workgroup per set: d_idx[out_off + k] = the k-th index i (ascending) with rank_i < keep
void budget(hipStream_t s, bool spread, float robust, const float* d_x, const float* d_y, const float* d_r, uint32_t total,
            const BudgetSet* d_sets, uint32_t n_sets, const BudgetBlock* d_blocks, uint32_t n_blocks, float* d_radius2, uint32_t* d_rank,
            uint32_t* d_idx);
}  // namespace launch

// ---- host keypoint logic (akz_keypoints.cpp) ---------------------------------------------
struct HostKeypoint {
    float x, y, response, size;
    uint32_t octave, class_id;
    float angle;
    // level coordinates + 4-neighbour Ldet values carried from the NMS kernel
    uint32_t lx, ly;
    float xp, xm, yp, ym;
};
// unordered NMS survivors of one image into the reference's scan order: level, then flat index
void sort_candidates(std::vector<Candidate>& cands, const std::vector<LevelPlan>& plan);
// scale_space_extrema.rs:12-132 on raster-ordered candidates, then :141-178 (refinement w/o orientation)
void select_keypoints(const Candidate* cands_sorted, size_t n_cands, const std::vector<LevelPlan>& plan,
                      const akz_config& cfg, std::vector<HostKeypoint>& out, uint64_t* n_extrema);
// the same selection from the device's neighbour lists (launch::candidate_relations; rel: k1 + k2 entries per candidate)
void select_keypoints_rel(const Candidate* cands_sorted, size_t n_cands, const uint16_t* rel, int k1, int k2, const std::vector<LevelPlan>& plan,
                          const akz_config& cfg, std::vector<HostKeypoint>& out, uint64_t* n_extrema);
// the per-level constants of the selection (f32, as select_keypoints forms them)
void selection_level_constants(const std::vector<LevelPlan>& plan, const akz_config& cfg, std::vector<float>& size, std::vector<float>& ratio);
// which of the sliding windows of compute_main_orientation contain atan2f(a, a), a > 0
void orientation_windows(unsigned long long* mask, uint32_t* n_windows);
float border_margin(const LevelPlan& lv, const akz_config& cfg);  // smax * sigma_size (f32)

}  // namespace akz

// ---- plane stores (device code only) --------------------------------------------------------------------------
// The tiled stencil / FED kernels use ordinary stores: streaming (nontemporal) stores measured the same there in
// round 1 (those kernels are bound by their on-chip dependency chains); the column march (akz_march.hip), which IS
// bound by the store path, uses them (+20 %).
#if defined(__HIPCC__)
namespace akz {
typedef float akz_f4a __attribute__((ext_vector_type(4)));                // 16-byte aligned group of four pixels
typedef float akz_f4u __attribute__((ext_vector_type(4), aligned(4)));    // dword-aligned group of four pixels
__device__ __forceinline__ void plane_store(float* p, float v) { *p = v; }
__device__ __forceinline__ void plane_store4(float* p, float a, float b, float c, float d) {  // p 16-byte aligned
    const akz_f4a t = {a, b, c, d};
    *reinterpret_cast<akz_f4a*>(p) = t;
}
__device__ __forceinline__ void plane_store4u(float* p, akz_f4a t) {  // p dword-aligned
    *reinterpret_cast<akz_f4u*>(p) = t;
}
}  // namespace akz
#endif
