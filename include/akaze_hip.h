/* akaze_hip.h — C ABI of the MI355X-native A-KAZE hot path (libakaze_hip.so).
 *
 * The reference crate (indianajohn/akaze-rust) has no FFI/plugin boundary; its
 * drop-in boundary is the public Rust API.  Every entry point below names the
 * reference item it replaces (paths relative to the reference repository root).
 * A Rust shim that re-exports the reference signatures over these symbols is in
 * akaze-rust_amd/rust/ and described in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns AKZ_OK (0) or a negative akz_status; nothing throws
 *     or aborts across the ABI.  akz_last_error() gives a thread-local message.
 *   - an akz_ctx is bound to one GPU and one HIP stream and is NOT thread-safe;
 *     use one context per host thread / per GPU.
 *   - images are row-major, contiguous, index = w*y + x, exactly like
 *     GrayFloatImage (akaze/src/types/image.rs:32-36).  A batch of n images of
 *     equal size is n such planes back to back (plane stride = w*h elements).
 *   - pointers named d_* are DEVICE pointers (hipMalloc / torch CUDA tensors);
 *     all others are host pointers.
 *   - "op" entry points enqueue on the context's stream and return without
 *     synchronising unless they hand a value back to the host.
 */
#ifndef AKAZE_HIP_H
#define AKAZE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 3): additions only -- akz_extract_begin_host_*, akz_ctx_set_host_threads, akz_ctx_set_eager_finish,
   akz_gather_image_rows, akz_match_all_pairs / akz_pairs_*, AKZ_INPUT_READY; the gather's overflow protocol.  Every
   entry point of version 2 keeps its signature and meaning.
   4 (round 4): akz_descriptor_match_sets_mutual_device and akz_pairs_holder added; akz_match_all_pairs matches every
   unordered image pair once and a rank's akz_pairs holds both lists of the pairs whose lead image it owns (version 3: the
   ordered pairs whose query image it owns); akz_ctx_set_eager_finish covers the context's own jobs and defaults to on;
   the kernel-family selectors and the synthetic-frame generator moved to akaze_hip_debug.h (still exported).  No
   signature changed.
   5 (round 5): additions -- akz_comm_create_external / akz_gather_blocks / akz_gather_deliver (the exchange carried by the
   caller), akz_comm_set_timeout, akz_pairs_totals, akz_ctx_warmup; akz_profile grew by the placement_* fields at its END
   (a caller built against version 4 must not pass its smaller struct to akz_ctx_get_profile); an akz_pairs may be freed
   after its communicator; AKZ_ERR_TIMEOUT.  No signature changed.
   6 (round 6): additions -- akz_ctx_get_profile2 (size-checked; akz_ctx_get_profile writes the ABI-4 prefix of akz_profile
   only from now on); akz_op_scharr accepts both and neither order as the reference does; a communicator whose exchange
   timed out is abandoned (akz_comm_set_timeout); AKZ_COMM_HOST communicators, akz_gather_begin_image_rows, akz_pairs_plan,
   akz_pairs_lead_sets.  No signature changed. */
#define AKZ_ABI_VERSION 6

typedef enum akz_status {
    AKZ_OK = 0,
    AKZ_ERR_INVALID_ARG = -1,  /* null pointer, zero size, unsupported Config value    */
    AKZ_ERR_HIP = -2,          /* a HIP runtime call failed (message in akz_last_error) */
    AKZ_ERR_NO_DEVICE = -3,    /* no gfx950 device visible / extension cannot run        */
    AKZ_ERR_TOO_SMALL = -4,    /* image smaller than the stencil supports                */
    AKZ_ERR_OVERFLOW = -5,     /* a fixed-capacity device buffer (candidates) overflowed */
    AKZ_ERR_UNSUPPORTED = -6,  /* reference behaviour that does not terminate / panics   */
    AKZ_ERR_BUFFER = -7,       /* caller buffer too small                                */
    AKZ_ERR_IO = -8,           /* an image file cannot be read / written or is malformed */
    AKZ_ERR_NO_MEMORY = -9,    /* host allocation failed                                 */
    AKZ_ERR_TIMEOUT = -10      /* an exchange did not complete within akz_comm_set_timeout (a peer is missing or hung) */
} akz_status;

/* types::evolution::Config — akaze/src/types/evolution.rs:8-38 (defaults :40-55). */
typedef struct akz_config {
    uint32_t num_sublevels;
    uint32_t max_octave_evolution;
    double base_scale_offset;
    double initial_contrast; /* declared by the reference, never read */
    double contrast_percentile;
    uint64_t contrast_factor_num_bins;
    double derivative_factor;
    double detector_threshold;
    uint64_t descriptor_channels;
    uint64_t descriptor_pattern_size;
} akz_config;

/* types::keypoint::Keypoint — akaze/src/types/keypoint.rs:8-30 (point = (x, y)). */
typedef struct akz_keypoint {
    float x, y;
    float response;
    float size;
    uint64_t octave;
    uint64_t class_id;
    float angle;
    uint32_t _pad;
} akz_keypoint;

/* types::feature_match::Match — akaze/src/types/feature_match.rs:9-16. */
typedef struct akz_match {
    uint64_t index_0;
    uint64_t index_1;
    double distance;
} akz_match;

/* EvolutionStep image fields in declaration order — akaze/src/types/evolution.rs:71-89. */
typedef enum akz_plane {
    AKZ_LT = 0, AKZ_LSMOOTH = 1, AKZ_LX = 2, AKZ_LY = 3, AKZ_LXX = 4,
    AKZ_LYY = 5, AKZ_LXY = 6, AKZ_LFLOW = 7, AKZ_LSTEP = 8, AKZ_LDET = 9
} akz_plane;

/* akz_extract_* flags */
enum {
    /* keep every EvolutionStep plane resident so akz_fetch_plane can return it
       (what extract_features returns, akaze/src/lib.rs:193).  Without it only the
       planes later stages read (Lt, Lsmooth, Lx, Ly, Lflow, Ldet) are materialised and
       Lxx/Lyy/Lxy/Lstep are never written. */
    AKZ_KEEP_ALL_PLANES = 1u << 0,
    /* leave keypoints/descriptors on the device only (no D2H of descriptors) */
    AKZ_NO_HOST_DESCRIPTORS = 1u << 1,
    /* akz_extract_from_planes only: upload the planes, skip the extrema pass (keypoints come from the caller through
       akz_result_describe_keypoints) */
    AKZ_NO_DETECT = 1u << 2,
    /* akz_extract_begin_device_*: the caller promises that the frames are COMPLETE in device memory when the call is made
       -- nothing still pending on the context's stream (or on any other) writes them -- and stay untouched until the job
       is finished.  The first stages of a large batch (level-0 blur, contrast factor) then do not wait for the work the
       context's stream still holds for the batch before and run under that batch's kernels.  Without the flag the
       library has to assume that the frames are produced by whatever the caller enqueued on the stream before the call.
       (akz_extract_begin_host_* knows when its own upload is complete and always runs ahead.)  Results are identical.
       Takes effect only in a process started with GPU_MAX_HW_QUEUES >= 8 in its environment (threading):
       with the runtime's default of 4 in-order hardware queues one more busy stream would serialise the pipeline. */
    AKZ_INPUT_READY = 1u << 3
};

typedef struct akz_ctx akz_ctx;
typedef struct akz_result akz_result;
typedef struct akz_job akz_job; /* an extraction in flight, see akz_extract_begin_* */

/* ---- library ------------------------------------------------------------------------ */
int akz_abi_version(void);
const char* akz_last_error(void);
/* Config::default() — akaze/src/types/evolution.rs:40-55 */
void akz_config_default(akz_config* out);

/* ---- context ------------------------------------------------------------------------ */
/* stream: the hipStream_t every kernel and copy of this context is enqueued on, e.g.
   torch.cuda.current_stream().cuda_stream.  NULL is the device's default (null) stream, as in
   every HIP API.  akz_stream_create/destroy give non-torch hosts a private stream. */
int akz_ctx_create(int device, void* stream, akz_ctx** out);
int akz_stream_create(int device, void** stream_out);
int akz_stream_destroy(int device, void* stream);
/* Results and jobs of the context may be freed after it (they keep their host data; device accessors then
   return AKZ_ERR_INVALID_ARG). */
int akz_ctx_destroy(akz_ctx* ctx);
int akz_ctx_synchronize(akz_ctx* ctx);
void* akz_ctx_stream(akz_ctx* ctx);

/* plain device-memory helpers so a non-torch host (the Rust shim) needs no HIP bindings */
int akz_device_malloc(akz_ctx* ctx, size_t bytes, void** d_out);
int akz_device_free(akz_ctx* ctx, void* d_ptr);
int akz_memcpy_h2d(akz_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int akz_memcpy_d2h(akz_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* ---- host-side planning (scalar code the reference also runs on the CPU) ------------- */
/* ops::fed_tau::fed_tau_by_process_time — akaze/src/ops/fed_tau.rs:27-30 (+ :43-106).
   Writes min(*n, cap) step sizes.  AKZ_ERR_UNSUPPORTED where the reference never
   terminates (n == 1 with reordering, fed_tau.rs:95). */
int akz_fed_tau_by_process_time(double T, int M, double tau_max, int reordering, double* out, uint64_t cap,
                                uint64_t* n);
/* types::image::gaussian_kernel — akaze/src/types/image.rs:352-365 */
int akz_gaussian_kernel(float sigma, uint64_t kernel_size, float* out);
/* ops::derivatives::scharr_{main,off}_axis_kernel — akaze/src/ops/derivatives.rs:74-101 */
int akz_scharr_kernels(uint32_t scale, float* main_axis, float* off_axis);
/* types::evolution::allocate_evolutions — akaze/src/types/evolution.rs:135-161.
   Level sizes follow the chained half_size of create_nonlinear_scale_space (lib.rs:80-90). */
int akz_plan_num_levels(uint32_t w, uint32_t h, const akz_config* cfg, uint64_t* n_levels);
int akz_plan_level_info(uint32_t w, uint32_t h, const akz_config* cfg, uint64_t level, double* etime, double* esigma,
                        uint32_t* octave, uint32_t* sublevel, uint32_t* sigma_size, uint32_t* level_w,
                        uint32_t* level_h, uint32_t* detector_sigma, uint64_t* n_tau, double* tau, uint64_t tau_cap);

/* ---- per-op entry points on device planes (mirror of `pub mod ops` / `types::image`) -- */
/* types::image::horizontal_filter / vertical_filter incl. fill_border — image.rs:239-332 */
int akz_op_horizontal_filter(akz_ctx* ctx, const float* d_in, float* d_out, uint32_t w, uint32_t h, uint32_t n,
                             const float* taps, uint32_t ntaps);
int akz_op_vertical_filter(akz_ctx* ctx, const float* d_in, float* d_out, uint32_t w, uint32_t h, uint32_t n,
                           const float* taps, uint32_t ntaps);
/* types::image::gaussian_blur — image.rs:374-380 */
int akz_op_gaussian_blur(akz_ctx* ctx, const float* d_in, float* d_out, uint32_t w, uint32_t h, uint32_t n,
                         float sigma);
/* create_unit_float_image + gaussian_blur on 8-bit luma — image.rs:127-140, lib.rs:56 */
int akz_op_gaussian_blur_u8(akz_ctx* ctx, const uint8_t* d_in, float* d_out, uint32_t w, uint32_t h, uint32_t n,
                            float sigma);
/* ImageFunctions::half_size — image.rs:102-118 ; out is (w/2) x (h/2) */
int akz_op_half_size(akz_ctx* ctx, const float* d_in, float* d_out, uint32_t w, uint32_t h, uint32_t n);
/* ops::derivatives::scharr — derivatives.rs:112-130, all four order combinations as the reference has them:
 * x only / y only -> scharr_horizontal / scharr_vertical; both -> the horizontal derivative added to itself (:118-122 via
 * image.rs:218-231); neither -> a zero image (:127-128; sigma_size unused). */
int akz_op_scharr(akz_ctx* ctx, const float* d_in, float* d_out, uint32_t w, uint32_t h, uint32_t n, int x_order,
                  int y_order, uint32_t sigma_size);
/* pm_g2 — lib.rs:26-41 ; d_k: n contrast factors (double) on the device */
int akz_op_pm_g2(akz_ctx* ctx, const float* d_lx, const float* d_ly, float* d_out, uint32_t w, uint32_t h, uint32_t n,
                 const double* d_k);
/* ops::contrast_factor::compute_contrast_factor — contrast_factor.rs:18-71 ; writes n doubles to d_k_out */
int akz_op_contrast_factor(akz_ctx* ctx, const float* d_in, uint32_t w, uint32_t h, uint32_t n, double percentile,
                           double gradient_histogram_scale, uint64_t num_bins, double* d_k_out);
/* Lsmooth -> Lflow of one level: scharr(sigma 1) x2 + pm_g2 — lib.rs:98-105.
   d_k: per-image contrast factor of octave 0; k_scale_pow = number of x0.75 octave steps (lib.rs:84). */
int akz_op_flow(akz_ctx* ctx, const float* d_lsmooth, float* d_lflow, uint32_t w, uint32_t h, uint32_t n,
                const double* d_k, uint32_t k_scale_pow);
/* ops::nonlinear_diffusion::calculate_step, n_tau times — nonlinear_diffusion.rs:15-144.
   d_lt is updated in place (as the reference does); d_lstep (may be NULL) receives the
   last step's increment.  taus are the f64 step sizes of the level. */
int akz_op_fed_steps(akz_ctx* ctx, float* d_lt, const float* d_lflow, float* d_lstep, uint32_t w, uint32_t h,
                     uint32_t n, const double* taus, uint32_t n_tau);
/* compute_multiscale_derivatives_for_evolution + Ldet — detector_response.rs:8-14, :40-54.
   d_lxx/d_lyy/d_lxy may be NULL (not materialised). */
int akz_op_detector_response(akz_ctx* ctx, const float* d_lsmooth, uint32_t sigma_size, float* d_lx, float* d_ly,
                             float* d_lxx, float* d_lyy, float* d_lxy, float* d_ldet, uint32_t w, uint32_t h,
                             uint32_t n);

/* ---- the hot path: extract_features -------------------------------------------------- */
/* akaze::extract_features — akaze/src/lib.rs:167-194, minus image::open/to_luma (ingest is
   upstream of the path).  Host-buffer forms copy the frame(s) H2D first. */
int akz_extract_gray_u8(akz_ctx* ctx, const uint8_t* img, uint32_t w, uint32_t h, const akz_config* cfg,
                        uint32_t flags, akz_result** out);
int akz_extract_gray_f32(akz_ctx* ctx, const float* img, uint32_t w, uint32_t h, const akz_config* cfg,
                         uint32_t flags, akz_result** out);
/* n equally sized frames already resident in HBM; one result handle for the batch */
int akz_extract_device_u8(akz_ctx* ctx, const uint8_t* d_imgs, uint32_t w, uint32_t h, uint32_t n,
                          const akz_config* cfg, uint32_t flags, akz_result** out);
int akz_extract_device_f32(akz_ctx* ctx, const float* d_imgs, uint32_t w, uint32_t h, uint32_t n,
                           const akz_config* cfg, uint32_t flags, akz_result** out);

/* Two-phase form for streaming: begin enqueues the scale space, the detector response and the extrema
   candidates of a batch on the context's stream and returns WITHOUT synchronising; finish waits for
   that batch only, runs the host keypoint logic, orientation and descriptors (on an auxiliary stream)
   and hands the result over.  Begin the next batch before finishing the previous one and the host
   phase of one runs under the kernels of the other.  Up to 3 jobs in flight per context; a job must be
   finished (or abandoned) exactly once; the frames must stay valid until then. */
int akz_extract_begin_device_u8(akz_ctx* ctx, const uint8_t* d_imgs, uint32_t w, uint32_t h, uint32_t n,
                                const akz_config* cfg, uint32_t flags, akz_job** out);
int akz_extract_begin_device_f32(akz_ctx* ctx, const float* d_imgs, uint32_t w, uint32_t h, uint32_t n,
                                 const akz_config* cfg, uint32_t flags, akz_job** out);
/* The same for frames in HOST memory (the reference's extract_features starts from host data, lib.rs:171-178): the
   n frames are copied into a staging buffer of the context on its COPY stream, the extraction waits for that copy
   only -- so with batch j+1 begun before batch j is finished, the upload of j+1 runs under the kernels of j.  Pinned
   memory (hipHostMalloc / hipHostRegister) makes the copy asynchronous; pageable memory works and is staged by the
   runtime.  h_imgs must stay valid until the job is finished or abandoned. */
int akz_extract_begin_host_u8(akz_ctx* ctx, const uint8_t* h_imgs, uint32_t w, uint32_t h, uint32_t n,
                              const akz_config* cfg, uint32_t flags, akz_job** out);
int akz_extract_begin_host_f32(akz_ctx* ctx, const float* h_imgs, uint32_t w, uint32_t h, uint32_t n,
                               const akz_config* cfg, uint32_t flags, akz_job** out);
int akz_extract_finish(akz_job* job, akz_result** out);
int akz_job_abandon(akz_job* job);

/* ---- frames as their producer holds them: colour, pitched, strided, cropped ---------- */
/* `image::open(path).to_luma()` (akaze/src/lib.rs:171-172) for frames that are already in memory: what a decoder, a torch
   pipeline or a region of interest hands over, read where it lies.  The luma of a colour pixel is DynamicImage::to_luma's
   (f32 weights 0.2126 / 0.7152 / 0.0722, unfused, truncated) -- bit for bit the frame akz_image_load_luma gives for the
   same pixels, so a picture gives the same keypoints through a file and through these calls. */
typedef enum akz_frame_format {
    AKZ_FRAME_GRAY8 = 0,        /* 1 byte / px; to_luma of a one-channel image is the identity (an NV12 Y plane is this, with its pitch) */
    AKZ_FRAME_RGB8 = 1, AKZ_FRAME_BGR8 = 2,      /* interleaved, 3 bytes / px */
    AKZ_FRAME_RGBA8 = 3, AKZ_FRAME_BGRA8 = 4,    /* interleaved, 4 bytes / px; alpha ignored, as to_luma of an Rgba image drops it */
    AKZ_FRAME_RGB8_PLANAR = 5                    /* three planes R, G, B (torch [N,3,H,W]) */
} akz_frame_format;
/* A crop is the caller's pointer moved to the region's first pixel plus the parent's pitch (no origin fields).  Tight
   values: row_pitch = width * bytes per pixel (1 for the planar format); plane_stride = row_pitch * height; frame_stride =
   row_pitch * height, planar 3 * plane_stride.  Only the bytes of the declared rows are ever read, in naturally aligned
   words of 4 bytes that hold at least one of them: no padding behind the last row is needed. */
typedef struct akz_frame_layout {
    uint32_t format, width, height;   /* width x height: the region extracted, in pixels */
    uint64_t row_pitch;     /* bytes from a row to the next; 0 = tight (width * bytes per pixel) */
    uint64_t frame_stride;  /* bytes from a frame to the next; 0 = tight */
    uint64_t plane_stride;  /* planar only: bytes from R to G and G to B; 0 = row_pitch * height */
} akz_frame_layout;
/* Refusals of the four calls below, all AKZ_ERR_INVALID_ARG with the field named in akz_last_error, nothing written or
   enqueued and *out = NULL: a null pointer, n = 0, an unknown format, a zero width or height, a nonzero row_pitch,
   frame_stride or plane_stride below its tight value.  Frames too small for the stencils: AKZ_ERR_TOO_SMALL, as ever. */
/* The statement: luma[n][height][width] (packed) of n frames in HOST memory.  No context, no GPU call. */
int akz_luma_from_frames_host(const uint8_t* src, const akz_frame_layout* layout, uint32_t n, uint8_t* luma);
/* The same on the device, enqueued on the context's stream (not synchronised).  d_luma may have any alignment; only its
   n * width * height bytes are written. */
int akz_luma_from_frames_device(akz_ctx* ctx, const uint8_t* d_src, const akz_frame_layout* layout, uint32_t n, uint8_t* d_luma);
/* The result of akz_extract_device_u8 on akz_luma_from_frames_device of the frames, bit for bit.  The luma frames go
   into a staging buffer of the context that belongs to the job (AKZ_FRAME_GRAY8 with tight strides is handed to
   akz_extract_device_u8 as it is). */
int akz_extract_device_frames(akz_ctx* ctx, const uint8_t* d_src, const akz_frame_layout* layout, uint32_t n,
                              const akz_config* cfg, uint32_t flags, akz_result** out);
/* The two-phase form (akz_extract_begin_device_u8).  Without AKZ_INPUT_READY the frames may be the output of work the
   caller enqueued on the context's stream before the call: the conversion runs on that stream (for a job dealt to a
   lane, on the lane's stream once the caller's stream has reached this point).  With AKZ_INPUT_READY the caller promises
   that the frames are complete NOW: the conversion runs on the context's copy stream, as the upload of
   akz_extract_begin_host_* does, under the kernels of the batch before.  d_src must stay valid and unchanged until the
   job is finished or abandoned. */
int akz_extract_begin_device_frames(akz_ctx* ctx, const uint8_t* d_src, const akz_frame_layout* layout, uint32_t n,
                                    const akz_config* cfg, uint32_t flags, akz_job** out);

/* ---- a detection mask: masked pixels raise no candidates ------------------------------ */
/* The second argument of detectAndCompute.  A mask is height x width bytes per frame, the frame's own size; nonzero means
   detect here (a torch bool tensor is this).  The pyramid, the contrast factor and every plane are untouched by it.  An
   extrema candidate of level l (octave o, r = 1 << o) at level pixel (x, y) exists only if
       mask[(y << o) + (r >> 1)][(x << o) + (r >> 1)] != 0
   -- the rounded position the reference gives the unrefined keypoint (x r + 0.5 (r - 1), scale_space_extrema.rs:89-92), always
   inside the frame.  A masked candidate never reaches the keypoint cache, like one the border test removes; so it suppresses
   no neighbour, which a filter over the finished keypoints cannot undo.  Everything behind the candidate list is unchanged
   (cache walk, second pass, sub-pixel step, orientation, descriptors): a keypoint may be refined up to one level pixel into a
   masked pixel.  Cost: one 12-byte fill and one small launch per job, between the extrema pass and everything that reads
   its list; calls without a mask enqueue and allocate nothing new.
   mask_layout: format AKZ_FRAME_GRAY8, the frames' width and height; row_pitch and frame_stride are free, as for frames.
   n_masks: 1 (one mask for every frame; its frame_stride is not looked at) or n.  d_mask == NULL together with mask_layout ==
   NULL is the unmasked call.  The mask follows the frames' stream rules: without AKZ_INPUT_READY it may be the output of work
   queued earlier on the context's stream, with it the promise covers the mask too; it must stay valid and unchanged until the
   job is finished or abandoned.
   Refusals (AKZ_ERR_INVALID_ARG, the field named in akz_last_error, nothing enqueued, *out = NULL), besides the frames' own:
   exactly one of d_mask / mask_layout null; another format; another size; n_masks not 1 or n; a nonzero row_pitch or
   frame_stride below its tight value.
   f32 frames, akz_extract_from_planes and the file calls (akz_extract_features_file / _files) have no masked form. */
int akz_extract_device_frames_masked(akz_ctx* ctx, const uint8_t* d_src, const akz_frame_layout* layout, uint32_t n,
                                     const uint8_t* d_mask, const akz_frame_layout* mask_layout, uint32_t n_masks,
                                     const akz_config* cfg, uint32_t flags, akz_result** out);
int akz_extract_begin_device_frames_masked(akz_ctx* ctx, const uint8_t* d_src, const akz_frame_layout* layout, uint32_t n,
                                           const uint8_t* d_mask, const akz_frame_layout* mask_layout, uint32_t n_masks,
                                           const akz_config* cfg, uint32_t flags, akz_job** out);
/* akz_extract_gray_u8 with a mask in HOST memory: w * h bytes, tight, uploaded with the frame (mask must not be NULL). */
int akz_extract_gray_u8_masked(akz_ctx* ctx, const uint8_t* img, const uint8_t* mask, uint32_t w, uint32_t h,
                               const akz_config* cfg, uint32_t flags, akz_result** out);

/* ops::scale_space_extrema::detect_keypoints (scale_space_extrema.rs:199-203) and ops::descriptors::extract_descriptors
   (descriptors.rs:14-27) on evolutions the CALLER holds (the reference's `pub mod ops` takes `&[EvolutionStep]` that
   need not come from extract_features): planes = n_levels x 10 host pointers in akz_plane order (row-major f32 of the
   level's size, NULL where the caller has nothing; Lt, Lx, Ly of every level are required, Ldet unless
   AKZ_NO_DETECT), n_levels = what akz_plan_num_levels returns for (w, h, cfg).  The planes are uploaded, the extrema
   test runs on the uploaded Ldet, and the result carries keypoints (with orientation) and descriptors exactly as if
   the pyramid had been built here.  With AKZ_NO_DETECT the result has no keypoints and serves
   akz_result_describe_keypoints / akz_fetch_plane. */
int akz_extract_from_planes(akz_ctx* ctx, uint32_t w, uint32_t h, const akz_config* cfg, const float* const* planes,
                            uint64_t n_levels, uint32_t flags, akz_result** out);

/* Releases the result; its device blocks (pyramid planes, descriptor rows) go back to the context's pool.  Work of the
   CALLER that reads device pointers obtained from the result (akz_result_device_plane, akz_result_device_descriptors) must
   have completed: the next batch's first stages may run ahead on another stream of the context (AKZ_INPUT_READY,
   akz_extract_begin_host_*) and write a pooled block before anything still queued on the caller's stream has run. */
int akz_result_free(akz_result* res);
int akz_result_num_images(const akz_result* res, uint64_t* n_images);
/* (Vec<EvolutionStep>.len(), Vec<Keypoint>.len(), Descriptor.vector.len()) of image `img` */
int akz_result_counts(const akz_result* res, uint64_t img, uint64_t* n_levels, uint64_t* n_keypoints,
                      uint64_t* desc_bytes);
int akz_result_keypoints(const akz_result* res, uint64_t img, akz_keypoint* out /* n_keypoints */);
/* unpadded: n_keypoints * desc_bytes bytes, Descriptor.vector of each keypoint back to back */
int akz_result_descriptors(const akz_result* res, uint64_t img, uint8_t* out);
/* ops::scale_space_extrema::compute_main_orientation (scale_space_extrema.rs:207-329) and
   ops::descriptors::extract_descriptors (descriptors.rs:14-35) for caller-supplied keypoints of image `img` on the
   retained pyramid: uses point, size, octave and class_id of every keypoint; with compute_orientation != 0 the
   angle field is (re)computed and written back, otherwise the given angle is used.  descriptors: n x desc_bytes.
   As in the reference, the orientation divides by 2^octave of the keypoint's LEVEL (class_id) and the descriptor by
   2^octave of the KEYPOINT; the two differ only for keypoints the detector did not emit.  class_id >= n_levels and
   octave > 30 are refused (AKZ_ERR_INVALID_ARG, nothing written).
   Samples outside the plane: every sample coordinate is converted to an integer (saturating, NaN to 0; the orientation
   takes negatives as 0 first, like the reference's `as usize`) and then clamped to [0, w-1] x [0, h-1], so any
   keypoint, non-finite fields included, is memory-safe.  Where all of a keypoint's samples lie inside its plane the
   result is the reference's, bit for bit.  Where the reference would read past the end of a row (x >= w, not on the
   last row: GrayFloatImage::get is the flat buffer[w * y + x], so it reads the next row and completes) this clamps to
   the row's last pixel instead: a documented deviation, for keypoints the detector never emits (it drops everything
   within about twice the descriptor's reach of the border).  Elsewhere (an index past the buffer, a negative
   descriptor coordinate) the reference ends the call with a panic, or wraps, by build profile. */
int akz_result_describe_keypoints(const akz_result* res, uint64_t img, akz_keypoint* kps, uint64_t n_keypoints,
                                  int compute_orientation, uint8_t* descriptors);
/* device-resident descriptors, 64-byte rows (desc_bytes used, rest zero), for akz_match_device / RCCL gather */
int akz_result_device_descriptors(const akz_result* res, uint64_t img, const uint8_t** d_desc, uint64_t* n_keypoints);
/* D2D copy of ALL images' descriptor rows (image 0 first, 64-byte rows) into a caller buffer of
   capacity_rows rows, e.g. a torch tensor that is then all-gathered over RCCL.  Runs on the context's
   auxiliary stream and is complete on return (it never waits for batches still in flight). */
int akz_result_copy_device_descriptors(const akz_result* res, uint8_t* d_dst, uint64_t capacity_rows,
                                       uint64_t* rows);
/* the contrast factor compute_contrast_factor returned for image `img` (lib.rs:64-69) */
int akz_result_contrast(const akz_result* res, uint64_t img, double* k);
/* scalar fields of EvolutionStep — evolution.rs:59-70, :91 */
int akz_result_level_info(const akz_result* res, uint64_t level, double* etime, double* esigma, uint32_t* octave,
                          uint32_t* sublevel, uint32_t* sigma_size, uint32_t* w, uint32_t* h, uint64_t* n_tau,
                          double* tau, uint64_t tau_cap);
/* lazy D2H of one EvolutionStep image; *n_px = 0 for the 0x0 planes (level 0 Lflow/Lstep).  Planes the
   extraction did not keep (Lxx, Lyy, Lxy, Lstep without AKZ_KEEP_ALL_PLANES) are recomputed for this image
   from the kept ones with the same kernels — bit-identical, at the cost of a few launches per call — so an
   EvolutionStep is complete either way.  out may be NULL to query the size. */
int akz_fetch_plane(const akz_result* res, uint64_t img, uint64_t level, akz_plane plane, float* out,
                    uint64_t* n_px);
/* The EvolutionStep images of image `img` of a result, all levels at once, into caller memory (Vec<EvolutionStep>,
   akaze/src/lib.rs:193).  dst has n_levels * 10 entries, level-major, in akz_plane order: dst[level * 10 + plane].
   A NULL entry skips that plane.  Entry (level, plane) needs room for that level's w*h floats
   (akz_result_level_info).  Level 0's Lflow / Lstep (0 x 0) are ignored.
   Planes the extraction did not keep are recomputed, bit-identical to akz_fetch_plane, once per level for all of
   that level's missing planes.  Page-locked destinations (hipHostMalloc, hipHostRegister) are written by DMA directly;
   pageable ones through pinned staging buffers of the context.  *bytes_out (may be NULL) = bytes written.  Returns
   when every byte is in place.  Every argument is checked before the first byte moves (AKZ_ERR_INVALID_ARG: null
   result, img out of range, dst NULL, n_dst != n_levels * 10; nothing is written then).
   Thread rules of akz_fetch_plane: call it from the thread that uses the result's context, never while another call
   on that context runs.  A job of the context that is begun and not yet finished is not disturbed. */
int akz_fetch_pyramid(const akz_result* res, uint64_t img, float* const* dst, uint64_t n_dst,
                      uint64_t* bytes_out);
/* device address of a resident plane (NULL if not kept) */
int akz_result_device_plane(const akz_result* res, uint64_t img, uint64_t level, akz_plane plane,
                            const float** d_plane);

/* ---- the hot path: match_features (descriptor part) ---------------------------------- */
/* ops::feature_matching::descriptor_match — akaze/src/ops/feature_matching.rs:23-94.
   d0: n0 x desc_bytes, d1: n1 x desc_bytes (host, unpadded).  out must hold n0 entries. */
int akz_descriptor_match(akz_ctx* ctx, const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1,
                         uint64_t desc_bytes, uint64_t distance_threshold, double lowes_ratio, akz_match* out,
                         uint64_t* n_out);
/* same on device-resident 64-byte descriptor rows (what akz_result_device_descriptors and the
   RCCL gather produce: an M-LDB descriptor has at most 61 bytes, bytes 61..63 of a row are padding
   and are NOT compared).  d_out: n0 akz_match records on the device, compacted in index_0
   order; *d_n_out (device uint64) receives the count. */
int akz_descriptor_match_device(akz_ctx* ctx, const uint8_t* d_d0, uint64_t n0, const uint8_t* d_d1, uint64_t n1,
                                uint64_t distance_threshold, double lowes_ratio, akz_match* d_out,
                                uint64_t* d_n_out);
/* One query set against n_sets train sets in one launch (all-pairs matching, BASELINE configs[4]): d_train
   holds the sets' 64-byte rows one after the other, set_rows[k] (host) the number of rows of set k.
   Results of set k: matches at d_out + k * n0 (room for n0 each), count at d_n_out[k] (device uint64),
   index_1 relative to the set — exactly what n_sets calls of akz_descriptor_match_device return, at the
   rate of one large product. */
int akz_descriptor_match_sets_device(akz_ctx* ctx, const uint8_t* d_q, uint64_t n0, const uint8_t* d_train,
                                     const uint64_t* set_rows, uint64_t n_sets, uint64_t distance_threshold,
                                     double lowes_ratio, akz_match* d_out, uint64_t* d_n_out);
/* The same launch with the OPPOSITE direction riding along: hamming(a, b) = hamming(b, a), so one pass over the distances of
   a (query set, train set k) block yields both descriptor_match(query set, set k) -- rows as above -- and
   descriptor_match(set k, query set) (feature_matching.rs:23-94 with the arguments exchanged: index_0 a row of set k,
   index_1 a row of the query set, lowest index among equal minima): its matches go to d_out_cols + (number of rows of the
   sets before k) (room for set_rows[k]), its count to d_n_cols[k] (device uint64).  Identical to 2 * n_sets calls of
   akz_descriptor_match_device at the matrix-core work of n_sets.  (On the FP4 matcher, the default; the other matcher
   kernels compute the second direction separately.) */
int akz_descriptor_match_sets_mutual_device(akz_ctx* ctx, const uint8_t* d_q, uint64_t n0, const uint8_t* d_train,
                                            const uint64_t* set_rows, uint64_t n_sets, uint64_t distance_threshold,
                                            double lowes_ratio, akz_match* d_out, uint64_t* d_n_out, akz_match* d_out_cols,
                                            uint64_t* d_n_cols);

/* ---- multi-GPU: the path's one exchange step ----------------------- */
/* extract_features has no cross-image state (akaze/src/lib.rs:167-194): images are sharded one per GPU slot and
   extraction needs no collective.  Before a cross-image brute-force match (feature_matching.rs:23-94 across shards)
   the 64-byte descriptor rows of every rank are all-gathered over RCCL (xGMI).  The reference is a single-process CPU
   crate and has no counterpart.  RCCL is loaded at run time (librccl.so.1); without it these calls return
   AKZ_ERR_UNSUPPORTED and nothing else in the library is affected.
   One process per GPU: rank 0 creates the id and hands its AKZ_COMM_ID_BYTES bytes to every rank by any means (a
   file, MPI, torch.distributed); every rank then calls akz_comm_create (collective). */
#define AKZ_COMM_ID_BYTES 128
typedef struct akz_comm akz_comm;
typedef struct akz_gather akz_gather; /* one exchange in flight */
int akz_comm_unique_id(uint8_t* id_out /* AKZ_COMM_ID_BYTES */);
int akz_comm_create(int device, const uint8_t* id, int rank, int nranks, akz_comm** out);
/* The same communicator with the transport left to the CALLER (MPI, gloo, shared memory; a rehearsal of several ranks on
   ONE GPU, which RCCL refuses): RCCL is not loaded, no id is needed, the call is not collective.  An exchange is then
       akz_gather_begin / akz_gather_begin_rows  -> this rank's block is complete in device memory on return
       akz_gather_blocks(g, &d_send, &d_recv, &bytes)  -> move every rank r's d_send block to d_recv + r * bytes on every
                                                          rank (this rank's own block included)
       akz_gather_deliver(g, stream)                   -> the blocks are complete in the order of `stream` (NULL: now)
   and everything behind it (akz_gather_finish, akz_gather_stream_wait, akz_match_all_pairs, ...) as with RCCL.  The wire
   format is the one described below; akz_gather_descriptors (the synchronous two-collective form) is not available. */
int akz_comm_create_external(int device, int rank, int nranks, akz_comm** out);
/* device = AKZ_COMM_HOST: the same object with its blocks (and the caller's descriptor rows) in HOST memory -- no GPU call is
   made by any akz_comm_* / akz_gather_* function on it.  It serves the wire format, the overflow protocol and the all-pairs
   plan (akz_pairs_plan) to hosts that stage descriptors in host memory and to CPU-only rehearsals of the multi-rank job
   (tests/test_distributed.py under gloo); rows come in through akz_gather_begin_rows / akz_gather_begin_image_rows as host
   pointers, akz_gather_blocks returns host pointers, akz_gather_begin and akz_match_all_pairs (device work) are
   AKZ_ERR_UNSUPPORTED. */
#define AKZ_COMM_HOST (-1)
int akz_comm_destroy(akz_comm* comm);
/* How long akz_gather_finish (and what calls it: akz_gather_descriptors, akz_match_all_pairs) waits for an exchange before
   it gives up with AKZ_ERR_TIMEOUT -- a peer that crashed or never joined leaves a collective waiting for ever, and a host
   that can report that is worth more than one that hangs.  0 (default): wait without limit.  After a timeout the
   communicator is ABANDONED: the stuck collective still sits on its stream, so nothing waits for that stream any more --
   akz_gather_free and akz_comm_destroy return at once and leak the device buffers, streams and the RCCL communicator (freeing
   them would wait for the collective), new exchanges are refused with AKZ_ERR_TIMEOUT.  (An exchange that was only slow: a
   later akz_gather_finish of the same gather -- after a longer akz_comm_set_timeout, or 0 -- that sees it complete puts the
   communicator back in service.)  The host is expected to report the
   error and end the process with a non-zero status WITHOUT running the GPU runtime's exit handlers (`_exit` / `os._exit`:
   they, too, may wait for the stuck stream). */
int akz_comm_set_timeout(akz_comm* comm, double seconds);
/* Optional, once, with idle streams (before the first step): moves the communicator's two streams onto hardware queues and
   command-processor pipes that `ctx`'s busy streams (the caller's, the coarse chain's, the finish half's) do not use -- the
   collective of a step runs beside the next batch's kernels, and two busy streams on one queue or pipe slow both (see
   akz_ctx / INTEGRATION.md, threading).  Triggers the context's own stream-placement probe if it has not run. */
int akz_comm_place_streams(akz_comm* comm, akz_ctx* ctx);
int akz_comm_info(const akz_comm* comm, int* rank, int* nranks);
/* Appendix C form, synchronous: every rank contributes n_local rows (device, 64 bytes each, as returned by
   akz_result_device_descriptors); on return *d_all points at the rows of all ranks in rank order (device memory owned
   by the communicator, valid until the next call) and counts[r] is rank r's row count (host, nranks entries). */
int akz_gather_descriptors(akz_comm* comm, const uint8_t* d_local, uint64_t n_local, const uint8_t** d_all,
                           uint64_t* counts /* nranks */);
/* Pipelined form: ONE fixed-size all-gather per call, enqueued on the communicator's own streams without touching
   the extraction stream.  Every rank contributes a block of 1 + cap_rows rows: a header row {u64 rows, u64 images,
   u64 cap_rows, u64 sequence, u64 overflow, u64 table rows, 0, 0} followed by the descriptor rows of all images of all
   `results` (in order) and, for akz_gather_begin, a table of the rows per image (eight u64 per row; it counts against
   cap_rows: allow one row per eight images);
   cap_rows MUST be the same on every rank (the message sizes of the collective depend on it: a mismatch is fatal
   for the communicator and cannot be detected before the collective is issued) and should be at least the largest
   shard.  A rank whose shard does not fit still takes part — it sends its header alone, marked — and
   akz_gather_finish then returns AKZ_ERR_BUFFER on EVERY rank, with counts[] holding what each rank needed, so that
   all ranks can repeat the exchange with the same larger capacity; the communicator stays usable.
   akz_gather_begin returns as soon as the local rows have been copied — the results may be freed, the next batch
   begun — and never waits for a collective; akz_gather_begin_rows takes raw device rows that are complete in the
   order of producer_stream (may be NULL: complete now) and must stay valid until the gather is finished. */
int akz_gather_begin(akz_comm* comm, const akz_result* const* results, uint64_t n_results, uint64_t cap_rows,
                     akz_gather** out);
int akz_gather_begin_rows(akz_comm* comm, const uint8_t* d_local, uint64_t n_local, uint64_t cap_rows,
                          void* producer_stream, akz_gather** out);
/* external transport only (akz_comm_create_external): the block this rank sends, where the blocks of all ranks go, bytes per block */
int akz_gather_blocks(akz_gather* g, const uint8_t** d_send, uint8_t** d_recv, uint64_t* block_bytes);
int akz_gather_deliver(akz_gather* g, void* stream);
/* make `stream` (e.g. the matcher's) wait for the gathered blocks without a host synchronisation */
int akz_gather_stream_wait(akz_gather* g, void* stream);
/* host wait.  *d_all: nranks blocks of *block_rows (= 1 + cap_rows) rows, rank r's descriptor rows start one row into
   block r; counts / images (host, nranks entries, may be NULL) are read from the headers.  Rows beyond a rank's count
   are unspecified. */
int akz_gather_finish(akz_gather* g, const uint8_t** d_all, uint64_t* block_rows, uint64_t* counts, uint64_t* images);
/* rows of every image of rank `rank`'s shard, in its shard order (host, after akz_gather_finish): a block carries them
   behind its descriptor rows, eight u64 per row (akz_gather_begin_rows sends its rows as ONE image).  *n_images = the
   rank's image count; rows_per_image receives min(cap, *n_images) entries. */
int akz_gather_image_rows(akz_gather* g, int rank, uint64_t* rows_per_image, uint64_t cap, uint64_t* n_images);
/* hand the blocks back to the communicator (waits for the collective if it is still running) */
int akz_gather_free(akz_gather* g);
/* akz_gather_begin_rows for the rows of SEVERAL images held by the caller (device memory, or host memory on an
   AKZ_COMM_HOST communicator): n_images images back to back, rows_per_image[i] rows each; the per-image table travels
   behind the rows exactly as with akz_gather_begin. */
int akz_gather_begin_image_rows(akz_comm* comm, const uint8_t* d_local, const uint64_t* rows_per_image, uint64_t n_images,
                                uint64_t cap_rows, void* producer_stream, akz_gather** out);

/* BASELINE configs[4] — the cross-GPU all-pairs match for hosts that are not Python: after an
   exchange every rank holds the descriptor rows of every image of the job (numbered rank-major).  Every UNORDERED image
   pair {a, b} is matched once, in both directions, by the rank that owns the pair's lead image (lo if hi - lo is odd,
   else hi: every image leads about half of its pairs): the lead image is the query set of one both-direction launch
   (akz_descriptor_match_sets_mutual_device) against the images it leads, so the matrix-core work of a block serves
   descriptor_match(a, b) and descriptor_match(b, a) (ops::feature_matching::descriptor_match, feature_matching.rs:23-94;
   every list identical to akz_descriptor_match of the pair).  The call enqueues on the context's stream and returns; it
   allocates only when the job grows (buffers are pooled in the communicator) and finishes the gather if the caller has
   not; the gather may be freed afterwards (a later exchange that reuses its buffers is ordered behind this call's copies). */
typedef struct akz_pairs akz_pairs;
int akz_match_all_pairs(akz_ctx* ctx, akz_gather* gather, uint64_t distance_threshold, double lowes_ratio, akz_pairs** out);
/* The PLAN of akz_match_all_pairs without the match: finishes the gather and returns an akz_pairs that answers
   akz_pairs_info / _image_rows / _holder / _lead_sets / _totals (lists and distances this rank would compute; no matches) --
   host arithmetic only, also on an AKZ_COMM_HOST communicator.  akz_pairs_matches on it is an error. */
int akz_pairs_plan(akz_gather* gather, akz_pairs** out);
/* the images that `lead_image` (one this rank owns) is matched against by this rank, ascending: with akz_pairs_holder
   these say who computes every unordered pair of the job */
int akz_pairs_lead_sets(const akz_pairs* p, uint64_t lead_image, uint64_t* images, uint64_t cap, uint64_t* n);
/* *n_images: images of the whole job; this rank's are first_owned .. first_owned + n_owned - 1 */
int akz_pairs_info(const akz_pairs* p, uint64_t* n_images, uint64_t* first_owned, uint64_t* n_owned);
int akz_pairs_image_rows(const akz_pairs* p, uint64_t image, uint64_t* rows, int* owner_rank);
/* the rank whose akz_pairs holds both lists of the pair {image_a, image_b} (the owner of its lead image) */
int akz_pairs_holder(const akz_pairs* p, uint64_t image_a, uint64_t image_b, int* rank);
/* descriptor_match(query, image) for a pair this rank holds (akz_pairs_holder; either image may be the query): index_0
   into the query's rows, index_1 into `image`'s; ordered by index_0.  out may be NULL (count only); at most cap records are
   written.  The pair (query, query) is empty.  The first call waits for the launches of akz_match_all_pairs. */
int akz_pairs_matches(const akz_pairs* p, uint64_t query, uint64_t image, akz_match* out, uint64_t cap, uint64_t* n);
/* Everything this rank holds at once (waits for the launches like the first akz_pairs_matches): *n_lists = match lists held
   (two per unordered pair it leads), *n_matches = their records in all, *n_distances = descriptor pairs whose distance was
   formed (rows(a) x rows(b) per unordered pair; each serves both directions).  Any pointer may be NULL. */
int akz_pairs_totals(const akz_pairs* p, uint64_t* n_lists, uint64_t* n_matches, uint64_t* n_distances);
/* Lifetime: an akz_pairs may be freed before or after akz_comm_destroy of the communicator it came from (the communicator
   keeps a list of the objects it has handed out and cuts them loose when it is destroyed; until then a freed object's
   buffers are pooled there, at most two of them).  It must be freed before akz_ctx_destroy of the context it ran on. */
int akz_pairs_free(akz_pairs* p);

/* ---- the rest of match_features (host post-filter) -------------------- */
/* ops::estimate_fundamental_matrix::remove_outliers — estimate_fundamental_matrix.rs:99-165: 8-point
   fundamental matrix + RANSAC over the matches; fewer than 8 matches are returned unchanged.  Host code.
   The reference's own output is not reproducible (HashSet order, `random` crate), so this is a
   behavioural restatement, not a parity target.  out must hold n_matches entries. */
int akz_remove_outliers(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                        const akz_match* matches, uint64_t n_matches, uint64_t num_trials, float epsilon_model,
                        float epsilon_inlier, akz_match* out, uint64_t* n_out);
/* ops::estimate_fundamental_matrix::estimate_fundamental_matrix — estimate_fundamental_matrix.rs:17-69: the 8-point
   model of exactly 8 matches; *found = 0 where the reference returns None (fewer than 8 singular values above
   epsilon); f receives the 3x3 matrix row by row. */
int akz_estimate_fundamental_matrix(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1,
                                    uint64_t n1, const akz_match* matches8, float epsilon, float* f /* 9 */, int* found);
/* akaze::match_features — akaze/src/lib.rs:252-275: descriptor_match(d0, d1, 10000, lowes_ratio) on the
   GPU, then remove_outliers(kp0, kp1, matches, ransac_trials, 0.05, ransac_epsilon_inliers): samples, winner and final
   filter on the host, the trials' models and inlier counts on the device (the host's arithmetic, bit for bit).
   Descriptors are host arrays of n_descriptors x desc_bytes (both sets the same desc_bytes); keypoints and
   descriptors of a set are counted separately, as the reference's slices are — a set with more descriptors than
   keypoints is AKZ_ERR_INVALID_ARG (the reference panics once such a match reaches RANSAC).  out must hold
   n_descriptors_0 entries. */
int akz_match_features(akz_ctx* ctx, const akz_keypoint* keypoints_0, uint64_t n_keypoints_0, const uint8_t* descriptors_0,
                       uint64_t n_descriptors_0, const akz_keypoint* keypoints_1, uint64_t n_keypoints_1,
                       const uint8_t* descriptors_1, uint64_t n_descriptors_1, uint64_t desc_bytes, double lowes_ratio,
                       uint64_t ransac_trials, float ransac_epsilon_inliers, akz_match* out, uint64_t* n_out);
/* A feature set of akz_match_features_pairs: host keypoints and host descriptors (n_descriptors x desc_bytes, unpadded). */
typedef struct akz_feature_set {
    const akz_keypoint* keypoints;
    uint64_t n_keypoints;
    const uint8_t* descriptors;
    uint64_t n_descriptors;
} akz_feature_set;
/* akz_match_features over many pairs in one call (a loop of akaze/src/lib.rs:252-275).  pairs: 2 x n_pairs set indices,
   (first, second) per pair; pairs may repeat, be reversed or be (a, a).
   * Same result as the loop: pair p's list is what akz_match_features(sets[a], sets[b], desc_bytes, lowes_ratio,
     ransac_trials, ransac_epsilon_inliers) returns when it is called for p = 0, 1, ... in order on the calling thread, from
     the same state of that thread's random source, bit for bit; afterwards the source is in the state that loop leaves it in.
   * Output: pair p's list starts at out + sum_{q<p} sets[pairs[2q]].n_descriptors, its length goes to n_out[p]; out must
     hold sum_p sets[pairs[2p]].n_descriptors entries (fixed room per pair: a call never needs a retry).
   * Refusals (AKZ_ERR_INVALID_ARG, the message names the pair or set) all come before the first random draw and before any
     GPU work, and then nothing is written and the random source is untouched: every refusal akz_match_features makes for
     a pair (a set with more descriptors than keypoints, desc_bytes outside 1..64, null pointers), a set index >= n_sets,
     a null ctx while n_pairs > 0.  n_pairs = 0 is AKZ_OK.
   * No new limits: every argument akz_match_features accepts; pairs with fewer than 8 matches are returned unchanged and draw
     nothing; ransac_trials = 0 gives the zero model (every match kept if epsilon > 0).  desc_bytes 62..64 compare every byte
     of a row, as akz_descriptor_match does.
   * Work runs on the context's stream with the context's scratch; the call returns synchronously.  What may run on the
     context at the same time is the same as for akz_match_features.
   Each distinct set is uploaded once; the descriptor scans, the keypoint gather, the trials of all pairs, the choice of
   each winner and the final filter run on the GPU; the samples are drawn on the calling thread in pair order. */
int akz_match_features_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                             uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                             float ransac_epsilon_inliers, akz_match* out, uint64_t* n_out /* n_pairs */);

/* ---- homography RANSAC (an addition: the reference filters with the fundamental matrix only) --------------------------
   For planar scenes and pure rotations, where F is not determined.  Model: the 4-point DLT with Hartley normalisation,
   decomposed by the one-sided Jacobi SVD of the fundamental-matrix path, in f64 with one source for host and device (same
   bits).  Samples whose normalised points are collinear in either image (|cross product| <= 1e-9, two equal points
   included) or whose triples change orientation between the images give no model.  H is row-major with H[8] = 1 (it maps
   image 0 onto image 1); a match is an inlier iff w = h6 x0 + h7 y0 + h8 > 0 and |H p0 - p1| < epsilon_inlier, evaluated
   without a division as (U - x1 w)^2 + (V - y1 w)^2 < (epsilon_inlier w)^2 in f32.  The returned H is the winning trial's
   model; akz_refine_homography and the _refined calls below refit it on its inliers.  Samples come from the calling thread's default random source, 4 per trial (see
   akz_random_seed).  DESIGN.md 8. */
/* epsilon_model of the two context calls: every rotated row norm of the normalised 8 x 9 design matrix must exceed it */
#define AKZ_HOMOGRAPHY_EPSILON_MODEL 1e-6f
/* The model of exactly 4 matches: *found = 0 for a degenerate sample or a rank below 8 at epsilon; h receives H. */
int akz_estimate_homography(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                            const akz_match* matches4, float epsilon, float* h /* 9 */, int* found);
/* The host RANSAC (akz_remove_outliers with the homography): fewer than 4 matches are returned unchanged with *found = 0 and
   nothing drawn; no trial with a model of more than 0 inliers: every match kept, *found = 0; otherwise *found = 1, h = the
   winner (the first trial with the most inliers) and its inliers in match order.  out must hold n_matches entries; h and
   found may be NULL. */
int akz_remove_outliers_homography(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                   const akz_match* matches, uint64_t n_matches, uint64_t num_trials, float epsilon_model,
                                   float epsilon_inlier, akz_match* out, uint64_t* n_out, float* h /* 9, may be NULL */,
                                   int* found /* may be NULL */);
/* descriptor_match(d0, d1, 10000, lowes_ratio) on the GPU, then the homography RANSAC with AKZ_HOMOGRAPHY_EPSILON_MODEL, its
   trials, the winner and the final filter on the GPU: the result of akz_remove_outliers_homography on that list from the
   same random state, bit for bit (list, H, found, the source's state afterwards).  Arguments and refusals are those of
   akz_match_features; h (9) and found may be NULL. */
int akz_match_features_homography(akz_ctx* ctx, const akz_keypoint* keypoints_0, uint64_t n_keypoints_0,
                                  const uint8_t* descriptors_0, uint64_t n_descriptors_0, const akz_keypoint* keypoints_1,
                                  uint64_t n_keypoints_1, const uint8_t* descriptors_1, uint64_t n_descriptors_1,
                                  uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers,
                                  akz_match* out, uint64_t* n_out, float* h /* 9 */, int* found);
/* akz_match_features_homography over many pairs, with every promise of akz_match_features_pairs (the loop's lists in pair
   order from the same random state, the source left where the loop leaves it, all refusals before the first draw and any
   GPU work, fixed room per pair in out).  h: 9 floats per pair (zeros where found is 0), found: one flag per pair; either
   may be NULL. */
int akz_match_features_homography_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                        uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                        float ransac_epsilon_inliers, akz_match* out, uint64_t* n_out /* n_pairs */,
                                        float* h /* 9 x n_pairs */, int* found /* n_pairs */);

/* ---- guided matching (an addition: the reference matches a pair once, blind) -----------------------------------------
   descriptor_match (feature_matching.rs:37-81) repeated once a model of the pair is known: a train row j competes for a
   query i only if it lies within `radius` pixels of where the model sends keypoint i -- minimum, second minimum, the lowest
   index among equal minima, ratio and threshold are taken over those rows alone.  The ratio test of the blind scan compares
   with the second best of the WHOLE other image, which repeated structure fails although the geometry leaves one candidate.
   model_kind AKZ_GUIDED_HOMOGRAPHY: model = H, row-major, image 0 onto image 1; the gate is the inlier test of the
   homography RANSAC above, w > 0 and (U - x1 w)^2 + (V - y1 w)^2 < (radius w)^2 in f32 in that order.
   model_kind AKZ_GUIDED_FUNDAMENTAL: model = F, row-major, with p1^T F p0 = 0 (the convention of
   akz_estimate_fundamental_matrix); the gate is the distance of (x1, y1) to the epipolar line of (x0, y0) in PIXELS --
   l_r = (f[3r] x0 + f[3r+1] y0) + f[3r+2], n = l0 l0 + l1 l1, s = (l0 x1 + l1 y1) + l2, passes iff s s < (radius radius) n,
   in f32 in that order -- and not the algebraic |p1^T F p0| < epsilon of akz_remove_outliers.
   Both comparisons are strict: radius 0, F = 0 or a NaN pass nothing.  Model entries are not checked.  Host and GPU form
   the gate from one source without contraction: the same bits.
   Only x and y of the first n_descriptors keypoints of a set are read.  Both distances start at distance_threshold (values
   above 2^31 - 1 count as that); a query is kept iff (double)min < (double)second * lowes_ratio^2 and min < threshold; the
   list is in index_0 order, index_1 indexes the whole second set.  Every byte of a row is compared (desc_bytes 1..64).
   Refusals (AKZ_ERR_INVALID_ARG, before any GPU work, nothing written): those of akz_match_features(_pairs), a model_kind
   other than these two, a NULL model, a radius that is negative or not finite.  n_pairs = 0 and empty sets are AKZ_OK. */
#define AKZ_GUIDED_HOMOGRAPHY 0
#define AKZ_GUIDED_FUNDAMENTAL 1
/* The plain host statement (no GPU call): the loop of feature_matching.rs with the gate at the top of the inner loop. */
int akz_descriptor_match_guided_host(const akz_keypoint* keypoints_0, uint64_t n_keypoints_0, const uint8_t* descriptors_0,
                                     uint64_t n_descriptors_0, const akz_keypoint* keypoints_1, uint64_t n_keypoints_1,
                                     const uint8_t* descriptors_1, uint64_t n_descriptors_1, uint64_t desc_bytes, int model_kind,
                                     const float* model /* 9 */, float radius, uint64_t distance_threshold, double lowes_ratio,
                                     akz_match* out /* n_descriptors_0 */, uint64_t* n_out);
/* The same list from the GPU (the pairs call below with one pair). */
int akz_descriptor_match_guided(akz_ctx* ctx, const akz_keypoint* keypoints_0, uint64_t n_keypoints_0, const uint8_t* descriptors_0,
                                uint64_t n_descriptors_0, const akz_keypoint* keypoints_1, uint64_t n_keypoints_1,
                                const uint8_t* descriptors_1, uint64_t n_descriptors_1, uint64_t desc_bytes, int model_kind,
                                const float* model /* 9 */, float radius, uint64_t distance_threshold, double lowes_ratio,
                                akz_match* out /* n_descriptors_0 */, uint64_t* n_out);
/* Many pairs in one call, each with its own model (models + 9 p); sets, pairs, the layout of out and the room per pair are
   those of akz_match_features_pairs.  Each distinct set is uploaded once, all pairs are scanned by one launch; pair p's list
   is what akz_descriptor_match_guided returns for that pair, bit for bit. */
int akz_descriptor_match_guided_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                      uint64_t n_pairs, uint64_t desc_bytes, int model_kind, const float* models /* 9 x n_pairs */,
                                      float radius, uint64_t distance_threshold, double lowes_ratio, akz_match* out,
                                      uint64_t* n_out /* n_pairs */);
/* akz_match_features_homography(_pairs) followed by the guided scan with the H it found: per pair exactly what the
   homography call does (same draws, same H, same found); where found = 1 the returned list is
   akz_descriptor_match_guided(pair, AKZ_GUIDED_HOMOGRAPHY, H, guided_radius, 10000, guided_lowes_ratio), where found = 0 it
   is the homography call's list unchanged.  H stays on the device between the two stages and the sets are uploaded once.
   With guided_radius = ransac_epsilon_inliers and guided_lowes_ratio = lowes_ratio the guided list contains every match the
   homography call keeps (same index_1, same distance). */
int akz_match_features_homography_guided(akz_ctx* ctx, const akz_keypoint* keypoints_0, uint64_t n_keypoints_0,
                                         const uint8_t* descriptors_0, uint64_t n_descriptors_0, const akz_keypoint* keypoints_1,
                                         uint64_t n_keypoints_1, const uint8_t* descriptors_1, uint64_t n_descriptors_1,
                                         uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                         float ransac_epsilon_inliers, float guided_radius, double guided_lowes_ratio,
                                         akz_match* out, uint64_t* n_out, float* h /* 9 */, int* found);
int akz_match_features_homography_guided_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                               uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                               float ransac_epsilon_inliers, float guided_radius, double guided_lowes_ratio,
                                               akz_match* out, uint64_t* n_out /* n_pairs */, float* h /* 9 x n_pairs */,
                                               int* found /* n_pairs */);

/* ---- the refit of the RANSAC homography on its inliers (an addition) -------------------------------------
   Local optimisation of a homography over a pair's RAW match list (the ratio-test list, so the set can grow):
       S = { i : inlier(h, i, epsilon_inlier) }  (the inlier test above);  done = 0
       while done < max_iterations:
           h' = fit(S)            no model: stop
           S' = inliers(h')
           |S'| < |S|: stop       h' is rejected
           grew = |S'| > |S|;  h, S = h', S';  done += 1
           not grew: stop
   The result never has fewer inliers than the input.  fit(S) for |S| >= 4 is the least-squares DLT over all of S: Hartley
   normalisation of both images (centroid, mean distance d, s = sqrt(2) / d; d = 0: no model), the normal matrix M = A^T A
   of the design rows of the 4-point model in normalised coordinates, its null vector by the one-sided Jacobi sweeps on the
   9 rows of M (the row of the smallest norm dropped; every kept norm above AKZ_HOMOGRAPHY_EPSILON_MODEL^2 |S| / 4, else no
   model), then the denormalisation, the H[8] rule and the rounding of the 4-point model.  All of it in f64 in one order,
   every sum over S by lanes (element i in lane i mod 256, ascending, from +0.0) and the tree p[l] += p[l + s],
   s = 128 .. 1: host and GPU give the same bits.
   akz_refine_homography is the plain host statement (no GPU call).  out must hold n_matches entries; it receives S in
   match order, h_out (9, may be NULL) the final h, *iterations (may be NULL) the number of accepted fits; with 0 accepted
   fits that is h_in unchanged and its inliers.  Refusals: those of akz_remove_outliers_homography, a NULL h_in, an
   epsilon_inlier that is not finite or <= 0. */
int akz_refine_homography(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                          const akz_match* matches, uint64_t n_matches, const float* h_in /* 9 */, float epsilon_inlier,
                          uint32_t max_iterations, akz_match* out, uint64_t* n_out, float* h_out /* 9, may be NULL */,
                          uint32_t* iterations /* may be NULL */);
/* akz_match_features_homography(_pairs) with the refit as one more stage on the GPU: draws, winner and found are exactly the
   unrefined call's and the random source ends where that call leaves it; where found = 1 the list and H are those of
   akz_refine_homography(raw list, winner, ransac_epsilon_inliers, refine_iterations); where found = 0 or a pair has fewer
   than 4 matches the list is the unrefined call's and iterations is 0.  refine_iterations = 0 is the unrefined call bit for
   bit.  iterations: one per pair, may be NULL.  Refusals are the unrefined call's, before the first draw and any GPU work. */
int akz_match_features_homography_refined(akz_ctx* ctx, const akz_keypoint* keypoints_0, uint64_t n_keypoints_0,
                                          const uint8_t* descriptors_0, uint64_t n_descriptors_0, const akz_keypoint* keypoints_1,
                                          uint64_t n_keypoints_1, const uint8_t* descriptors_1, uint64_t n_descriptors_1,
                                          uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                          float ransac_epsilon_inliers, uint32_t refine_iterations, akz_match* out, uint64_t* n_out,
                                          float* h /* 9 */, int* found, uint32_t* iterations);
int akz_match_features_homography_refined_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                                uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                                float ransac_epsilon_inliers, uint32_t refine_iterations, akz_match* out,
                                                uint64_t* n_out /* n_pairs */, float* h /* 9 x n_pairs */, int* found /* n_pairs */,
                                                uint32_t* iterations /* n_pairs */);
/* The refined call followed by the guided stage of akz_match_features_homography_guided(_pairs), gating with the REFINED H. */
int akz_match_features_homography_refined_guided(akz_ctx* ctx, const akz_keypoint* keypoints_0, uint64_t n_keypoints_0,
                                                 const uint8_t* descriptors_0, uint64_t n_descriptors_0,
                                                 const akz_keypoint* keypoints_1, uint64_t n_keypoints_1,
                                                 const uint8_t* descriptors_1, uint64_t n_descriptors_1, uint64_t desc_bytes,
                                                 double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers,
                                                 uint32_t refine_iterations, float guided_radius, double guided_lowes_ratio,
                                                 akz_match* out, uint64_t* n_out, float* h /* 9 */, int* found, uint32_t* iterations);
int akz_match_features_homography_refined_guided_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets,
                                                       const uint64_t* pairs, uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio,
                                                       uint64_t ransac_trials, float ransac_epsilon_inliers, uint32_t refine_iterations,
                                                       float guided_radius, double guided_lowes_ratio, akz_match* out,
                                                       uint64_t* n_out /* n_pairs */, float* h /* 9 x n_pairs */,
                                                       int* found /* n_pairs */, uint32_t* iterations /* n_pairs */);

/* ---- the RANSAC fundamental matrix handed back, refitted on its inliers, and guiding (an addition) ---------
   akz_remove_outliers, akz_match_features and akz_match_features_pairs return a list only, as the reference does.  The calls
   below run the same RANSAC -- the same draws from the calling thread's random source, the same list bit for bit -- and also
   hand back the model that filtered: f, row-major, with p1^T F p0 = 0 as in akz_estimate_fundamental_matrix, the winner (the
   first trial with the most inliers); found = 1 iff some trial had a model with more than 0 inliers.  Without a winner the
   list is still what akz_remove_outliers returns (the zero model is evaluated), f is zeros and found is 0.  Fewer than 8
   matches: the list is unchanged, f is zeros, found is 0 and nothing is drawn.  f and found may be NULL.
   akz_remove_outliers_fundamental is the plain host statement (no GPU call; refusals of akz_remove_outliers). */
int akz_remove_outliers_fundamental(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                    const akz_match* matches, uint64_t n_matches, uint64_t num_trials, float epsilon_model,
                                    float epsilon_inlier, akz_match* out, uint64_t* n_out, float* f /* 9, may be NULL */,
                                    int* found /* may be NULL */);
/* akz_match_features(_pairs) with the model: descriptor_match(d0, d1, 10000, lowes_ratio), then the RANSAC with the reference's
   epsilon_model 0.05, all on the GPU but the draws; equal to akz_remove_outliers_fundamental on that raw list from the same
   random state -- list, F bits, found, and the state of the random source afterwards.  f: 9 floats per pair (zeros where found
   is 0), found: one flag per pair; either may be NULL.  Refusals, the layout of out and every other promise are those of
   akz_match_features_pairs. */
int akz_match_features_fundamental(akz_ctx* ctx, const akz_keypoint* keypoints_0, uint64_t n_keypoints_0,
                                   const uint8_t* descriptors_0, uint64_t n_descriptors_0, const akz_keypoint* keypoints_1,
                                   uint64_t n_keypoints_1, const uint8_t* descriptors_1, uint64_t n_descriptors_1,
                                   uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers,
                                   akz_match* out, uint64_t* n_out, float* f /* 9 */, int* found);
int akz_match_features_fundamental_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                         uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                         float ransac_epsilon_inliers, akz_match* out, uint64_t* n_out /* n_pairs */,
                                         float* f /* 9 x n_pairs */, int* found /* n_pairs */);
/* The refit.  The winner of the RANSAC is the model of ONE 8-point sample in raw pixel coordinates: it is not of rank 2 and it
   is as noisy as its eight points.  akz_refine_fundamental_matrix runs the loop of akz_refine_homography, unchanged, over a
   pair's RAW match list with the inlier rule of the RANSAC itself, |p1^T F p0| < epsilon_inlier in f32 in the order of
   akz_remove_outliers -- so the result never has fewer inliers than the input.  fit(S) for |S| >= 8 (fewer: no model), in f64
   in one order, every sum over S by lanes and the tree as for the homography:
     1. Hartley normalisation of both images as for the homography (a mean distance of 0: no model);
     2. with p = (x, y, 1), q = (u, v, 1) normalised, a = {x x, x y, x, y y, y, 1} and b the same six products of q, the 36 sums
        of a[k] b[l]: the normal matrix M = A^T A of the design rows of the 8-point model (entry 3 i + j is p_i q_j),
        M[3 i + j][3 k + l] = sum p_i p_k q_j q_l;
     3. the null vector by the one-sided Jacobi sweeps on the 9 rows of M: the row of the smallest norm (the first among
        equals), normalised; every other row norm must exceed AKZ_FUNDAMENTAL_REFIT_EPSILON^2 |S| / 8, else no model;
     4. rank 2: the same rotations on the three rows of F^; with r the row of the smallest norm afterwards and v3 = r / |r|
        (|r| = 0: nothing to remove), F' = F^ - (F^ v3) v3^T;
     5. F = T1^T F' T0, scaled to unit Frobenius norm -- the trial models have it, and epsilon_inlier only means anything at
        that scale -- and rounded to f32; a norm that is zero or not finite: no model.
   out must hold n_matches entries; it receives S in match order, f_out (9, may be NULL) the final f, *iterations (may be NULL)
   the number of accepted fits; with 0 accepted fits that is f_in unchanged and its inliers.  Refusals are those of
   akz_refine_homography (a NULL f_in, an epsilon_inlier that is not finite or <= 0, an index past a keypoint array, ...);
   nothing is written after one. */
#define AKZ_FUNDAMENTAL_REFIT_EPSILON 1e-6f
int akz_refine_fundamental_matrix(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                  const akz_match* matches, uint64_t n_matches, const float* f_in /* 9 */, float epsilon_inlier,
                                  uint32_t max_iterations, akz_match* out, uint64_t* n_out, float* f_out /* 9, may be NULL */,
                                  uint32_t* iterations /* may be NULL */);
/* akz_match_features_fundamental(_pairs) with the refit and / or the guided scan as further stages on the GPU, with the
   arguments and promises of the homography family above.  Draws, winner and found are exactly the unrefined call's and the
   random source ends where that call leaves it.  _refined: where found = 1 the list and F are those of
   akz_refine_fundamental_matrix(raw list, winner, ransac_epsilon_inliers, refine_iterations); refine_iterations = 0 is the
   unrefined call bit for bit.  _guided: where found = 1 the returned list is akz_descriptor_match_guided(pair,
   AKZ_GUIDED_FUNDAMENTAL, F, guided_radius, 10000, guided_lowes_ratio) -- with the REFINED F in the _refined_guided forms; F
   stays on the device between the stages and the sets are uploaded once.  Where found = 0 or a pair has fewer than 8
   matches the list is the unrefined call's, iterations is 0 and the guided stage is skipped.
   There is NO superset promise here, unlike the homography's guided call: the guided gate is a distance to the epipolar
   line in pixels, the RANSAC's rule is the algebraic |p1^T F p0| -- a match the RANSAC keeps can lie outside the band, and
   the other way round.  iterations: one per pair, may be NULL.  Refusals are the unrefined call's (and the guided call's
   radius rule), before the first draw and any GPU work.  So a ransac_epsilon_inliers that akz_refine_fundamental_matrix
   refuses (not finite, or <= 0) is NOT refused here, as the unrefined call does not refuse it: the stage runs the same loop
   with it (+infinity: every match with a finite error is an inlier; NaN, 0 or less: none is, and nothing is fitted), and
   the equality with the host statement is promised for the epsilons that statement accepts. */
int akz_match_features_fundamental_refined(akz_ctx* ctx, const akz_keypoint* keypoints_0, uint64_t n_keypoints_0,
                                           const uint8_t* descriptors_0, uint64_t n_descriptors_0, const akz_keypoint* keypoints_1,
                                           uint64_t n_keypoints_1, const uint8_t* descriptors_1, uint64_t n_descriptors_1,
                                           uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                           float ransac_epsilon_inliers, uint32_t refine_iterations, akz_match* out, uint64_t* n_out,
                                           float* f /* 9 */, int* found, uint32_t* iterations);
int akz_match_features_fundamental_refined_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                                 uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                                 float ransac_epsilon_inliers, uint32_t refine_iterations, akz_match* out,
                                                 uint64_t* n_out /* n_pairs */, float* f /* 9 x n_pairs */, int* found /* n_pairs */,
                                                 uint32_t* iterations /* n_pairs */);
int akz_match_features_fundamental_guided(akz_ctx* ctx, const akz_keypoint* keypoints_0, uint64_t n_keypoints_0,
                                          const uint8_t* descriptors_0, uint64_t n_descriptors_0, const akz_keypoint* keypoints_1,
                                          uint64_t n_keypoints_1, const uint8_t* descriptors_1, uint64_t n_descriptors_1,
                                          uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                          float ransac_epsilon_inliers, float guided_radius, double guided_lowes_ratio,
                                          akz_match* out, uint64_t* n_out, float* f /* 9 */, int* found);
int akz_match_features_fundamental_guided_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                                uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio, uint64_t ransac_trials,
                                                float ransac_epsilon_inliers, float guided_radius, double guided_lowes_ratio,
                                                akz_match* out, uint64_t* n_out /* n_pairs */, float* f /* 9 x n_pairs */,
                                                int* found /* n_pairs */);
int akz_match_features_fundamental_refined_guided(akz_ctx* ctx, const akz_keypoint* keypoints_0, uint64_t n_keypoints_0,
                                                  const uint8_t* descriptors_0, uint64_t n_descriptors_0,
                                                  const akz_keypoint* keypoints_1, uint64_t n_keypoints_1,
                                                  const uint8_t* descriptors_1, uint64_t n_descriptors_1, uint64_t desc_bytes,
                                                  double lowes_ratio, uint64_t ransac_trials, float ransac_epsilon_inliers,
                                                  uint32_t refine_iterations, float guided_radius, double guided_lowes_ratio,
                                                  akz_match* out, uint64_t* n_out, float* f /* 9 */, int* found, uint32_t* iterations);
int akz_match_features_fundamental_refined_guided_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets,
                                                        const uint64_t* pairs, uint64_t n_pairs, uint64_t desc_bytes, double lowes_ratio,
                                                        uint64_t ransac_trials, float ransac_epsilon_inliers, uint32_t refine_iterations,
                                                        float guided_radius, double guided_lowes_ratio, akz_match* out,
                                                        uint64_t* n_out /* n_pairs */, float* f /* 9 x n_pairs */,
                                                        int* found /* n_pairs */, uint32_t* iterations /* n_pairs */);

/* ---- seeded RANSAC: samples drawn on the GPU, trials stopped by confidence (an addition) ------------------------
   Every call above draws its samples on the calling thread from the thread's random source, in pair order, and runs exactly
   ransac_trials trials.  The calls below use a counter-based generator instead: the sample of trial t of a pair is a pure
   function of (seed, stream, t), so the trial kernel draws it itself, pairs do not depend on each other, and a confidence
   stops a pair's trials on the device.  The calling thread's random source is neither read nor advanced by any of them.
   The statement (csrc/akz_ransac_seeded.hpp; u64 arithmetic wraps):
     G = 0x9E3779B97F4A7C15;  mix64(z): z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31
     k0 = mix64(seed[0] + G), k1 = mix64(seed[1] ^ k0), ks = mix64(k1 + G (stream + 1)),
     v(t, i) = mix64(ks + G (8 t + i + 1)) for draw i < K of trial t; K = 8 (fundamental matrix) or 4 (homography).
   Sample of trial t over n >= K matches (Floyd: K draws, no rejection, every K-subset equally likely): for i = 0 .. K-1 with
   j = n - K + i, r = the high 64 bits of v(t, i) (j + 1); j is inserted if r is in the set already, else r; the K indices in
   ascending order.  The model of a sample and the inlier rule are those of akz_remove_outliers_fundamental (epsilon_model
   0.05) / akz_remove_outliers_homography (AKZ_HOMOGRAPHY_EPSILON_MODEL).  Trials run in rounds of 128 (the last may be
   shorter); after each round, with T trials done and best the largest inlier count so far (the first trial that reached it is
   the winner: a later tie does not replace it), a pair with confidence > 0 stops iff best >= need(n, K, T, confidence), the
   smallest b in 1 .. n with powi(1 - powi(b / n, K), T) <= 1 - confidence in f64 -- powi(w, K) by K - 1 successive
   multiplications by w, powi(q, T) by binary exponentiation (res = 1; while T: if T & 1: res *= q; T >>= 1; if T: q *= q),
   no contraction --; otherwise it stops at T = max_trials.  confidence = 0 switches the rule off: exactly max_trials run.
   Per pair: trials_run; found = best > 0; the model of the winner (zeros where found is 0, for both models); the list by the
   rules of the calls above -- fewer than K matches: unchanged, nothing run, trials_run 0; no winner: the zero model is
   evaluated (fundamental) or every match is kept (homography); max_trials = 0 as ransac_trials = 0.  Where found = 1 and
   refine_iterations > 0, the list, the model and iterations are those of akz_refine_fundamental_matrix / akz_refine_homography
   on the raw list from the winner with epsilon_inliers. */
/* A third model kind, for the seeded calls alone (akz_remove_outliers_seeded, akz_match_features_seeded_pairs; the guided calls
   refuse it, as they refuse 2): the Hartley-normalised 8-point algorithm with rank 2 enforced, judged in pixels.  The kind
   above keeps the reference's trial model -- the raw-pixel design matrix, no rank-2 step, the algebraic |p1^T F p0| -- because
   every call that promises the reference's bits must; the seeded calls promise none, and this is the model to use with them.
     model of a sample: fit(S) of akz_refine_fundamental_matrix over the eight matches in ascending order (steps 1 - 5 above
       with |S| = 8 and AKZ_FUNDAMENTAL_REFIT_EPSILON), every sum over e0 .. e7 as ((e0 + e4) + (e2 + e6)) + ((e1 + e5) +
       (e3 + e7)), each element from +0.0 -- what the 256-lane tree does to eight members.  So it equals one fit of
       akz_refine_fundamental_matrix(those eight, any f, an epsilon that keeps all eight, 1), bit for bit.  No model: a mean
       distance of 0 in either image, the rank rule, a norm that is zero or not finite.
     inlier rule (the Sampson distance below epsilon_inliers PIXELS, without a division; f32 in this order):
       l0 = (f0 x0 + f1 y0) + f2;  l1 = (f3 x0 + f4 y0) + f5;  l2 = (f6 x0 + f7 y0) + f8;  s = (l0 x1 + l1 y1) + l2
       m0 = (f0 x1 + f3 y1) + f6;  m1 = (f1 x1 + f4 y1) + f7;  d = ((l0 l0 + l1 l1) + m0 m0) + m1 m1
       inlier iff s s < (eps eps) d.  Strict: a zero model or a NaN passes nothing -- so without a winner the list is EMPTY
       (the zero model is evaluated, as for the other fundamental kind), the model is zeros and found is 0.
     refit: akz_refine_fundamental_normalised, which is akz_refine_fundamental_matrix with that inlier rule.
     guided stage: the epipolar band of AKZ_GUIDED_FUNDAMENTAL with the returned F.
   Fewer than 8 matches: the list is unchanged and trials_run is 0.  The value is 3: 2 stays refused. */
#define AKZ_RANSAC_FUNDAMENTAL_NORMALISED 3
/* The model of exactly 8 matches (given in ascending order of their position in the list they were sampled from): *found = 0
   where there is no model; f receives F (unit Frobenius norm, rank 2, p1^T F p0 = 0) where there is one. */
int akz_estimate_fundamental_normalised(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                        const akz_match* matches8, float* f /* 9 */, int* found);
/* akz_refine_fundamental_matrix with the Sampson rule above in place of |p1^T F p0| < epsilon_inlier: epsilon_inlier is a
   distance in pixels.  Arguments, results and refusals are those of akz_refine_fundamental_matrix. */
int akz_refine_fundamental_normalised(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                                      const akz_match* matches, uint64_t n_matches, const float* f_in /* 9 */, float epsilon_inlier,
                                      uint32_t max_iterations, akz_match* out, uint64_t* n_out, float* f_out /* 9, may be NULL */,
                                      uint32_t* iterations /* may be NULL */);
typedef struct akz_ransac_options {
    uint32_t struct_size;       /* sizeof(akz_ransac_options) */
    int32_t model_kind;         /* AKZ_GUIDED_HOMOGRAPHY, AKZ_GUIDED_FUNDAMENTAL or AKZ_RANSAC_FUNDAMENTAL_NORMALISED; the
                                   resection calls below: AKZ_RANSAC_RESECTION, and nothing else */
    double lowes_ratio;         /* of the descriptor scan (GPU call only) */
    uint64_t max_trials;        /* <= 1 << 24; the GPU call enqueues 2 launches per round of 128 and, per window of 8 rounds
                                   still running, computes 8 need() values per pair on the calling thread */
    float epsilon_inliers;
    uint32_t refine_iterations; /* 0: the refit is off */
    double confidence;          /* 0: off; otherwise 0 < c < 1 */
    uint64_t seed[2];
    uint64_t stream_base;       /* pair p of a call uses stream stream_base + p */
    int32_t guided;             /* != 0: the guided stage (GPU call only) */
    float guided_radius;
    double guided_lowes_ratio;
} akz_ransac_options;
/* fundamental matrix, ratio 0.86, 1 000 trials, confidence 0.99, seed {42, 69}, stream_base 0, the refit and the guided stage off (its
   radius 3 px and ratio 0.86 are set for a caller who switches it on); epsilon_inliers 0.02, the value tools/fundamental_refit.py
   measures with: |p1^T F p0| at unit norm, 1 .. 5 px on 1080p two-view scenes -- a homography wants pixels, set it */
void akz_ransac_options_default(akz_ransac_options* options);
/* the sample alone: out receives the k (4, 8, or the resection's 6) ascending indices of trial `trial` of `stream` over
   n_matches >= k matches */
int akz_draw_sample_seeded(uint64_t seed0, uint64_t seed1, uint64_t stream, uint64_t trial, uint64_t n_matches, int k,
                           uint64_t* out /* k */);
/* need(n_matches, k, trials, confidence) of the statement; k 4, 6 or 8, n_matches and trials >= 1, 0 < confidence < 1 */
int akz_ransac_required_inliers(uint64_t n_matches, int k, uint64_t trials, double confidence, uint64_t* need);
/* The host statement: rounds, winner, filter and refit over one raw match list with stream `stream`.  No GPU call and no
   descriptor work: lowes_ratio and the guided fields are ignored.  out must hold n_matches entries; model (9), found, iterations
   and trials_run may be NULL.  Refusals (AKZ_ERR_INVALID_ARG, nothing written): those of akz_remove_outliers, and of the
   options -- NULL, a struct_size other than sizeof(akz_ransac_options), an unknown model_kind, max_trials > 1 << 24, a confidence
   that is negative, NaN or >= 1 -- and, with refine_iterations > 0, an epsilon_inliers that akz_refine_homography refuses. */
int akz_remove_outliers_seeded(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                               const akz_match* matches, uint64_t n_matches, const akz_ransac_options* options, uint64_t stream,
                               akz_match* out, uint64_t* n_out, float* model /* 9 */, int* found, uint32_t* iterations,
                               uint64_t* trials_run);
/* match_features over many pairs with the seeded RANSAC, all on the GPU: sets, pairs, the layout of out and the fixed room per
   pair are those of akz_match_features_pairs.  Pair p's result equals akz_remove_outliers_seeded on that pair's raw list
   descriptor_match(d0, d1, 10000, lowes_ratio) with stream = stream_base + p, bit for bit: the list, the model bits, found,
   iterations and trials_run.  With guided != 0, where found = 1 the returned list is akz_descriptor_match_guided(pair,
   model_kind, the final model, guided_radius, 10000, guided_lowes_ratio), exactly as in the _guided forms above.  A pair's result
   therefore does not depend on the other pairs of the call: the batch equals the loop of one-pair calls with stream_base + p.
   model: 9 floats per pair, found / iterations / trials_run: one per pair; each may be NULL.
   Refusals (AKZ_ERR_INVALID_ARG, before any GPU work, nothing written): everything akz_match_features_pairs refuses, the
   options' refusals above, n_pairs >= 1 << 28, and with guided the guided call's radius rule (finite, >= 0) and limits.
   epsilon_inliers is NOT refused here, whatever refine_iterations is: the rule stated for the _refined forms above applies,
   and the equality with the host statement is promised for the epsilons that statement accepts. */
int akz_match_features_seeded_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                    uint64_t n_pairs, uint64_t desc_bytes, const akz_ransac_options* options, akz_match* out,
                                    uint64_t* n_out /* n_pairs */, float* model /* 9 x n_pairs */, int* found /* n_pairs */,
                                    uint32_t* iterations /* n_pairs */, uint64_t* trials_run /* n_pairs */);

/* ---- cross-checked matching: a match is kept only if both directions agree (additions) ------------------------------
   For descriptor sets A (n0 rows) and B (n1 rows), a distance_threshold and a lowes_ratio:
     fwd = descriptor_match(A, B, distance_threshold, lowes_ratio)    feature_matching.rs:23-94; index_0 a row of A
     rev = descriptor_match(B, A, distance_threshold, lowes_ratio)    arguments exchanged; index_0 a row of B
     cross(A, B) = [ m in fwd, in fwd's order : rev contains r with r.index_0 == m.index_1 and r.index_1 == m.index_0 ]
   Both directions follow the rules of descriptor_match: the minimum must be below the threshold, the test is
   (double)min < (double)second * lowes_ratio^2, ties go to the lowest index among equal minima.  A kept record is the forward
   record unchanged (its distance equals the reverse one: hamming is symmetric).  The result is never longer than fwd: out
   needs room for n0 records.  A lowes_ratio above 1 makes the ratio test nearly vacuous and leaves plain mutual nearest
   neighbours; it is accepted wherever descriptor_match accepts it.  cross(A, A) follows from the same statement, and an empty
   set on either side gives an empty result. */
/* The host statement: two scans and a lookup, no GPU call, no context.  Refusals (AKZ_ERR_INVALID_ARG, nothing written): those
   of akz_descriptor_match -- a NULL n_out, desc_bytes outside 1..64, NULL rows or out where there are rows. */
int akz_descriptor_match_cross_host(const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes,
                                    uint64_t distance_threshold, double lowes_ratio, akz_match* out, uint64_t* n_out);
/* The same list from the GPU for host arrays; arguments and refusals are those of akz_descriptor_match.  On the FP4 matcher (the
   default) and rows of at most 61 bytes both directions come from ONE pass over the distances
   (akz_descriptor_match_sets_mutual_device); rows of 62..64 bytes and the other matcher kernels scan twice.  The intersection
   runs on the device (k_pairs_cross_filter): one list comes back. */
int akz_descriptor_match_cross(akz_ctx* ctx, const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes,
                               uint64_t distance_threshold, double lowes_ratio, akz_match* out, uint64_t* n_out);
/* The same on device-resident 64-byte rows, as akz_descriptor_match_device (bytes 61..63 are padding and NOT compared): d_out
   holds n0 records, compacted in index_0 order, *d_n_out (device uint64) receives the count.  The call enqueues on the context's
   stream and returns; the scratch for the reverse list comes from the context. */
int akz_descriptor_match_cross_device(akz_ctx* ctx, const uint8_t* d_d0, uint64_t n0, const uint8_t* d_d1, uint64_t n1,
                                      uint64_t distance_threshold, double lowes_ratio, akz_match* d_out, uint64_t* d_n_out);
/* akz_match_features_seeded_pairs with cross(A, B, 10000, options->lowes_ratio) in place of descriptor_match(A, B) as each pair's
   raw list: the signature, the layout of out, the refusals and the promises are those of that call.  Pair p's result equals
   akz_remove_outliers_seeded on akz_descriptor_match_cross_host(pair p) with stream = stream_base + p, bit for bit -- the list,
   the model, found, iterations and trials_run -- so the batch still equals the loop of one-pair calls.
   The cross-check applies to the list RANSAC sees.  The guided stage, where switched on, stays what it is: a one-directional
   scan gated by the returned model, which is NOT cross-checked. */
int akz_match_features_seeded_cross_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                                          uint64_t n_pairs, uint64_t desc_bytes, const akz_ransac_options* options, akz_match* out,
                                          uint64_t* n_out /* n_pairs */, float* model /* 9 x n_pairs */, int* found /* n_pairs */,
                                          uint32_t* iterations /* n_pairs */, uint64_t* trials_run /* n_pairs */);

/* ---- relative pose: R, t and a cheirality filter per pair (additions) ------------------------------------------
   With known intrinsics, the step after a fundamental matrix: E = K1^T F K0, its four (R, t) candidates, the candidate that
   puts the matches in front of both cameras, and the matches that are in front.  The statement (csrc/akz_pose.hpp, ONE source
   for host and device; f64, no contraction, every sum of three terms is (t0 + t1) + t2):
     camera: a pinhole in pixels, K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]; no skew, no distortion.
     E = K1^T (F K0) with F as every call here returns it (p1^T F p0 = 0 in pixels).
     decomposition: the Hestenes rotations of the refit's rank-2 step on the three rows of E; the rotated rows are sigma_i v_i^T.
       Rows ordered by norm descending, the first among equals first: sigma1 >= sigma2 >= sigma3, v1, v2.  No pose if sigma1 is
       zero or not finite, or if !(sigma2 > AKZ_FUNDAMENTAL_REFIT_EPSILON sigma1) -- a zero model, a rank-1 F, a pure rotation in
       exact data.  u1 = E v1 / sigma1, u2 = E v2 / sigma2, u3 = u1 x u2, v3 = v1 x v2 (U and V are proper), W = [[0, -1, 0],
       [1, 0, 0], [0, 0, 1]], Ra = U W V^T, Rb = U W^T V^T, t = u3 / |u3|.  sigma3 is ignored: the unrefitted winner of
       model_kind 1 is not of rank 2, and sigma[] tells how far off it is.
     candidates, with x1 = R x0 + t:  0 = (Ra, +t), 1 = (Ra, -t), 2 = (Rb, +t), 3 = (Rb, -t).  (Which of the two rotations the
       decomposition calls Ra follows from the signs its rotations leave on v1 and v2: another SVD may number the same four
       candidates 3, 2, 1, 0.)
     cheirality of a match under (R, t): a = ((x0 - cx0) / fx0, (y0 - cy0) / fy0, 1), b likewise in image 1, c = R a,
       det = (c.c)(b.b) - (c.b)^2, n0 = (c.b)(b.t) - (c.t)(b.b), n1 = (c.c)(b.t) - (c.b)(c.t); in front iff det > 0 and n0 > 0
       and n1 > 0 -- the signs of the depths lambda0 = n0 / det, lambda1 = n1 / det at which the two rays meet in the
       least-squares sense.  A NaN passes nothing.
     winner: the candidate with the most matches in front, the first among equals; a largest count of 0: no pose.
     list: with a pose, the input matches in front under the winner, in input order; without one, the input unchanged.
     points (optional): per kept match X = (lambda0 a + R^T (lambda1 b - t)) / 2 in camera 0's frame at the scale |t| = 1. */
typedef struct akz_camera {
    double fx, fy, cx, cy;
} akz_camera;
typedef struct akz_pose {
    float r[9];           /* row-major */
    float t[3];           /* unit norm */
    float sigma[3];       /* sigma_i / sigma1 */
    uint32_t in_front[4]; /* per candidate */
    uint32_t winner;
    int32_t found;        /* 0: r, t and winner are zero; sigma and in_front hold what was computed, else zeros */
} akz_pose;
/* The host statement: no GPU call, no context.  out must hold n_matches entries; points (3 floats per kept match, in list
   order) may be NULL and is written only with a pose.  n_matches = 0: AKZ_OK with found 0.  Refusals (AKZ_ERR_INVALID_ARG,
   nothing written): those of akz_refine_fundamental_matrix for the keypoint and match arguments; a NULL f, camera, pose or
   n_out; a camera whose fx or fy is zero or whose fields are not finite. */
int akz_recover_pose_host(const akz_keypoint* keypoints_0, uint64_t n0, const akz_keypoint* keypoints_1, uint64_t n1,
                          const akz_match* matches, uint64_t n_matches, const float* f /* 9 */, const akz_camera* camera_0,
                          const akz_camera* camera_1, akz_match* out, uint64_t* n_out, akz_pose* pose,
                          float* points /* 3 x n_matches, may be NULL */);
/* akz_match_features_seeded_pairs (cross_check != 0: akz_match_features_seeded_cross_pairs) with the pose stage behind it, all
   on the GPU: ONE more launch in front of the one read-back.  Pair p equals akz_remove_outliers_seeded on its raw list followed,
   where found = 1, by akz_recover_pose_host with that list, that model and cameras[pairs[2 p]], cameras[pairs[2 p + 1]], bit for
   bit: the list, the model, found, iterations, trials_run, every field of the pose and the points.  Where found = 0 (fewer than
   8 matches among them) the seeded call's result stands and the pose is all zeros.  points: 3 floats per slot of out at the
   same offsets (pair p's k-th kept match at 3 (offset of pair p + k)); may be NULL.
   Refusals (AKZ_ERR_INVALID_ARG, before any GPU work, nothing written): everything the seeded call refuses; model_kind
   AKZ_GUIDED_HOMOGRAPHY; guided != 0 (a guided rescan behind a pose is later work); NULL cameras or poses; a camera that
   akz_recover_pose_host refuses among the n_sets. */
int akz_match_features_seeded_pose_pairs(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets,
                                         const akz_camera* cameras /* n_sets */, const uint64_t* pairs, uint64_t n_pairs,
                                         uint64_t desc_bytes, const akz_ransac_options* options, int cross_check, akz_match* out,
                                         uint64_t* n_out /* n_pairs */, float* model /* 9 x n_pairs */, int* found /* n_pairs */,
                                         uint32_t* iterations /* n_pairs */, uint64_t* trials_run /* n_pairs */,
                                         akz_pose* poses /* n_pairs */, float* points /* 3 per slot of out, may be NULL */);

/* ---- absolute pose: seeded 6-point resection RANSAC over many problems (additions) -----------------------------
   The call that places a camera against points that exist already: from 2D-3D correspondences -- for instance the `points` of
   the pose call above joined with the matches of a third image -- R and t with x_cam = R X + t, by the seeded RANSAC of the
   family above with a fourth model.  The statement (csrc/akz_resection.hpp, ONE source for host and device; f64 unless stated,
   no contraction):
     problem: n correspondences, each a point (X, Y, Z) in f32 and a pixel (u, v) in f32, and one akz_camera.  The camera's
       fields are cast to f32 ONCE per problem; the fit widens those casts to f64 again and the inlier rule uses them as they
       are.
     sample: K = 6 distinct indices in ascending order, the seeded statement's sample with K = 6 (draw i of trial t is
       v(t, i) = mix64(ks + G (8 t + i + 1)), as for 4 and 8).
     fit(S), the trial model with |S| = 6 and the refit's model with S the inliers:
       1. a = (u - cx) / fx, b = (v - cy) / fy.
       2. centroids of (a, b) and of (X, Y, Z); the mean distance of (a, b) from its centroid, sqrt(da da + db db), is scaled
          to sqrt 2, that of the points, sqrt((dX dX + dY dY) + dZ dZ), to sqrt 3; a mean distance of 0 on either side: no model.
       3. with Xh = (x, y, z, 1) normalised and q = {xx, xy, xz, x, yy, yz, y, zz, z, 1}: the 40 sums of q[k], a q[k], b q[k],
          (a a + b b) q[k] -- the blocks of M = A^T A = [[P, 0, -Qa], [0, P, -Qb], [-Qa, -Qb, W]] (12 x 12) for the DLT rows
          [Xh, 0, -a Xh], [0, Xh, -b Xh].  Every sum over S is formed in the order of akz_refine_homography's tree (element i
          in lane i mod 256, ascending from +0.0, then s = 128 .. 1); six members: ((e0 + e4) + e2) + ((e1 + e5) + e3) with
          every e_j entering as 0.0 + e_j and every absent element as + 0.0.
       4. the one-sided Jacobi sweeps on the 12 rows of M; the row of the smallest norm (the first among equals), normalised,
          is P~ (3 x 4, row-major); every other row norm must exceed AKZ_FUNDAMENTAL_REFIT_EPSILON^2 |S| / 6, else no model.
       5. P^ = T2^-1 P~ T3 (both normalisations undone) = s [R | t]; its sign flips if det of its left 3 x 3 block M3 is
          negative.  The Hestenes rotations of the relative pose's decomposition on the rows of M3 give sigma1 >= sigma2 >=
          sigma3 and v_i; u_i = M3 v_i / sigma_i; R = U V^T with R[r][c] = (u1[r] v1[c] + u2[r] v2[c]) + u3[r] v3[c], the
          rotation nearest M3; t = P^[:, 3] / (((sigma1 + sigma2) + sigma3) / 3); both rounded to f32.  No model where sigma1
          is zero or not finite or where !(sigma3 > AKZ_FUNDAMENTAL_REFIT_EPSILON sigma1).
       THE DLT CANNOT DO A PLANE: on coplanar points the null space of A has more than one dimension, and the sigma3 rule is
       what answers "no model" there.  A planar target needs another solver.
     inlier rule, f32 in this order, no division, with fx, fy, cx, cy the f32 casts:
       c_r = ((R[r][0] X + R[r][1] Y) + R[r][2] Z) + t[r];  ex = fx c_0 - (u - cx) c_2;  ey = fy c_1 - (v - cy) c_2;
       inlier iff c_2 > 0 and ex ex + ey ey < (eps eps)(c_2 c_2).  eps = epsilon_inliers is in PIXELS; the test is strict and
       a NaN passes nothing.
     rounds, winner, stop: the seeded statement's -- rounds of 128, the first maximum wins, a problem with confidence > 0
       stops after the round in which best >= need(n, 6, T, confidence).
     refit (refine_iterations > 0, where there is a winner): the loop of akz_refine_homography unchanged -- S, fit, reclassify,
       reject if smaller, stop when not grown -- over the problem's correspondences.
     result per problem: R, t, sigma_i / sigma1 and found; the indices of the kept correspondences, ascending; the fits
       accepted; trials_run.  found = 0 -- n < 6 (trials_run 0), no trial with a model, or a best count of 0 -- : the kept
       list is EMPTY and the pose is all zeros.
   Advice on epsilon_inliers: the 6-point DLT is a linear fit of twelve numbers to six points and its winner is far noisier than
   its data.  With pixel noise of standard deviation s, set epsilon_inliers to 4 s at the least, better 5 to 6 s, and
   refine_iterations to 2 or more: measured on 24 scenes of 800 true correspondences and 20 % outliers at s = 0.7 px, 3 px
   brings the refit to the whole true set at the median but to 48 % on the worst scene, 4 px to the whole set on all 24; at 2 px
   some winners are too poor for the refit to grow (README, the resection row; profiles/r32_resection.json).
   akz_ransac_options_default's 0.02 is the fundamental matrix's unit and is WRONG here: set it. */
#define AKZ_RANSAC_RESECTION 4 /* the resection calls' model_kind; every other call refuses it */
typedef struct akz_resection_problem {
    const float* points; /* 3 n: X, Y, Z per correspondence */
    const float* pixels; /* 2 n: u, v per correspondence */
    uint64_t n;          /* < 1 << 32 */
    akz_camera camera;
} akz_resection_problem;
typedef struct akz_resection {
    float r[9];     /* row-major */
    float t[3];
    float sigma[3]; /* sigma_i / sigma1 of the left block of P^: how far it was from a scaled rotation */
    int32_t found;  /* 0: everything above is zero */
} akz_resection;
/* fit(S) of exactly six correspondences, given in ascending order of their position in the problem they were sampled from.
   *found (may be NULL) and pose->found: 0 where there is no model, and the pose is zeros.  Refusals (AKZ_ERR_INVALID_ARG,
   nothing written): a NULL array, camera or pose; a camera that akz_recover_pose_host refuses. */
int akz_estimate_resection(const float* points6 /* 18 */, const float* pixels6 /* 12 */, const akz_camera* camera,
                           akz_resection* pose, int* found);
/* The refit alone, on the host: the loop above from pose_in's R and t (its sigma and found are not read) with epsilon in
   pixels.  kept (room for problem->n) receives the indices of the final set, ascending, *n_kept their number; pose_out (may
   be NULL): the last accepted fit with found = 1, or *pose_in unchanged where none was accepted; *iterations (may be NULL):
   the fits accepted.  Refusals (nothing written): a NULL problem, pose_in or n_kept; NULL points, pixels or kept where
   n > 0; n >= 1 << 32; the camera, as above; an epsilon that is not finite and > 0. */
int akz_refine_resection(const akz_resection_problem* problem, const akz_resection* pose_in, float epsilon,
                         uint32_t max_iterations, uint32_t* kept, uint64_t* n_kept, akz_resection* pose_out,
                         uint32_t* iterations);
/* The host statement: rounds, winner, filter and refit of one problem with stream `stream`.  No GPU call, no context.
   options: akz_ransac_options as it is, with model_kind = AKZ_RANSAC_RESECTION; lowes_ratio, guided_radius and
   guided_lowes_ratio are ignored.  kept: room for problem->n indices; iterations and trials_run may be NULL.
   Refusals (AKZ_ERR_INVALID_ARG, nothing written): the options' refusals of akz_remove_outliers_seeded with "model_kind is not
   AKZ_RANSAC_RESECTION" in place of the unknown kind; guided != 0; with refine_iterations > 0 an epsilon_inliers that
   akz_refine_resection refuses; a NULL problem, n_kept or pose; NULL points, pixels or kept where n > 0; n >= 1 << 32; a
   camera that akz_recover_pose_host refuses. */
int akz_resection_seeded_host(const akz_resection_problem* problem, const akz_ransac_options* options, uint64_t stream,
                              uint32_t* kept, uint64_t* n_kept, akz_resection* pose, uint32_t* iterations,
                              uint64_t* trials_run);
/* The same over many problems, all on the GPU: one upload (the problems packed into five f32 planes X | Y | Z | u | v behind one
   table of offsets and f32 cameras), per round of 128 trials two launches for all problems that still run, one launch for the
   filter and the refit, ONE read-back and one synchronisation.  Problem p uses stream options->stream_base + p and its kept
   indices (relative to the problem) start at kept[sum of n_q, q < p]; it equals akz_resection_seeded_host(problems + p,
   options, stream_base + p) bit for bit -- the indices, every word of the pose, iterations and trials_run -- so the batch
   equals the loop of one-problem calls.  kept beyond a problem's n_kept is not written.  n_kept, poses: one per problem;
   iterations, trials_run: one per problem, each may be NULL.  Scratch comes from the context and is kept for the next call.
   Refusals (AKZ_ERR_INVALID_ARG, before any GPU work, nothing written): a NULL ctx; everything akz_resection_seeded_host
   refuses, of any problem; n_problems >= 1 << 28; correspondences of all problems together >= 1 << 32.
   n_problems = 0: AKZ_OK, nothing done. */
int akz_resection_seeded_problems(akz_ctx* ctx, const akz_resection_problem* problems, uint64_t n_problems,
                                  const akz_ransac_options* options, uint32_t* kept, uint64_t* n_kept /* n_problems */,
                                  akz_resection* poses /* n_problems */, uint32_t* iterations /* n_problems */,
                                  uint64_t* trials_run /* n_problems */);

/* ---- feature banks: match pairs over feature sets that stay on the device (additions, not in the reference) -----
   An akz_bank is a list of feature sets resident on the device in the layout the pairs calls scan: every set's descriptors as
   64-byte rows (bytes at or beyond desc_bytes are zero) in ONE contiguous buffer, set after set, and the x and y of the
   keypoints those rows belong to (one float each per row).  It is immutable: nothing is appended or evicted, and no call writes to
   it.  It belongs to the context it was created on and owns its device block itself (the library's resource counters count it):
   akz_bank_free returns it.  A bank may outlive akz_ctx_destroy, exactly as an akz_result may: the context's own resources go
   with akz_ctx_destroy, the bank keeps its block and nothing else until akz_bank_free, and every call that takes the bank and its
   context is refused from then on.  Free every bank; one context's banks may be created, used and freed in any order. */
typedef struct akz_bank akz_bank;
/* The sets are every image of every result, in order: results[0] image 0, 1, ..., results[1] image 0, ...  A set's n_keypoints
   equals its n_descriptors, the image's keypoint count (0 for an image without keypoints).  The rows never leave the device:
   one launch (k_bank_gather) copies them from the results' row blocks, whatever the number of results and images, and writes the
   bytes beyond desc_bytes as zero whatever the source holds; x and y come from the results' host keypoints, one upload each.
   Complete on return: the results may be freed at once.  The results may belong to other contexts of the same device.
   Refusals (AKZ_ERR_INVALID_ARG, *out = NULL, before any GPU work and before any allocation): a NULL ctx, results, out or
   results[i]; n_results = 0; a result on another device than ctx; results whose descriptor sizes differ (descriptor_channels);
   a result whose finish half has not completed. */
int akz_bank_create_from_results(akz_ctx* ctx, const akz_result* const* results, uint64_t n_results, akz_bank** out);
/* The same object from host sets (features read from files; host sets that are matched again then pay the packing and the upload
   once): set k of the bank is sets[k], its rows packed and uploaded exactly as akz_match_features_pairs uploads a set a pair names
   -- the x and y of its first n_descriptors keypoints.  n_sets = 0 gives an empty bank.  Refusals (as above): for EVERY set what
   akz_match_features_pairs refuses for a set a pair names (more descriptors than keypoints, NULL keypoints or descriptors where
   there are some), desc_bytes outside 1..64, NULL sets while n_sets > 0, a NULL ctx or out. */
int akz_bank_create_from_sets(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, uint64_t desc_bytes, akz_bank** out);
/* A bank under a keypoint budget (akz_keypoint_budget, below): every set cut by akz_keypoint_budget_host.  With K_s, D_s the
   n_s keypoints and descriptors of source set s and idx_s what akz_keypoint_budget_host(K_s, n_s, budget, ...) returns, set s of
   the bank is (K_s[idx_s], D_s[idx_s]) in that ascending order, and the bank is byte for byte the one akz_bank_create_from_sets
   builds from those sliced host sets -- rows, the zero bytes at or beyond desc_bytes, x, y, akz_bank_info and akz_bank_set_info
   (n_keypoints = n_descriptors = min(max_keypoints, n_s)) -- so every bank call returns over it the bytes of the sets call over
   the sliced sets.  max_keypoints >= every n_s gives the bytes of the unbudgeted constructor, max_keypoints = 0 a bank of
   n_sets empty sets.  akz_bank_set_indices gives idx_s back.
   From results, the sets are those of akz_bank_create_from_results.  x, y and response of the results' host keypoints are uploaded
   once, the budget's kernels leave every set's kept indices on the device, and ONE launch (k_bank_select) gathers rows, x and y
   through them into the bank, whatever the number of sets; the kept indices come to the host with the call's one
   synchronisation.  No row of a result leaves the device.  Complete on return: the results may be freed at once.
   Refusals (AKZ_ERR_INVALID_ARG, *out = NULL, before any GPU work and before any allocation; the message names the result and
   the image): those of akz_bank_create_from_results, and the budget's -- a NULL budget, an unknown mode, SPREAD with robust
   outside (0, 1], a keypoint whose x, y or response is not finite, more than 2^31 - 1 keypoints in the call. */
typedef struct akz_keypoint_budget akz_keypoint_budget;
int akz_bank_create_from_results_budget(akz_ctx* ctx, const akz_result* const* results, uint64_t n_results,
                                        const akz_keypoint_budget* budget, akz_bank** out);
/* The same from host sets: the full sets are packed and uploaded to the context's staging as akz_match_features_pairs uploads
   them, and the same budget and the same launch select from there into the bank.  Refusals: those of akz_bank_create_from_sets,
   the budget's (the message names the set), and a set with n_descriptors != n_keypoints -- the budget is defined over keypoints
   that all have a row. */
int akz_bank_create_from_sets_budget(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, uint64_t desc_bytes,
                                     const akz_keypoint_budget* budget, akz_bank** out);
/* For every row of a set, in order, the index in its source set of the keypoint the row came from, so that the index_0 / index_1
   of a match record over the bank can be carried back to the extraction result: idx_s for a budgeted bank, the identity
   0 .. n - 1 for a bank of the two constructors without a budget.  Plain host code: the bank keeps the indices on the host.
   Refusals: a NULL bank, NULL indices for a set that is not empty, a set index >= n_sets. */
int akz_bank_set_indices(const akz_bank* bank, uint64_t set, uint64_t* indices /* that set's n_keypoints */);
/* n_sets, desc_bytes and the rows of all sets; each pointer may be NULL. */
int akz_bank_info(const akz_bank* bank, uint64_t* n_sets, uint64_t* desc_bytes, uint64_t* rows);
/* One set's counts and its first row in the bank's buffers; each pointer may be NULL.  A set index >= n_sets is refused. */
int akz_bank_set_info(const akz_bank* bank, uint64_t set, uint64_t* n_keypoints, uint64_t* n_descriptors, uint64_t* row0);
/* The bank's device buffers, for callers that read them with their own kernels (torch): rows x 64 bytes, rows floats, rows floats.
   Read-only, valid until akz_bank_free; each pointer may be NULL. */
int akz_bank_device(const akz_bank* bank, const uint8_t** d_rows, const float** d_x, const float** d_y);
int akz_bank_free(akz_bank* bank);
/* akz_match_features_seeded_pairs (cross_check != 0: akz_match_features_seeded_cross_pairs) over the sets of a bank: for a bank made
   from sets S -- by either constructor; from results, S is every image's keypoints and descriptors -- the call returns what that
   call returns over (S, n_sets, desc_bytes), bit for bit: lists, counts, models, found, iterations and trials_run, in the same
   layout of out, the guided stage included.  No set is packed or uploaded; the bank is not written.  Refusals
   (AKZ_ERR_INVALID_ARG, before any GPU work, nothing written): those of that call that do not concern a set's pointers, a NULL bank,
   a bank of another context. */
int akz_match_features_seeded_bank_pairs(akz_ctx* ctx, const akz_bank* bank, const uint64_t* pairs, uint64_t n_pairs,
                                         const akz_ransac_options* options, int cross_check, akz_match* out,
                                         uint64_t* n_out /* n_pairs */, float* model /* 9 x n_pairs */, int* found /* n_pairs */,
                                         uint32_t* iterations /* n_pairs */, uint64_t* trials_run /* n_pairs */);
/* akz_match_features_seeded_pose_pairs over the sets of a bank, one camera per set of the bank; the same promise -- every field of
   the poses and the points too -- and the same refusals. */
int akz_match_features_seeded_pose_bank_pairs(akz_ctx* ctx, const akz_bank* bank, const akz_camera* cameras /* n_sets */,
                                              const uint64_t* pairs, uint64_t n_pairs, const akz_ransac_options* options,
                                              int cross_check, akz_match* out, uint64_t* n_out /* n_pairs */,
                                              float* model /* 9 x n_pairs */, int* found /* n_pairs */,
                                              uint32_t* iterations /* n_pairs */, uint64_t* trials_run /* n_pairs */,
                                              akz_pose* poses /* n_pairs */, float* points /* 3 per slot of out, may be NULL */);

/* ---- k-nearest-neighbour matching: the k best train rows of every query, with their distances (additions) -----------
   For descriptor sets A (n0 rows) and B (n1 rows), 1 <= k <= AKZ_KNN_MAX_K and a distance_threshold, knn(A, B, k, threshold) is,
   for every row i of A:
     * take all rows j of B with d(i, j) = hamming(A_i, B_j) < distance_threshold (strict, the threshold of descriptor_match; any
       threshold above 8 * desc_bytes therefore means none);
     * order them by (d, j) ascending -- among equal distances the lowest train index first, descriptor_match's tie rule
       extended to k -- and keep the first k;
     * counts[i] = the number kept, 0 .. min(k, n1);
     * out[i * k + r], r < counts[i]  = {index_0 = i, index_1 = j_r, distance = (double)d_r};
     * out[i * k + r], r >= counts[i] = {index_0 = i, index_1 = UINT64_MAX, distance = +infinity}: every slot is defined, whole
       buffers can be compared.
   No ratio test is applied: descriptor_match(A, B, thr, ratio) keeps query i iff, with min = d_0 (thr if counts[i] < 1) and
   second = d_1 (thr if counts[i] < 2) of knn(A, B, 2, thr), (double)min < (double)second * ratio^2 and min < thr -- and then
   names j_0.  out holds n0 * k records, counts n0 values.  n1 == 0: every count is 0 and every slot padding; n0 == 0: nothing
   is written.  Refusals (AKZ_ERR_INVALID_ARG, before any GPU work, nothing written): k == 0 or k > AKZ_KNN_MAX_K, desc_bytes
   outside 1..64, a NULL out or counts, NULL rows where there are rows, n0 or n1 above 0x7fffffff. */
#define AKZ_KNN_MAX_K 8
/* The host statement: a popcount scan with a sorted insertion, no GPU call, no context.  Every one of the desc_bytes bytes counts. */
int akz_descriptor_match_knn_host(const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes, uint64_t k,
                                  uint64_t distance_threshold, akz_match* out, uint32_t* counts);
/* The same buffers from the GPU for host arrays, complete on return: the distances come from the FP4 matrix instruction
   (k_knn_fp4), exact integers, so the result equals the statement bit for bit.  desc_bytes 1..61; rows of 62..64 bytes return
   AKZ_ERR_UNSUPPORTED with nothing written (the FP4 image carries 488 columns, and there is no popcount form of this call). */
int akz_descriptor_match_knn(akz_ctx* ctx, const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes, uint64_t k,
                             uint64_t distance_threshold, akz_match* out, uint32_t* counts);
/* The same on device-resident 64-byte rows, as akz_descriptor_match_device (bytes 61..63 are padding and NOT compared): d_out
   receives n0 * k records, d_counts n0 values, both on the device.  The call enqueues on the context's stream and returns
   without synchronising; the scratch for the partial lists comes from the context. */
int akz_descriptor_match_knn_device(akz_ctx* ctx, const uint8_t* d_d0, uint64_t n0, const uint8_t* d_d1, uint64_t n1, uint64_t k,
                                    uint64_t distance_threshold, akz_match* d_out, uint32_t* d_counts);

/* ---- keypoint budget: at most N keypoints of a set, the strongest or the best spread (additions) -----------------------
   A stage of its own over feature sets, between extract_features and the matching calls (every matching cost grows with the
   square of the keypoint count); no extraction or matching call changes.  For one set of n keypoints take x_i, y_i and
   r_i = response, all f32; every operation below is one IEEE f32 operation, rounded on its own (no contraction, subnormals kept):
     * AKZ_BUDGET_STRONGEST: the order is (r descending, index ascending).  Responses compare as float values: -0 equals +0.
     * AKZ_BUDGET_SPREAD (adaptive non-maximal suppression; Brown, Szeliski and Winder 2005):
         d2(i, j)  = fl(fl(dx * dx) + fl(dy * dy))  with dx = fl(x_i - x_j), dy = fl(y_i - y_j);
         j dominates i iff r_i < fl(robust * r_j)  (j = i is not excepted: a keypoint with a negative response dominates itself);
         radius2_i = the minimum of d2(i, j) over all j that dominate i, +infinity where none does;
         the order is (radius2 descending, r descending, index ascending).
     * the first min(max_keypoints, n) of the order are kept and reported in ASCENDING index order -- the detector's order is
       preserved, indices[0 .. *n_out) -- and *n_out is their number.  max_keypoints = 0 keeps nothing and is AKZ_OK.
     * radius2 (optional, SPREAD only): all n values of the set, every slot defined.
   The minimum and the place in the order depend on no traversal order, so every tiling gives the same bits.
   Refusals (AKZ_ERR_INVALID_ARG, before any GPU work, nothing written, the message names the set): NULL options, an unknown mode,
   SPREAD with robust outside (0, 1] (NaN included), an x, y or response that is not finite, NULL keypoints where n > 0, a NULL
   indices or n_out, a non-NULL radius2 in STRONGEST mode, a set of more than 2^31 - 1 keypoints. */
#define AKZ_BUDGET_STRONGEST 0
#define AKZ_BUDGET_SPREAD 1
typedef struct akz_keypoint_budget {
    uint64_t max_keypoints;
    uint32_t mode;  /* AKZ_BUDGET_* */
    float robust;   /* SPREAD: 0 < robust <= 1 (0.9 is customary); STRONGEST: not read */
} akz_keypoint_budget;
/* The host statement for one set: plain loops and a sort, no GPU call, no context.  indices has room for min(max_keypoints, n)
   entries, radius2 (may be NULL) for n. */
int akz_keypoint_budget_host(const akz_keypoint* keypoints, uint64_t n, const akz_keypoint_budget* options, uint64_t* indices,
                             uint64_t* n_out, float* radius2);
/* The statement over many sets in one call, on the GPU, bit for bit the host statement per set.  Of every akz_feature_set only
   keypoints and n_keypoints are read (descriptors may be NULL).  Fixed room per set, as in akz_match_features_pairs: set s writes
   its indices (n_out[s] of them) and its radius2 values (all n_keypoints) from offset sum_{q<s} sets[q].n_keypoints on; indices
   and radius2 hold sum_s sets[s].n_keypoints entries, n_out holds n_sets.  Empty sets and n_sets = 0 are AKZ_OK.  Further
   refusals: a NULL ctx or NULL sets while n_sets > 0, all sets together above 2^31 - 1 keypoints.
   One upload (x, y, response of all sets and two tables), the all-pairs radius and rank passes (k_budget_walk: a keypoint is kept
   iff fewer than N others stand before it in the order -- counted, not sorted, exact under ties), one ordered compaction per set
   and one download, on the context's stream with the context's scratch; complete on return. */
int akz_keypoint_budget_sets(akz_ctx* ctx, const akz_feature_set* sets, uint64_t n_sets, const akz_keypoint_budget* options,
                             uint64_t* indices, uint64_t* n_out /* n_sets */, float* radius2);

/* ---- on-disk formats of akaze-util ---------------------------------- */
/* akaze_util::{serialize,deserialize}_{features,matches}_{to,from}_file — akaze-util/src/lib.rs:17-67.
   A path ending in ".json" is serde_json, anything else bincode 1.x (little-endian, u64 lengths), exactly
   as the reference chooses (lib.rs:24-28).  descriptors: n x desc_bytes.  The read functions return the
   counts when the output pointers are NULL. */
int akz_write_features(const char* path, const akz_keypoint* kps, uint64_t n, const uint8_t* descriptors,
                       uint64_t desc_bytes);
int akz_read_features(const char* path, akz_keypoint* kps, uint8_t* descriptors, uint64_t cap_keypoints,
                      uint64_t cap_desc_bytes, uint64_t* n_keypoints, uint64_t* n_descriptors, uint64_t* desc_bytes);
int akz_write_matches(const char* path, const akz_match* matches, uint64_t n);
int akz_read_matches(const char* path, akz_match* out, uint64_t cap, uint64_t* n_out);

/* ---- host-only pieces, callable without a GPU --------------------------------------------- */
/* find_scale_space_extrema's order-dependent cache logic + the sub-pixel step
   (scale_space_extrema.rs:43-178) on NMS candidates {u32 level, u32 flat_idx, f32 v, xp, xm, yp, ym,
   u32 pad} that already passed threshold, 4-neighbour maximum and the border test.  Keypoints are
   returned without orientation (angle = 0). */
int akz_host_select_keypoints(uint32_t w, uint32_t h, const akz_config* cfg, const void* cand, uint64_t n_cand,
                              akz_keypoint* out, uint64_t cap, uint64_t* n_out, uint64_t* n_extrema);

/* ---- measurement hooks --------------------------------------------------------------- */
/* Stage timing with HIP events recorded on the context's stream (device stages) and the host
   clock (host stages).  Off by default; when on, every extract call adds its stage times. */
typedef enum akz_stage {
    AKZ_ST_BLUR0 = 0,    /* level-0 Gaussian blur (lib.rs:56)                            */
    AKZ_ST_CONTRAST = 1, /* compute_contrast_factor (lib.rs:64-69)                       */
    AKZ_ST_PREP = 2,     /* per level: clone/half_size, Lsmooth, Lflow (lib.rs:80-105)   */
    AKZ_ST_FED = 3,      /* per level: the calculate_step launches (lib.rs:109-118)      */
    AKZ_ST_DETECTOR = 4, /* detector_response (detector_response.rs:38-55)               */
    AKZ_ST_NMS = 5,      /* stand-alone NMS launches (if any) + D2H of the candidate lists */
    AKZ_ST_HOST_KP = 6,  /* host: sort, cache logic, refinement                          */
    AKZ_ST_ORIENT = 7,   /* orientation kernel + host atan2f/cosf/sinf                   */
    AKZ_ST_MLDB = 8,     /* descriptor kernel + D2H                                      */
    AKZ_ST_TOTAL = 9,    /* wall time of the whole extract call (host clock)             */
    AKZ_STAGE_COUNT = 10
} akz_stage;
typedef struct akz_profile {
    double ms[AKZ_STAGE_COUNT];
    uint64_t fed_launches;   /* FED kernel launches inside AKZ_ST_FED                        */
    uint64_t fed_px_steps;   /* sum over launches of pixels x steps advanced (x batch)       */
    uint64_t calls;          /* extract calls accumulated                                     */
    uint64_t pixels;         /* input pixels accumulated (w*h*n per call)                     */
    uint64_t det_launches;   /* detector kernel launches inside AKZ_ST_DETECTOR               */
    uint64_t det_px;         /* sum over those launches of level pixels (x batch)             */
    uint64_t fused_px;       /* level pixels (x batch) whose preparation ran inside a FED launch (k_level_march) */
    /* What the context's stream-placement probe found (akz_ctx_warmup / the first large batch; state, not accumulated):
       probed 0/1; early_stages 2 = a batch's level-0 stages run ahead on the copy stream, 0 = on the caller's stream (the
       copy stream could not be given a hardware queue and a pipe of its own: perf only, -5 %); replaced = streams the probe
       re-created; shared = streams that still share a queue or pipe with another busy one; retries = measurements repeated
       because the first answer was "shared" or ambiguous */
    uint32_t placement_probed, placement_early_stages, placement_replaced, placement_shared, placement_retries, placement_reserved;
} akz_profile;
/* on: 0 = off, 1 = every stage (two HIP events per stage and level), 2 = light: only the FED and detector spans and
   the host-clock stages (what bench.py uses inside its timed region) */
int akz_ctx_set_profiling(akz_ctx* ctx, int on);
/* akz_profile has grown at its end (ABI 5) and may again.  akz_ctx_get_profile2 writes min(struct_size, sizeof(akz_profile))
   bytes -- pass sizeof(akz_profile) of the header the caller was compiled against; akz_ctx_get_profile, the original symbol,
   writes the ABI-4 prefix only (everything before placement_probed), so a host built against the smaller struct is never
   written past its end. */
int akz_ctx_get_profile2(akz_ctx* ctx, akz_profile* out, uint64_t struct_size, int reset);
int akz_ctx_get_profile(akz_ctx* ctx, akz_profile* out, int reset);
/* Optional, once, with the caller's stream idle and NOT being captured: runs the stream-placement probe now (~2 ms: spins
   and tiny kernels on the context's streams, which are synchronised) instead of inside the first large akz_extract_begin_*
   -- that call then stays asynchronous.  The probe measures which of the context's streams share a hardware queue or a
   command-processor pipe and replaces those that do; every timing that says "shared" is repeated and the shortest decides.
   Results never depend on it; akz_ctx_get_profile reports what it found. */
int akz_ctx_warmup(akz_ctx* ctx);
/* Extrema candidates per image that the next extraction reserves room for (default 32768; it grows to 1.25x
   the largest count seen).  A list that overflows is detected by akz_extract_finish, which enlarges it and
   repeats the extrema pass on the stored Ldet planes — results are the same, the call is slower; the setter
   exists so that this path can be tested and so that callers with very dense frames can skip the retry. */
int akz_ctx_set_candidate_hint(akz_ctx* ctx, uint32_t per_image);
/* Lanes for small jobs.  A lone 1080p frame is a chain of ~45 launches of a few hundred workgroups each: the chip is busy
   but only a fraction of it at a time.  With lanes = k (2..8) the extract_begin calls of jobs below 2.4 Mpx (the lane gate of DESIGN.md 6.1) are dealt in
   turn to k child contexts with their own streams, scratch planes, candidate buffers and HOST THREAD: the finish half of
   a lane's job (candidate round trip, keypoint selection, orientation / descriptor kernels and their copies) starts on
   the lane's thread as soon as the job has been begun, so that the chains of consecutive frames overlap on the chip and
   their host halves on the host; akz_extract_finish waits for the lane and hands the result over.  Larger jobs, and
   everything at lanes = 1 (default), run on the context itself.  The caller's stream is respected (a lane starts behind
   what the caller enqueued before the call); results are bit-identical and are used through the same calls. */
int akz_ctx_set_lanes(akz_ctx* ctx, uint32_t lanes);
/* The finish half on the context's own thread (default ON).  The finish half of every job begun through
   akz_extract_begin_* -- candidate fetch, keypoint selection, orientation / descriptor kernels, copies -- is started by the
   begin call on a thread the library owns; akz_extract_finish waits for it and hands the result over (results, error
   reporting through akz_extract_finish and akz_job_abandon are the same either way; the synchronous akz_extract_* calls
   run both halves on the caller's thread).  The caller's thread then only enqueues: with two batches begun ahead, whatever
   else it does between the calls (the exchange of a multi-GPU job, file I/O) no longer delays the keypoint half of the
   batches in flight -- worth +13 % on a rank with two host cores, nothing on sixteen.  Entry points that share state with
   the finish half (result queries that launch kernels, the setters) wait until the thread is idle; akz_extract_begin_*, the
   matcher and akz_result_free do not.  on = 0: akz_extract_finish runs the finish half itself (jobs dealt to lanes are
   always finished by their lane's thread). */
int akz_ctx_set_eager_finish(akz_ctx* ctx, int on);
/* Host threads of the finish half of an extraction (candidate bucketing, per-image keypoint selection, libm calls):
   0 (default) = automatic -- the affinity mask of the process, cut down by the cgroup CPU quota and divided by
   LOCAL_WORLD_SIZE (one process per GPU: torchrun sets it), at most 16.  A launcher that has already pinned each rank
   to its own cores passes that number here.  Not while extractions are in flight. */
int akz_ctx_set_host_threads(akz_ctx* ctx, uint32_t threads);
/* ---- image ingest, options files (host code) -------------------- */
/* What `image::open(path)` hands to the crate (akaze/src/lib.rs:171): JPEG (baseline / progressive
   Huffman, 8 bit, 1 or 3 components), PNG (non-interlaced) and binary PNM, decoded to 8-bit luma
   (*channels = 1) or RGB (*channels = 3) as stored.  The pixel buffers returned by the akz_image_*
   loaders are released with akz_image_free.  Decoding of lossy formats is not bit-pinned against the
   `image` / `jpeg-decoder` crates (their sources are not in the reference tree). */
int akz_image_load(const char* path, uint32_t* width, uint32_t* height, uint32_t* channels, uint8_t** pixels);
/* image::open(path).to_luma() — the input of create_unit_float_image (types/image.rs:127-140) */
int akz_image_load_luma(const char* path, uint32_t* width, uint32_t* height, uint8_t** luma);
/* image::open(path).to_rgb() — what the debug drawings are made on (extract_features.rs:94-96) */
int akz_image_load_rgb(const char* path, uint32_t* width, uint32_t* height, uint8_t** rgb);
void akz_image_free(void* pixels);
/* akaze::extract_features(input_image_path, options) — akaze/src/lib.rs:167-194: decode, to_luma,
   unit float image, scale space, keypoints, descriptors.  Equivalent to akz_image_load_luma +
   akz_extract_gray_u8: a JPEG is entropy-decoded on the host and reconstructed on the device (the same pixels). */
int akz_extract_features_file(akz_ctx* ctx, const char* path, const akz_config* cfg, uint32_t flags, akz_result** out);
/* akz_image_load_luma into device memory: the w * h luma bytes (row-major) at d_luma, complete on return.  A JPEG is
   entropy-decoded on the host and reconstructed on the device on the context's stream (bytes identical to
   akz_image_load_luma); PNG and PNM are decoded on the host and uploaded.  Same errors as akz_image_load_luma.  If
   capacity < w * h: AKZ_ERR_BUFFER, *width / *height set, nothing written (d_luma may be NULL with capacity 0). */
int akz_image_load_luma_device(akz_ctx* ctx, const char* path, uint8_t* d_luma, uint64_t capacity, uint32_t* width,
                               uint32_t* height);
/* extract_features over n files of one size as one batch job: the result of akz_extract_device_u8 on their luma frames.
   The files are decoded on the context's host threads (akz_ctx_set_host_threads), each uploaded and reconstructed into
   its frame while the others are still decoding.  Files of different sizes: AKZ_ERR_INVALID_ARG naming the first path
   whose size differs from paths[0]'s; an unreadable or corrupt file: the status of akz_image_load_luma.  No result then. */
int akz_extract_features_files(akz_ctx* ctx, const char* const* paths, uint64_t n, const akz_config* cfg, uint32_t flags,
                               akz_result** out);
/* serde_json form of Config (what `-o options.json` reads and writes, extract_features.rs:66-83).
   to_json: writes a NUL-terminated string, *len = its length (AKZ_ERR_BUFFER if cap is too small, *len
   then holds the size needed).  from_json: fields that are absent keep the value already in *cfg
   (serde itself would reject the file: every field is required there). */
int akz_config_to_json(const akz_config* cfg, char* buf, uint64_t cap, uint64_t* len);
int akz_config_from_json(const char* json, akz_config* cfg);

/* `random::default().seed([s0, s1])`: reseeds the calling thread's default random source — one Xorshift128+
   stream per thread, initially seeded [42, 69], shared by the RANSAC sampling of akz_remove_outliers /
   akz_match_features (estimate_fundamental_matrix.rs:118-121) and the colours of the debug drawings
   (types/image.rs:385-392), exactly as the `random` crate 0.12 behaves inside one process. */
int akz_random_seed(uint64_t s0, uint64_t s1);

/* ---- debug output (host code) ----------------------------------- */
/* 8-bit PNG, channels = 1 (luma) or 3 (RGB) */
int akz_image_save_png(const char* path, const uint8_t* pixels, uint32_t width, uint32_t height, uint32_t channels);
/* types::image::save — normalize to [0,1] (min/max), `(v * 255) as u8`, write (types/image.rs:168-197);
   a 0x0 plane writes nothing */
int akz_image_save_plane_png(const char* path, const float* plane, uint32_t width, uint32_t height);
/* types::evolution::write_evolutions (evolution.rs:175-218): Lt_00000..png ... Ldet_000NN..png (sic: build_path's
   set_extension(".png"), evolution.rs:163-168, keeps the dot of its argument) of image `img`
   into directory `dir` (must exist).  Needs a result extracted with AKZ_KEEP_ALL_PLANES to contain every
   plane; planes that were not kept are skipped like the reference skips 0x0 images. */
int akz_write_evolutions(const akz_result* res, uint64_t img, const char* dir);
/* types::image::random_color (image.rs:385-392): the next colour of the calling thread's default random source */
int akz_random_color(uint8_t* rgb /* 3 */);
/* types::image::draw_circle (image.rs:418-443) / draw_line (image.rs:453-480) on an 8-bit RGB image; pixels outside the
   image are skipped (the reference would panic) */
int akz_draw_circle(uint8_t* rgb, uint32_t width, uint32_t height, float x, float y, const uint8_t* color /* 3 */,
                    float radius);
int akz_draw_line(uint8_t* rgb, uint32_t width, uint32_t height, float x0, float y0, float x1, float y1,
                  const uint8_t* color /* 3 */, float radius);
/* types::keypoint::draw_keypoints_to_image (keypoint.rs:52-56): blends a disc of radius `size` at every
   keypoint into the RGB image, each in the next random_color() of the calling thread's default source
   (image.rs:385-392; see akz_random_seed).  Pixels outside the image are skipped (the reference would panic). */
int akz_draw_keypoints(uint8_t* rgb, uint32_t width, uint32_t height, const akz_keypoint* kps, uint64_t n);
/* types::feature_match::draw_matches (feature_match.rs:32-82): the two images side by side (each half as wide as
   the wider one), one line per match.  *out_rgb is released with akz_image_free. */
int akz_draw_matches(const uint8_t* rgb0, uint32_t w0, uint32_t h0, const uint8_t* rgb1, uint32_t w1, uint32_t h1,
                     const akz_keypoint* kp0, uint64_t n0, const akz_keypoint* kp1, uint64_t n1,
                     const akz_match* matches, uint64_t n_matches, uint32_t* out_w, uint32_t* out_h, uint8_t** out_rgb);

#ifdef __cplusplus
}
#endif
#endif /* AKAZE_HIP_H */
