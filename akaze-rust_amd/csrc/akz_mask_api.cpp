// C ABI of the detection mask: the masked forms of the frame calls and of akz_extract_gray_u8 hand a checked MaskSpec to the
// extraction (akz_extract.cpp; the filter itself is enqueued by extract_begin and, after an overflow, by the finish half), and the
// two debug hooks -- the kernel alone on a caller-made list, and the counts of the last masked job.
#include <string>

#include "akz_extract.hpp"

namespace {
// d_mask == NULL together with layout == NULL: no mask (*masked = false).  Otherwise a GRAY8 layout of the frames' size, n_masks
// 1 (shared: frame stride 0) or n; every refusal names its field.
int mask_resolve(const char* who, const uint8_t* d_mask, const akz_frame_layout* layout, uint32_t n_masks, uint32_t w, uint32_t h, uint32_t n,
                 MaskSpec& m, bool* masked) {
    auto refuse = [&](const std::string& what) {
        set_error(std::string(who) + ": " + what);
        return AKZ_ERR_INVALID_ARG;
    };
    *masked = false;
    if (!d_mask && !layout) return AKZ_OK;
    if (!d_mask) return refuse("d_mask is null but mask_layout is not (both null = no mask)");
    if (!layout) return refuse("mask_layout is null but d_mask is not (both null = no mask)");
    if (n_masks != 1 && n_masks != n) return refuse("n_masks must be 1 (one mask for every frame) or n");
    if (layout->format != AKZ_FRAME_GRAY8) return refuse("mask_layout.format must be AKZ_FRAME_GRAY8");
    if (layout->width != w || layout->height != h)
        return refuse("mask_layout.width x height (" + std::to_string(layout->width) + " x " + std::to_string(layout->height) +
                      ") is not the frames' (" + std::to_string(w) + " x " + std::to_string(h) + ")");
    FrameSpec ms;
    AKZ_TRY(frames_resolve((std::string(who) + ": mask_layout").c_str(), d_mask, layout, n_masks, ms));
    m = MaskSpec{d_mask, ms.row_pitch, n_masks == 1 ? 0 : ms.frame_stride};
    *masked = true;
    return AKZ_OK;
}
}  // namespace

extern "C" {

int akz_extract_device_frames_masked(akz_ctx* c, const uint8_t* d_src, const akz_frame_layout* layout, uint32_t n, const uint8_t* d_mask,
                                     const akz_frame_layout* mask_layout, uint32_t n_masks, const akz_config* cfg, uint32_t flags,
                                     akz_result** out) {
    static const char* who = "akz_extract_device_frames_masked";
    if (!out) {
        set_error(std::string(who) + ": null out");
        return AKZ_ERR_INVALID_ARG;
    }
    *out = nullptr;
    FrameSpec fs;
    AKZ_TRY(frames_resolve(who, d_src, layout, n, fs));
    MaskSpec m;
    bool masked = false;
    AKZ_TRY(mask_resolve(who, d_mask, mask_layout, n_masks, fs.w, fs.h, n, m, &masked));
    if (!c || !cfg) {
        set_error(std::string(who) + ": null context / config");
        return AKZ_ERR_INVALID_ARG;
    }
    return extract_frames(c, d_src, fs, n, cfg, flags, out, masked ? &m : nullptr);
}

int akz_extract_begin_device_frames_masked(akz_ctx* c, const uint8_t* d_src, const akz_frame_layout* layout, uint32_t n, const uint8_t* d_mask,
                                           const akz_frame_layout* mask_layout, uint32_t n_masks, const akz_config* cfg, uint32_t flags,
                                           akz_job** out) {
    static const char* who = "akz_extract_begin_device_frames_masked";
    if (!out) {
        set_error(std::string(who) + ": null out");
        return AKZ_ERR_INVALID_ARG;
    }
    *out = nullptr;
    FrameSpec fs;
    AKZ_TRY(frames_resolve(who, d_src, layout, n, fs));
    MaskSpec m;
    bool masked = false;
    AKZ_TRY(mask_resolve(who, d_mask, mask_layout, n_masks, fs.w, fs.h, n, m, &masked));
    if (!c || !cfg) {
        set_error(std::string(who) + ": null context / config");
        return AKZ_ERR_INVALID_ARG;
    }
    return extract_begin_frames(c, d_src, fs, n, cfg, flags, out, masked ? &m : nullptr);
}

int akz_debug_mask_candidates(akz_ctx* c, const void* d_records, uint32_t capacity, uint32_t* d_counts, const uint8_t* d_mask,
                              const akz_frame_layout* mask_layout, uint32_t n_masks, uint32_t w, uint32_t h, const akz_config* cfg, uint32_t n,
                              void* d_kept) {
    static const char* who = "akz_debug_mask_candidates";
    if (!d_records || !d_counts || !d_kept || !cfg || capacity == 0 || n == 0 || d_records == d_kept) {
        set_error(std::string(who) + ": null records / counts / kept / config, zero capacity or n, or kept == records");
        return AKZ_ERR_INVALID_ARG;
    }
    if ((uintptr_t)d_counts & 7) {
        set_error(std::string(who) + ": d_counts must be 8-byte aligned");
        return AKZ_ERR_INVALID_ARG;
    }
    MaskSpec m;
    bool masked = false;
    AKZ_TRY(mask_resolve(who, d_mask, mask_layout, n_masks, w, h, n, m, &masked));
    if (!masked) {
        set_error(std::string(who) + ": null mask");
        return AKZ_ERR_INVALID_ARG;
    }
    AKZ_TRY(bind(c));
    std::vector<LevelPlan> plan;
    AKZ_TRY(build_plan(w, h, *cfg, plan));
    if (plan.size() > (size_t)kMaxLevels) return AKZ_ERR_INVALID_ARG;
    std::vector<uint32_t> lw, lh, lo;
    for (const LevelPlan& lv : plan) lw.push_back(lv.w), lh.push_back(lv.h), lo.push_back(lv.octave);
    launch::mask_candidates(c->stream, (const Candidate*)d_records, (Candidate*)d_kept, capacity, d_counts, m.d, m.row_pitch, m.frame_stride,
                            lw.data(), lh.data(), lo.data(), (uint32_t)plan.size(), n);
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}

int akz_debug_mask_counts(akz_ctx* c, uint64_t out[3]) {
    if (!out) return AKZ_ERR_INVALID_ARG;
    AKZ_TRY(bind(c));
    const akz_ctx* q = c;
    for (const akz_ctx* l : c->lanes)
        if (l->mask_stamp.load() > q->mask_stamp.load()) q = l;
    for (int k = 0; k < 3; ++k) out[k] = q->mask_last[k].load();
    return AKZ_OK;
}

}  // extern "C"
