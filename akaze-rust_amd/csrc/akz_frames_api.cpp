// C ABI of frame ingest (akz_frames.hpp): the layout's checks, akz_luma_from_frames_host (the statement: plain loops around
// luma_u8), akz_luma_from_frames_device (k_frame_luma on the context's stream) and the two extraction entry points, which hand
// the checked layout to extract_begin_dispatch (akz_extract.cpp) -- the staging and the stream rules are there.
#include <string>

#include "akz_extract.hpp"

namespace akz {

int frames_resolve(const char* who, const void* src, const akz_frame_layout* l, uint32_t n, FrameSpec& fs) {
    auto refuse = [&](const char* what) {
        set_error(std::string(who) + ": " + what);
        return AKZ_ERR_INVALID_ARG;
    };
    if (!src) return refuse("null frames (src)");
    if (!l) return refuse("null layout");
    if (n == 0) return refuse("n is 0");
    if (l->format > AKZ_FRAME_RGB8_PLANAR) return refuse("unknown format");
    if (l->width == 0) return refuse("width is 0");
    if (l->height == 0) return refuse("height is 0");
    static const uint32_t kBpp[6] = {1, 3, 3, 4, 4, 1};
    fs.format = l->format, fs.w = l->width, fs.h = l->height, fs.bpp = kBpp[l->format];
    const bool planar = l->format == AKZ_FRAME_RGB8_PLANAR;
    const uint64_t tight_row = (uint64_t)fs.w * fs.bpp;
    fs.row_pitch = l->row_pitch ? l->row_pitch : tight_row;
    if (fs.row_pitch < tight_row) return refuse("row_pitch is smaller than width * bytes per pixel");
    if (fs.row_pitch > UINT64_MAX / 4 / fs.h) return refuse("row_pitch * height overflows");
    const uint64_t tight_plane = fs.row_pitch * fs.h;
    fs.plane_stride = planar ? (l->plane_stride ? l->plane_stride : tight_plane) : 0;
    if (planar && fs.plane_stride < tight_plane) return refuse("plane_stride is smaller than row_pitch * height");
    if (planar && fs.plane_stride > UINT64_MAX / 4) return refuse("plane_stride overflows");
    const uint64_t tight_frame = planar ? 3 * fs.plane_stride : tight_plane;
    fs.frame_stride = l->frame_stride ? l->frame_stride : tight_frame;
    if (fs.frame_stride < tight_frame) return refuse(planar ? "frame_stride is smaller than 3 * plane_stride" : "frame_stride is smaller than row_pitch * height");
    if (n > 1 && fs.frame_stride > UINT64_MAX / n) return refuse("frame_stride * n overflows");
    return AKZ_OK;
}

}  // namespace akz

int frames_enqueue(akz_ctx* c, hipStream_t s, const uint8_t* d_src, const FrameSpec& fs, uint32_t n, uint8_t* d_luma) {
    StageTimer t(c, kStageIngest, s);
    t.kernel(AKZ_KR_FRAME_LUMA, fs.format, fs.w, fs.h, n, 1, (uint64_t)fs.w * fs.h * n);
    launch::frame_luma(s, d_src, fs, n, d_luma);
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}

extern "C" {

int akz_luma_from_frames_host(const uint8_t* src, const akz_frame_layout* layout, uint32_t n, uint8_t* luma) {
    FrameSpec fs;
    AKZ_TRY(frames_resolve("akz_luma_from_frames_host", src, layout, n, fs));
    if (!luma) {
        set_error("akz_luma_from_frames_host: null destination (luma)");
        return AKZ_ERR_INVALID_ARG;
    }
    const bool swap = fs.format == AKZ_FRAME_BGR8 || fs.format == AKZ_FRAME_BGRA8;
    // bytes from a pixel's R to its G (and G to B), and from a pixel to the next
    const uint64_t chan = fs.format == AKZ_FRAME_RGB8_PLANAR ? fs.plane_stride : 1;
    uint8_t* o = luma;
    for (uint32_t f = 0; f < n; ++f)
        for (uint32_t y = 0; y < fs.h; ++y) {
            const uint8_t* row = src + (uint64_t)f * fs.frame_stride + (uint64_t)y * fs.row_pitch;
            if (fs.format == AKZ_FRAME_GRAY8) {
                for (uint32_t x = 0; x < fs.w; ++x) *o++ = row[x];
                continue;
            }
            for (uint32_t x = 0; x < fs.w; ++x) {
                const uint8_t* p = row + (uint64_t)x * fs.bpp;
                *o++ = swap ? luma_u8(p[2], p[1], p[0]) : luma_u8(p[0], p[chan], p[2 * chan]);
            }
        }
    return AKZ_OK;
}

int akz_luma_from_frames_device(akz_ctx* c, const uint8_t* d_src, const akz_frame_layout* layout, uint32_t n, uint8_t* d_luma) {
    FrameSpec fs;
    AKZ_TRY(frames_resolve("akz_luma_from_frames_device", d_src, layout, n, fs));
    if (!d_luma) {
        set_error("akz_luma_from_frames_device: null destination (d_luma)");
        return AKZ_ERR_INVALID_ARG;
    }
    AKZ_TRY(bind(c));
    return frames_enqueue(c, c->stream, d_src, fs, n, d_luma);
}

int akz_extract_device_frames(akz_ctx* c, const uint8_t* d_src, const akz_frame_layout* layout, uint32_t n, const akz_config* cfg,
                              uint32_t flags, akz_result** out) {
    if (!out) {
        set_error("akz_extract_device_frames: null out");
        return AKZ_ERR_INVALID_ARG;
    }
    *out = nullptr;
    FrameSpec fs;
    AKZ_TRY(frames_resolve("akz_extract_device_frames", d_src, layout, n, fs));
    if (!c || !cfg) {
        set_error("akz_extract_device_frames: null context / config");
        return AKZ_ERR_INVALID_ARG;
    }
    return extract_frames(c, d_src, fs, n, cfg, flags, out);
}

int akz_extract_begin_device_frames(akz_ctx* c, const uint8_t* d_src, const akz_frame_layout* layout, uint32_t n, const akz_config* cfg,
                                    uint32_t flags, akz_job** out) {
    if (!out) {
        set_error("akz_extract_begin_device_frames: null out");
        return AKZ_ERR_INVALID_ARG;
    }
    *out = nullptr;
    FrameSpec fs;
    AKZ_TRY(frames_resolve("akz_extract_begin_device_frames", d_src, layout, n, fs));
    if (!c || !cfg) {
        set_error("akz_extract_begin_device_frames: null context / config");
        return AKZ_ERR_INVALID_ARG;
    }
    return extract_begin_frames(c, d_src, fs, n, cfg, flags, out);
}

}  // extern "C"
