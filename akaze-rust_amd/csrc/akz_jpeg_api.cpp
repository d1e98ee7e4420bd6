// C ABI of file ingest with JPEG reconstruction on the device (akz_jpeg.hpp): akz_image_load_luma_device,
// akz_extract_features_file and akz_extract_features_files.  The host decoder entropy-decodes a JPEG straight into a
// pinned staging slot of the context; the dense int16 coefficients go to the device on the context's stream, where
// k_jpeg_idct and k_jpeg_luma turn them into the luma frame akz_image_load_luma would return.  PNG and PNM are decoded on
// the host and their luma frame goes up through the same slot.
#include <exception>
#include <string>

#include "akz_ctx.hpp"
#include "akz_jpeg.hpp"

namespace {

using akz::img::jpg::Frame;

// The event of a slot's last upload has passed: the slot may be written again.
int slot_wait(akz_ctx* c, int slot) {
    if (c->jpeg_up[slot]) AKZ_HIP_TRY(hipEventSynchronize(c->jpeg_up[slot]));
    return AKZ_OK;
}

// A file decoded into staging slot `slot`: a JPEG's coefficients (jpeg = true, frame f) or a host-decoded luma frame.
struct Staged {
    bool jpeg = false;
    Frame f{};
    uint32_t w = 0, h = 0;
};

// Reads and decodes `path` into slot `slot` with the host decoder's statuses and messages.  cap_px >= 0: the caller's
// destination holds cap_px bytes -- a frame larger than that stops the decode at the JPEG frame header (PNG / PNM: after
// decoding) with AKZ_ERR_BUFFER and its size in st.w / st.h.
int stage_file(akz_ctx* c, int slot, const char* path, int64_t cap_px, Staged& st) {
    std::vector<uint8_t> d;
    if (!img::read_file(path, d)) {
        set_error(std::string("image: cannot read ") + path);
        return AKZ_ERR_IO;
    }
    auto too_small = [&](uint32_t w, uint32_t h) {
        st.w = w; st.h = h;
        if (cap_px < 0 || (uint64_t)w * h <= (uint64_t)cap_px) return false;
        set_error("akz_image_load_luma_device: the destination is smaller than the frame (width x height bytes)");
        return true;
    };
    if (!img::is_jpeg(d)) {
        std::vector<uint8_t> luma;
        AKZ_TRY(img::load_luma_bytes(path, d, &st.w, &st.h, luma));
        if (too_small(st.w, st.h)) return AKZ_ERR_BUFFER;
        AKZ_TRY(slot_wait(c, slot));
        AKZ_TRY(ensure_pinned(c, c->jpeg_pin[slot], luma.size()));
        std::memcpy(c->jpeg_pin[slot].p, luma.data(), luma.size());
        st.jpeg = false;
        return AKZ_OK;
    }
    img::jpg::CoefAlloc alloc = [&](const Frame& f, int* status) -> int16_t* {
        if (too_small(f.width, f.height)) {
            *status = AKZ_ERR_BUFFER;
            return nullptr;
        }
        if ((*status = slot_wait(c, slot)) != AKZ_OK) return nullptr;
        if ((*status = ensure_pinned(c, c->jpeg_pin[slot], (size_t)f.nblocks * 64 * sizeof(int16_t))) != AKZ_OK) return nullptr;
        return (int16_t*)c->jpeg_pin[slot].p;
    };
    try {
        AKZ_TRY(img::jpg::decode_coefs(d.data(), d.size(), alloc, st.f));
    } catch (const std::exception& e) {  // as img::load: bad_alloc on absurd header sizes
        set_error(std::string("image: ") + e.what());
        return AKZ_ERR_NO_MEMORY;
    }
    st.jpeg = true;
    st.w = st.f.width;
    st.h = st.f.height;
    return AKZ_OK;
}

// Enqueues on the context's stream what turns slot `slot` into the luma frame at d_dst: the coefficient upload and the two
// kernels (a JPEG), or the frame's upload.  Records the slot's event behind the upload.
int reconstruct(akz_ctx* c, int slot, const Staged& st, uint8_t* d_dst) {
    hipStream_t s = c->stream;
    AKZ_TRY(c->jpeg_up[slot].ensure());
    if (!st.jpeg) {
        AKZ_HIP_TRY(hipMemcpyAsync(d_dst, c->jpeg_pin[slot].p, (size_t)st.w * st.h, hipMemcpyHostToDevice, s));
        AKZ_HIP_TRY(hipEventRecord(c->jpeg_up[slot], s));
        return AKZ_OK;
    }
    const Frame& f = st.f;
    const size_t coef_bytes = (size_t)f.nblocks * 64 * sizeof(int16_t);
    AKZ_TRY(ensure(c, c->jpeg_coef, coef_bytes));
    AKZ_TRY(ensure(c, c->jpeg_plane, f.plane_bytes));
    uint8_t* d_plane = (uint8_t*)c->jpeg_plane.p;
    {
        StageTimer t(c, kStageIngest, s);
        t.kernel(AKZ_KR_JPEG_COPY, f.nc, f.width, f.height, 1, 1, coef_bytes);
        AKZ_HIP_TRY(hipMemcpyAsync(c->jpeg_coef.p, c->jpeg_pin[slot].p, coef_bytes, hipMemcpyHostToDevice, s));
    }
    AKZ_HIP_TRY(hipEventRecord(c->jpeg_up[slot], s));
    {
        StageTimer t(c, kStageIngest, s);
        t.kernel(AKZ_KR_JPEG_IDCT, f.nc, f.width, f.height, 1, 1, (uint64_t)f.nblocks * 64);
        launch::jpeg_idct(s, f, (const int16_t*)c->jpeg_coef.p, d_plane);
    }
    {
        StageTimer t(c, kStageIngest, s);
        t.kernel(AKZ_KR_JPEG_LUMA, f.nc, f.width, f.height, 1, 1, (uint64_t)f.width * f.height);
        launch::jpeg_luma(s, f, d_plane, d_dst);
    }
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}

}  // namespace

extern "C" {

int akz_image_load_luma_device(akz_ctx* c, const char* path, uint8_t* d_luma, uint64_t capacity, uint32_t* width, uint32_t* height) {
    if (!c || !path || !width || !height || (!d_luma && capacity)) {
        set_error("akz_image_load_luma_device: null argument");
        return AKZ_ERR_INVALID_ARG;
    }
    AKZ_TRY(bind(c));
    Staged st;
    const int status = stage_file(c, 0, path, (int64_t)std::min<uint64_t>(capacity, (uint64_t)INT64_MAX), st);
    if (status == AKZ_ERR_BUFFER) {
        *width = st.w;
        *height = st.h;
    }
    AKZ_TRY(status);
    AKZ_TRY(reconstruct(c, 0, st, d_luma));
    AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    *width = st.w;
    *height = st.h;
    return AKZ_OK;
}

// akaze::extract_features(input_image_path, options) — akaze/src/lib.rs:167-194.  A JPEG is reconstructed on the device
// into the extraction's input; other formats take the host path (akz_image_load_luma + akz_extract_gray_u8).
int akz_extract_features_file(akz_ctx* c, const char* path, const akz_config* cfg, uint32_t flags, akz_result** out) {
    if (!c || !path || !out) {
        set_error("akz_extract_features_file: null argument");
        return AKZ_ERR_INVALID_ARG;
    }
    std::vector<uint8_t> head;
    {
        FILE* f = fopen(path, "rb");
        if (f) {
            head.resize(3);
            head.resize(fread(head.data(), 1, 3, f));
            fclose(f);
        }
    }
    if (!img::is_jpeg(head)) {
        uint32_t w = 0, h = 0;
        uint8_t* luma = nullptr;
        AKZ_TRY(akz_image_load_luma(path, &w, &h, &luma));
        const int st = akz_extract_gray_u8(c, luma, w, h, cfg, flags, out);
        akz_image_free(luma);
        return st;
    }
    AKZ_TRY(bind(c));
    Staged st;
    AKZ_TRY(stage_file(c, 0, path, -1, st));
    AKZ_TRY(ensure(c, c->jpeg_frames, (size_t)st.w * st.h));
    AKZ_TRY(reconstruct(c, 0, st, (uint8_t*)c->jpeg_frames.p));
    // the frame is consumed by level 0 on the same stream before anything else touches jpeg_frames
    return akz_extract_device_u8(c, (const uint8_t*)c->jpeg_frames.p, st.w, st.h, 1, cfg, flags, out);
}

int akz_extract_features_files(akz_ctx* c, const char* const* paths, uint64_t n, const akz_config* cfg, uint32_t flags,
                               akz_result** out) {
    if (!c || !paths || !n || !out) {
        set_error("akz_extract_features_files: null argument or no files");
        return AKZ_ERR_INVALID_ARG;
    }
    *out = nullptr;
    for (uint64_t i = 0; i < n; ++i)
        if (!paths[i]) {
            set_error("akz_extract_features_files: null path");
            return AKZ_ERR_INVALID_ARG;
        }
    if (n > 0xffffffffull) {
        set_error("akz_extract_features_files: too many files");
        return AKZ_ERR_INVALID_ARG;
    }
    AKZ_TRY(bind(c));
    WorkerPool& pool = c->pool();
    // one staging slot per thread that decodes (at most kJpegSlots): a thread holds its slot from the frame header to the
    // upload, so the pinned memory is bounded by the pool, not by n
    const int slots = (int)std::min<uint64_t>(std::min<unsigned>(pool.size(), akz_ctx::kJpegSlots), n);
    std::mutex free_m;
    std::vector<int> free_slots;
    for (int k = slots - 1; k >= 0; --k) free_slots.push_back(k);
    struct Item {
        int status = AKZ_OK;
        bool done = false;  // decoded (or failed); false: skipped after an earlier failure
        std::string error;
        uint32_t w = 0, h = 0;
    };
    std::vector<Item> items((size_t)n);
    std::atomic<size_t> first_stop{SIZE_MAX};  // the lowest index that failed: later files are not decoded
    auto stop_at = [&](size_t i) {
        size_t cur = first_stop.load();
        while (i < cur && !first_stop.compare_exchange_weak(cur, i)) {
        }
    };
    uint32_t bw = 0, bh = 0;  // frame size of the batch buffer (the first file uploaded; guarded by jpeg_m)
    pool.run((size_t)n, [&](size_t i) {
        Item& it = items[i];
        if (i > first_stop.load()) return;
        int slot;
        {
            std::lock_guard<std::mutex> lk(free_m);
            slot = free_slots.back();  // (never empty: a slot per thread of the pool)
            free_slots.pop_back();
        }
        Staged st;
        it.status = hipSetDevice(c->device) == hipSuccess ? AKZ_OK : AKZ_ERR_HIP;
        if (it.status == AKZ_OK) it.status = stage_file(c, slot, paths[i], -1, st);
        it.w = st.w;
        it.h = st.h;
        if (it.status == AKZ_OK) {
            std::lock_guard<std::mutex> lk(c->jpeg_m);
            if (!bw) {
                it.status = ensure(c, c->jpeg_frames, (size_t)st.w * st.h * n);
                if (it.status == AKZ_OK) bw = st.w, bh = st.h;
            }
            if (it.status == AKZ_OK && st.w == bw && st.h == bh)
                it.status = reconstruct(c, slot, st, (uint8_t*)c->jpeg_frames.p + (size_t)bw * bh * i);
            else if (it.status == AKZ_OK)
                stop_at(i);  // a size that differs: reported below against the first file
        }
        if (it.status != AKZ_OK) {
            it.error = get_error();  // (the message is per thread)
            stop_at(i);
        }
        it.done = true;
        std::lock_guard<std::mutex> lk(free_m);
        free_slots.push_back(slot);
    });
    // the first file (in order) that failed or differs in size from paths[0]: every file before the lowest index that
    // stopped the batch was decoded, and of a pair of sizes that disagree both files were
    int status = AKZ_OK;
    std::string error;
    for (size_t i = 0; i < items.size() && status == AKZ_OK; ++i) {
        const Item& it = items[i];
        if (!it.done) continue;
        if (it.status != AKZ_OK) {
            status = it.status;
            error = it.error;
        } else if (items[0].status == AKZ_OK && (it.w != items[0].w || it.h != items[0].h)) {
            status = AKZ_ERR_INVALID_ARG;
            error = "akz_extract_features_files: " + std::string(paths[i]) + " is " + std::to_string(it.w) + "x" + std::to_string(it.h) +
                    ", " + paths[0] + " is " + std::to_string(items[0].w) + "x" + std::to_string(items[0].h) +
                    " (the files of a batch must have one size)";
        }
    }
    if (status != AKZ_OK) {
        AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
        set_error(error);
        return status;
    }
    return akz_extract_device_u8(c, (const uint8_t*)c->jpeg_frames.p, bw, bh, (uint32_t)n, cfg, flags, out);
}

}  // extern "C"
