// Feature banks (additions; include/akaze_hip.h): feature sets kept on the device in the layout the pairs calls scan,
// so that extraction results reach the seeded pairs calls without a round trip through host memory and sets that are matched again
// are placed once.  akz_bank_create_from_results: bank_segments (the table, plain host code), x / y from the results' host
// keypoints through pinned staging, and launch::bank_gather (akz_bank.hip) -- ONE launch -- over the results' device rows.
// akz_bank_create_from_sets: the packing and the copies of pairs_upload (akz_match_api.cpp) into the bank's block.  The two bank
// forms of the seeded pairs calls are those calls with the bank handed down to pairs_front (akz_match_seeded_api.cpp).
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "akz_extract.hpp"

using namespace akz;

namespace {
int refuse(const std::string& what) {
    set_error(what);
    return AKZ_ERR_INVALID_ARG;
}
uint64_t result_desc_bytes(const akz_result* r) { return ((6 + 36 + 120) * r->cfg.descriptor_channels + 7) / 8; }  // (akz_result_counts)

// One segment per image of every result, in order: where its rows lie and where they go.  Returns the rows of all of them.
uint64_t bank_segments(const akz_result* const* results, uint64_t n_results, std::vector<launch::BankSeg>& segs) {
    segs.clear();
    uint64_t rows = 0;
    for (uint64_t i = 0; i < n_results; ++i) {
        const akz_result* r = results[i];
        for (uint32_t img = 0; img < r->n; ++img) {
            const uint64_t n = r->kps[img].size();
            segs.push_back(launch::BankSeg{n ? r->d_desc64 + r->desc_off[img] * 64 : nullptr, n, rows});
            rows += n;
        }
    }
    return rows;
}
// the bank's block for `rows` rows: rows | x | y, every part on 256 bytes
int bank_alloc(akz_ctx* c, akz_bank* b, uint64_t rows) {
    const uint64_t rows1 = std::max<uint64_t>(rows, 1);
    const size_t b_rows = up256((size_t)rows1 * 64), b_xy = up256((size_t)rows1 * 4);
    AKZ_HIP_TRY(b->dev.acquire(b_rows + 2 * b_xy, false));
    AKZ_HIP_TRY(alloc_fill(c, b->dev.p, b->dev.bytes));
    b->rows = rows;
    b->d_rows = (uint8_t*)b->dev.p;
    b->d_kx = (float*)(b->d_rows + b_rows), b->d_ky = (float*)(b->d_rows + b_rows + b_xy);
    return AKZ_OK;
}
void bank_place(akz_bank* b) {  // every set behind the one before it
    b->set_row.assign(b->sets.size(), 0);
    uint64_t rows = 0;
    for (size_t k = 0; k < b->sets.size(); ++k) {
        b->set_row[k] = rows;
        rows += b->sets[k].n_descriptors;
    }
}
akz_bank* bank_keep(akz_ctx* c, std::unique_ptr<akz_bank>& b) {
    b->ctx = c;
    ++c->live_results;
    return b.release();
}
// the table through pinned staging to c->mp_tab, then the one launch, on the context's stream (not synchronised); the table lies
// `pin_off` bytes into c->mp_pin_in, which holds at least pin_off + the table
int bank_gather_enqueue(akz_ctx* c, const std::vector<launch::BankSeg>& segs, size_t pin_off, uint64_t rows, uint64_t desc_bytes, uint8_t* d_dst) {
    if (segs.empty() || rows == 0) return AKZ_OK;
    hipStream_t st = c->stream;
    const size_t b_tab = segs.size() * sizeof(launch::BankSeg);
    AKZ_TRY(ensure(c, c->mp_tab, b_tab));
    char* h_tab = (char*)c->mp_pin_in.p + pin_off;
    std::memcpy(h_tab, segs.data(), b_tab);
    AKZ_HIP_TRY(hipMemcpyAsync(c->mp_tab.p, h_tab, b_tab, hipMemcpyHostToDevice, st));
    StageTimer t(c, kStageIngest, st);
    t.kernel(AKZ_KR_BANK_GATHER, (uint32_t)desc_bytes, 64, (uint32_t)std::min<uint64_t>(rows, 0xffffffffull), (uint32_t)segs.size(), 1, rows);
    launch::bank_gather(st, (const launch::BankSeg*)c->mp_tab.p, (uint32_t)segs.size(), rows, (uint32_t)desc_bytes, d_dst);
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}
}  // namespace

extern "C" {

int akz_bank_create_from_results(akz_ctx* c, const akz_result* const* results, uint64_t n_results, akz_bank** out) {
    const std::string name = "bank_create_from_results: ";
    if (out) *out = nullptr;
    if (!c || !results || !out) return refuse(name + "null context, results or out");
    if (n_results == 0) return refuse(name + "no result (the descriptor size of a bank is that of its results)");
    uint64_t images = 0, rows = 0;
    for (uint64_t i = 0; i < n_results; ++i) {
        const akz_result* r = results[i];
        const std::string at = name + "result " + std::to_string(i) + ": ";
        if (!r) return refuse(at + "null");
        if (!r->ctx || r->ctx->device != c->device) return refuse(at + "it lies on another device than the context");
        bool done = r->kps.size() == r->n && r->desc_off.size() == (size_t)r->n + 1;
        for (uint32_t img = 0; done && img < r->n; ++img) done = r->kps[img].empty() || r->d_desc64 != nullptr;
        if (!done) return refuse(at + "its finish half has not completed");
        if (result_desc_bytes(r) != result_desc_bytes(results[0]))
            return refuse(at + "descriptors of " + std::to_string(result_desc_bytes(r)) + " bytes, result 0 has " +
                          std::to_string(result_desc_bytes(results[0])));
        images += r->n;
        for (uint32_t img = 0; img < r->n; ++img) rows += r->kps[img].size();
    }
    if (images > 0xffffffffull || rows > launch::kBankMaxRows) return refuse(name + "too many images or rows for one launch");
    AKZ_TRY(bind(c));
    std::unique_ptr<akz_bank> b(new akz_bank);
    b->desc_bytes = result_desc_bytes(results[0]);
    std::vector<launch::BankSeg> segs;
    bank_segments(results, n_results, segs);
    for (const launch::BankSeg& s : segs) b->sets.push_back(akz_feature_set{nullptr, s.n_rows, nullptr, s.n_rows});
    bank_place(b.get());
    AKZ_TRY(bank_alloc(c, b.get(), rows));
    // x | y of every keypoint, then the table, in pinned memory: one copy each
    const size_t b_xy = up256((size_t)std::max<uint64_t>(rows, 1) * 4);
    AKZ_TRY(ensure_pinned(c, c->mp_pin_in, 2 * b_xy + segs.size() * sizeof(launch::BankSeg)));
    float *hx = (float*)c->mp_pin_in.p, *hy = (float*)((char*)c->mp_pin_in.p + b_xy);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n_results; ++i)
        for (const auto& kps : results[i]->kps)
            for (const akz_keypoint& k : kps) hx[at] = k.x, hy[at] = k.y, ++at;
    hipStream_t st = c->stream;
    if (rows) {
        AKZ_HIP_TRY(hipMemcpyAsync(b->d_kx, hx, (size_t)rows * 4, hipMemcpyHostToDevice, st));
        AKZ_HIP_TRY(hipMemcpyAsync(b->d_ky, hy, (size_t)rows * 4, hipMemcpyHostToDevice, st));
    }
    AKZ_TRY(bank_gather_enqueue(c, segs, 2 * b_xy, rows, b->desc_bytes, b->d_rows));
    AKZ_HIP_TRY(hipStreamSynchronize(st));  // complete on return: the results may go
    *out = bank_keep(c, b);
    return AKZ_OK;
}

int akz_bank_create_from_sets(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, uint64_t desc_bytes, akz_bank** out) {
    const std::string name = "bank_create_from_sets: ";
    if (out) *out = nullptr;
    if (!out) return refuse(name + "null out");
    if (desc_bytes == 0 || desc_bytes > 64) return refuse(name + "desc_bytes must be 1..64");
    if (n_sets && !sets) return refuse(name + "null sets");
    uint64_t rows = 0;
    for (uint64_t k = 0; k < n_sets; ++k) {
        const akz_feature_set& s = sets[k];
        const std::string at = name + "set " + std::to_string(k) + ": ";
        if (s.n_descriptors > s.n_keypoints) return refuse(at + "more descriptors than keypoints");
        if ((s.n_keypoints && !s.keypoints) || (s.n_descriptors && !s.descriptors)) return refuse(at + "null keypoints or descriptors");
        rows += s.n_descriptors;
    }
    if (!c) return refuse(name + "null context");
    AKZ_TRY(bind(c));
    std::unique_ptr<akz_bank> b(new akz_bank);
    b->desc_bytes = desc_bytes;
    for (uint64_t k = 0; k < n_sets; ++k) b->sets.push_back(akz_feature_set{nullptr, sets[k].n_keypoints, nullptr, sets[k].n_descriptors});
    bank_place(b.get());
    AKZ_TRY(bank_alloc(c, b.get(), rows));
    PairsFront f;  // every set, in order, as pairs_open would have placed it had every set been named
    f.set_row = b->set_row;
    for (uint64_t k = 0; k < n_sets; ++k) f.used.push_back(k);
    f.rows = rows;
    const uint64_t rows1 = std::max<uint64_t>(rows, 1);
    f.b_rows = up256((size_t)rows1 * 64), f.b_xy = up256((size_t)rows1 * 4);
    f.d_rows = b->d_rows, f.d_kx = b->d_kx, f.d_ky = b->d_ky;
    AKZ_TRY(ensure_pinned(c, c->mp_pin_in, f.b_rows + 2 * f.b_xy));
    if (rows) AKZ_TRY(pairs_upload(c, sets, desc_bytes, f));
    AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    *out = bank_keep(c, b);
    return AKZ_OK;
}

int akz_bank_info(const akz_bank* b, uint64_t* n_sets, uint64_t* desc_bytes, uint64_t* rows) {
    if (!b) return refuse("bank_info: null bank");
    if (n_sets) *n_sets = b->sets.size();
    if (desc_bytes) *desc_bytes = b->desc_bytes;
    if (rows) *rows = b->rows;
    return AKZ_OK;
}

int akz_bank_set_info(const akz_bank* b, uint64_t set, uint64_t* n_keypoints, uint64_t* n_descriptors, uint64_t* row0) {
    if (!b) return refuse("bank_set_info: null bank");
    if (set >= b->sets.size()) return refuse("bank_set_info: set index " + std::to_string(set) + " >= n_sets " + std::to_string(b->sets.size()));
    if (n_keypoints) *n_keypoints = b->sets[(size_t)set].n_keypoints;
    if (n_descriptors) *n_descriptors = b->sets[(size_t)set].n_descriptors;
    if (row0) *row0 = b->set_row[(size_t)set];
    return AKZ_OK;
}

int akz_bank_device(const akz_bank* b, const uint8_t** d_rows, const float** d_x, const float** d_y) {
    if (!b) return refuse("bank_device: null bank");
    if (d_rows) *d_rows = b->d_rows;
    if (d_x) *d_x = b->d_kx;
    if (d_y) *d_y = b->d_ky;
    return AKZ_OK;
}

// (as akz_result_free: a bank may outlive akz_ctx_destroy; the context struct then goes with its last object)
int akz_bank_free(akz_bank* b) {
    if (!b) return AKZ_OK;
    akz_ctx* c = b->ctx;
    (void)hipSetDevice(c->device);
    if (!c->dead) (void)hipStreamSynchronize(c->stream);
    delete b;
    if (--c->live_results == 0 && c->dead) delete c;
    return AKZ_OK;
}

int akz_match_features_seeded_bank_pairs(akz_ctx* c, const akz_bank* bank, const uint64_t* pairs, uint64_t n_pairs,
                                         const akz_ransac_options* options, int cross_check, akz_match* out, uint64_t* n_out, float* model,
                                         int* found, uint32_t* iterations, uint64_t* trials_run) {
    const char* name = "match_features_seeded_bank_pairs: ";
    if (!bank) return refuse(std::string(name) + "null bank");
    return match_seeded_pairs_impl(name, cross_check != 0, c, bank->sets.data(), bank->sets.size(), pairs, n_pairs, bank->desc_bytes, options, out,
                                   n_out, model, found, iterations, trials_run, nullptr, bank);
}

int akz_match_features_seeded_pose_bank_pairs(akz_ctx* c, const akz_bank* bank, const akz_camera* cameras, const uint64_t* pairs,
                                              uint64_t n_pairs, const akz_ransac_options* options, int cross_check, akz_match* out,
                                              uint64_t* n_out, float* model, int* found, uint32_t* iterations, uint64_t* trials_run,
                                              akz_pose* poses, float* points) {
    const char* name = "match_features_seeded_pose_bank_pairs: ";
    if (!bank) return refuse(std::string(name) + "null bank");
    AKZ_TRY(pose_pairs_refusals(name, options, cameras, bank->sets.size(), poses));
    const SeededPose pose{cameras, poses, points};
    return match_seeded_pairs_impl(name, cross_check != 0, c, bank->sets.data(), bank->sets.size(), pairs, n_pairs, bank->desc_bytes, options, out,
                                   n_out, model, found, iterations, trials_run, &pose, bank);
}

int akz_debug_bank_gather(akz_ctx* c, const uint8_t* d_src, uint64_t n_rows, uint64_t desc_bytes, uint8_t* d_dst) {
    if (desc_bytes == 0 || desc_bytes > 64 || n_rows > launch::kBankMaxRows || (n_rows && (!d_src || !d_dst)))
        return refuse("debug_bank_gather: desc_bytes must be 1..64, rows need a source and a destination");
    AKZ_TRY(bind(c));
    // two segments with an empty one between them, so that the hook's table is not the trivial one
    const uint64_t head = n_rows / 2;
    const std::vector<launch::BankSeg> segs = {{d_src, head, 0}, {nullptr, 0, head}, {d_src + head * 64, n_rows - head, head}};
    AKZ_TRY(ensure_pinned(c, c->mp_pin_in, segs.size() * sizeof(launch::BankSeg)));
    AKZ_TRY(bank_gather_enqueue(c, segs, 0, n_rows, desc_bytes, d_dst));
    AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    return AKZ_OK;
}

}  // extern "C"
