// Feature banks (additions; include/akaze_hip.h): feature sets kept on the device in the layout the pairs calls scan,
// so that extraction results reach the seeded pairs calls without a round trip through host memory and sets that are matched again
// are placed once.  akz_bank_create_from_results: bank_segments (the table, plain host code), x / y from the results' host
// keypoints through pinned staging, and launch::bank_gather (akz_bank.hip) -- ONE launch -- over the results' device rows.
// akz_bank_create_from_sets: the packing and the copies of pairs_upload (akz_match_api.cpp) into the bank's block.  The two bank
// forms of the seeded pairs calls are those calls with the bank in their PairsCall (akz_match_seeded_api.cpp).  A bank's block and
// the context's staging are SetsBlocks (akz_pairs_layout.hpp), every set placed in index order.
// The two constructors under a keypoint budget (bank_create_budgeted): the budget's plan / enqueue half (budget_enqueue,
// akz_budget_api.cpp) leaves every set's kept indices on the device, and launch::bank_select -- ONE launch -- gathers rows, x and y
// through them, from the results' row blocks or from the full sets that pairs_upload put into the context's staging.
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
// the block of the bank's sets, every set behind the one before it (with_src: with the source indices of a budgeted bank)
int bank_alloc(akz_ctx* c, akz_bank* b, bool with_src = false) {
    b->block.place(b->sets.data(), b->sets.size(), index_order(b->sets.size()));
    AKZ_HIP_TRY(b->dev.acquire(b->block.bytes(with_src), false));
    AKZ_HIP_TRY(alloc_fill(c, b->dev.p, b->dev.bytes));
    b->block.bind(b->dev.p, with_src);
    return AKZ_OK;
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
    AKZ_TRY(table_upload(c, c->mp_tab.p, (char*)c->mp_pin_in.p + pin_off, segs.data(), b_tab));
    StageTimer t(c, kStageIngest, st);
    t.kernel(AKZ_KR_BANK_GATHER, (uint32_t)desc_bytes, 64, (uint32_t)std::min<uint64_t>(rows, 0xffffffffull), (uint32_t)segs.size(), 1, rows);
    launch::bank_gather(st, (const launch::BankSeg*)c->mp_tab.p, (uint32_t)segs.size(), rows, (uint32_t)desc_bytes, d_dst);
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}
// the refusals of the constructors from results (`name` ends in ": "); rows: the keypoints of all images
int results_refusals(const std::string& name, const akz_ctx* c, const akz_result* const* results, uint64_t n_results, akz_bank** out,
                     uint64_t& rows) {
    if (!c || !results || !out) return refuse(name + "null context, results or out");
    if (n_results == 0) return refuse(name + "no result (the descriptor size of a bank is that of its results)");
    uint64_t images = 0;
    rows = 0;
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
    return AKZ_OK;
}
// the selection table through pinned staging (`pin_off` bytes into c->mp_pin_in, as above) to c->mp_tab, then the one launch of
// k_bank_select, on the context's stream (not synchronised)
int bank_select_enqueue(akz_ctx* c, const std::vector<launch::BankSel>& tab, size_t pin_off, uint64_t rows, uint64_t desc_bytes,
                        const uint32_t* d_idx, const float* d_sx, const float* d_sy, uint8_t* d_rows, float* d_x, float* d_y, uint32_t* d_index) {
    if (tab.empty() || rows == 0) return AKZ_OK;
    hipStream_t st = c->stream;
    const size_t b_tab = tab.size() * sizeof(launch::BankSel);
    AKZ_TRY(ensure(c, c->mp_tab, b_tab));
    AKZ_TRY(table_upload(c, c->mp_tab.p, (char*)c->mp_pin_in.p + pin_off, tab.data(), b_tab));
    StageTimer t(c, kStageIngest, st);
    t.kernel(AKZ_KR_BANK_SELECT, (uint32_t)desc_bytes, 64, (uint32_t)std::min<uint64_t>(rows, 0xffffffffull), (uint32_t)tab.size(), 1, rows);
    launch::bank_select(st, (const launch::BankSel*)c->mp_tab.p, (uint32_t)tab.size(), rows, (uint32_t)desc_bytes, d_idx, d_sx, d_sy, d_rows, d_x,
                        d_y, d_index);
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}
// What the two budgeted constructors share, behind their refusals and bind: the bank of min(max_keypoints, n) rows per set, the
// budget (budget_enqueue: its ONE upload carries x, y and response, so the bank's x / y are gathered, not uploaded again), the one
// k_bank_select from src_rows[s] (set s's rows on the device, 64 bytes each; `place`, given, enqueues what puts them there), the
// kept indices to the host and the call's one synchronisation.  sets: only keypoints / n_keypoints are read.  The selection
// table goes `pin_off` bytes into c->mp_pin_in, which holds at least pin_off + 40 bytes per set.
template <typename Place>
int bank_create_budgeted(akz_ctx* c, const std::vector<akz_feature_set>& sets, const std::vector<const uint8_t*>& src_rows, uint64_t desc_bytes,
                         const akz_keypoint_budget& o, size_t pin_off, Place place, akz_bank** out) {
    std::unique_ptr<akz_bank> b(new akz_bank);
    b->desc_bytes = desc_bytes;
    b->budgeted = true;
    for (const akz_feature_set& s : sets) {
        const uint64_t keep = std::min<uint64_t>(o.max_keypoints, s.n_keypoints);
        b->sets.push_back(akz_feature_set{nullptr, keep, nullptr, keep});
    }
    AKZ_TRY(bank_alloc(c, b.get(), true));
    const SetsBlock& blk = b->block;
    const uint64_t rows = blk.rows;
    AKZ_TRY(place());
    BudgetPlan p;
    AKZ_TRY(budget_enqueue(c, sets.data(), sets.size(), o, p));
    std::vector<launch::BankSel> tab;
    for (size_t s = 0; s < sets.size(); ++s)
        tab.push_back(launch::BankSel{p.tab[s].keep ? src_rows[s] : nullptr, p.tab[s].base, p.tab[s].keep, blk.set_row[s], p.tab[s].out_off});
    AKZ_TRY(bank_select_enqueue(c, tab, pin_off, rows, desc_bytes, p.d_idx, p.d_x, p.d_y, blk.d_rows, blk.d_kx, blk.d_ky, blk.d_src));
    hipStream_t st = c->stream;
    if (rows) AKZ_HIP_TRY(hipMemcpyAsync(p.h_down, blk.d_src, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
    AKZ_HIP_TRY(hipStreamSynchronize(st));  // complete on return: the sources may go
    if (rows) b->src.assign((const uint32_t*)p.h_down, (const uint32_t*)p.h_down + rows);
    *out = bank_keep(c, b);
    return AKZ_OK;
}
}  // namespace

extern "C" {

int akz_bank_create_from_results(akz_ctx* c, const akz_result* const* results, uint64_t n_results, akz_bank** out) {
    const std::string name = "bank_create_from_results: ";
    if (out) *out = nullptr;
    uint64_t rows = 0;
    AKZ_TRY(results_refusals(name, c, results, n_results, out, rows));
    AKZ_TRY(bind(c));
    std::unique_ptr<akz_bank> b(new akz_bank);
    b->desc_bytes = result_desc_bytes(results[0]);
    std::vector<launch::BankSeg> segs;
    bank_segments(results, n_results, segs);
    for (const launch::BankSeg& s : segs) b->sets.push_back(akz_feature_set{nullptr, s.n_rows, nullptr, s.n_rows});
    AKZ_TRY(bank_alloc(c, b.get()));
    // x | y of every keypoint, then the table, in pinned memory: one copy each
    const size_t b_xy = b->block.b_xy;
    AKZ_TRY(ensure_pinned(c, c->mp_pin_in, 2 * b_xy + segs.size() * sizeof(launch::BankSeg)));
    float *hx = (float*)c->mp_pin_in.p, *hy = (float*)((char*)c->mp_pin_in.p + b_xy);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n_results; ++i)
        for (const auto& kps : results[i]->kps)
            for (const akz_keypoint& k : kps) hx[at] = k.x, hy[at] = k.y, ++at;
    hipStream_t st = c->stream;
    if (rows) {
        AKZ_HIP_TRY(hipMemcpyAsync(b->block.d_kx, hx, (size_t)rows * 4, hipMemcpyHostToDevice, st));
        AKZ_HIP_TRY(hipMemcpyAsync(b->block.d_ky, hy, (size_t)rows * 4, hipMemcpyHostToDevice, st));
    }
    AKZ_TRY(bank_gather_enqueue(c, segs, 2 * b_xy, rows, b->desc_bytes, b->block.d_rows));
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
    for (uint64_t k = 0; k < n_sets; ++k)
        if (const char* why = set_refusal(sets[k])) return refuse(name + "set " + std::to_string(k) + ": " + why);
    if (!c) return refuse(name + "null context");
    AKZ_TRY(bind(c));
    std::unique_ptr<akz_bank> b(new akz_bank);
    b->desc_bytes = desc_bytes;
    for (uint64_t k = 0; k < n_sets; ++k) b->sets.push_back(akz_feature_set{nullptr, sets[k].n_keypoints, nullptr, sets[k].n_descriptors});
    AKZ_TRY(bank_alloc(c, b.get()));
    AKZ_TRY(ensure_pinned(c, c->mp_pin_in, b->block.bytes(false)));
    if (b->block.rows) AKZ_TRY(pairs_upload(c, sets, desc_bytes, b->block, index_order(n_sets)));
    AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    *out = bank_keep(c, b);
    return AKZ_OK;
}

int akz_bank_create_from_results_budget(akz_ctx* c, const akz_result* const* results, uint64_t n_results, const akz_keypoint_budget* budget,
                                        akz_bank** out) {
    const std::string name = "bank_create_from_results_budget: ";
    if (out) *out = nullptr;
    if (out && !budget_options_ok(name.c_str(), budget, out, out, nullptr)) return AKZ_ERR_INVALID_ARG;  // (no indices, n_out or radius2 here)
    uint64_t rows = 0;
    AKZ_TRY(results_refusals(name, c, results, n_results, out, rows));
    if (rows > kBudgetMaxKeypoints) return refuse(name + "the results hold more than 2^31 - 1 keypoints together");
    std::vector<akz_feature_set> sets;
    std::vector<const uint8_t*> src_rows;
    for (uint64_t i = 0; i < n_results; ++i) {
        const akz_result* r = results[i];
        for (uint32_t img = 0; img < r->n; ++img) {
            const std::vector<akz_keypoint>& k = r->kps[img];
            if (!budget_set_ok(name.c_str(), "result " + std::to_string(i) + " image " + std::to_string(img) + ": ", k.data(), k.size()))
                return AKZ_ERR_INVALID_ARG;
            sets.push_back(akz_feature_set{k.data(), k.size(), nullptr, 0});
            src_rows.push_back(k.empty() ? nullptr : r->d_desc64 + r->desc_off[img] * 64);
        }
    }
    AKZ_TRY(bind(c));
    AKZ_TRY(ensure_pinned(c, c->mp_pin_in, sets.size() * sizeof(launch::BankSel)));
    return bank_create_budgeted(c, sets, src_rows, result_desc_bytes(results[0]), *budget, 0, [] { return (int)AKZ_OK; }, out);
}

int akz_bank_create_from_sets_budget(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, uint64_t desc_bytes,
                                     const akz_keypoint_budget* budget, akz_bank** out) {
    const std::string name = "bank_create_from_sets_budget: ";
    if (out) *out = nullptr;
    if (!out) return refuse(name + "null out");
    if (desc_bytes == 0 || desc_bytes > 64) return refuse(name + "desc_bytes must be 1..64");
    if (n_sets && !sets) return refuse(name + "null sets");
    if (!budget_options_ok(name.c_str(), budget, out, out, nullptr)) return AKZ_ERR_INVALID_ARG;
    uint64_t rows = 0;
    for (uint64_t k = 0; k < n_sets; ++k) {
        const akz_feature_set& s = sets[k];
        const std::string at = "set " + std::to_string(k) + ": ";
        if (s.n_descriptors != s.n_keypoints)
            return refuse(name + at + std::to_string(s.n_descriptors) + " descriptors for " + std::to_string(s.n_keypoints) +
                          " keypoints (the budget is defined over keypoints that all have a row)");
        if (const char* why = set_refusal(s)) return refuse(name + at + why);  // (null pointers: the counts are equal)
        if (!budget_set_ok(name.c_str(), at, s.keypoints, s.n_keypoints)) return AKZ_ERR_INVALID_ARG;
        rows += s.n_descriptors;
        if (rows > kBudgetMaxKeypoints) return refuse(name + at + "the sets of one call hold more than 2^31 - 1 keypoints together");
    }
    if (!c) return refuse(name + "null context");
    AKZ_TRY(bind(c));
    // the FULL sets to the context's staging, every set in index order
    const std::vector<uint64_t> order = index_order(n_sets);
    SetsBlock full;
    full.place(sets, n_sets, order);
    AKZ_TRY(ensure(c, c->mp_in, full.bytes(false)));
    AKZ_TRY(ensure_pinned(c, c->mp_pin_in, full.bytes(false) + (size_t)n_sets * sizeof(launch::BankSel)));
    full.bind(c->mp_in.p, false);
    std::vector<const uint8_t*> src_rows;
    for (uint64_t k = 0; k < n_sets; ++k) src_rows.push_back(full.d_rows + full.set_row[(size_t)k] * 64);
    const std::vector<akz_feature_set> all(sets, sets + n_sets);
    return bank_create_budgeted(c, all, src_rows, desc_bytes, *budget, full.bytes(false),
                                [&] { return rows ? pairs_upload(c, sets, desc_bytes, full, order) : (int)AKZ_OK; }, out);
}

int akz_bank_set_indices(const akz_bank* b, uint64_t set, uint64_t* indices) {
    if (!b) return refuse("bank_set_indices: null bank");
    if (set >= b->sets.size()) return refuse("bank_set_indices: set index " + std::to_string(set) + " >= n_sets " + std::to_string(b->sets.size()));
    const uint64_t n = b->sets[(size_t)set].n_keypoints, row0 = b->block.set_row[(size_t)set];
    if (n && !indices) return refuse("bank_set_indices: null indices for a set of " + std::to_string(n) + " keypoints");
    for (uint64_t t = 0; t < n; ++t) indices[t] = b->budgeted ? b->src[(size_t)(row0 + t)] : t;
    return AKZ_OK;
}

int akz_bank_info(const akz_bank* b, uint64_t* n_sets, uint64_t* desc_bytes, uint64_t* rows) {
    if (!b) return refuse("bank_info: null bank");
    if (n_sets) *n_sets = b->sets.size();
    if (desc_bytes) *desc_bytes = b->desc_bytes;
    if (rows) *rows = b->block.rows;
    return AKZ_OK;
}

int akz_bank_set_info(const akz_bank* b, uint64_t set, uint64_t* n_keypoints, uint64_t* n_descriptors, uint64_t* row0) {
    if (!b) return refuse("bank_set_info: null bank");
    if (set >= b->sets.size()) return refuse("bank_set_info: set index " + std::to_string(set) + " >= n_sets " + std::to_string(b->sets.size()));
    if (n_keypoints) *n_keypoints = b->sets[(size_t)set].n_keypoints;
    if (n_descriptors) *n_descriptors = b->sets[(size_t)set].n_descriptors;
    if (row0) *row0 = b->block.set_row[(size_t)set];
    return AKZ_OK;
}

int akz_bank_device(const akz_bank* b, const uint8_t** d_rows, const float** d_x, const float** d_y) {
    if (!b) return refuse("bank_device: null bank");
    if (d_rows) *d_rows = b->block.d_rows;
    if (d_x) *d_x = b->block.d_kx;
    if (d_y) *d_y = b->block.d_ky;
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
    return match_seeded_pairs_impl({name, c, bank->sets.data(), bank->sets.size(), pairs, n_pairs, bank->desc_bytes, out, n_out, bank}, cross_check != 0,
                                   options, model, found, iterations, trials_run);
}

int akz_match_features_seeded_pose_bank_pairs(akz_ctx* c, const akz_bank* bank, const akz_camera* cameras, const uint64_t* pairs,
                                              uint64_t n_pairs, const akz_ransac_options* options, int cross_check, akz_match* out,
                                              uint64_t* n_out, float* model, int* found, uint32_t* iterations, uint64_t* trials_run,
                                              akz_pose* poses, float* points) {
    const char* name = "match_features_seeded_pose_bank_pairs: ";
    if (!bank) return refuse(std::string(name) + "null bank");
    AKZ_TRY(pose_pairs_refusals(name, options, cameras, bank->sets.size(), poses));
    const SeededPose pose{cameras, poses, points};
    return match_seeded_pairs_impl({name, c, bank->sets.data(), bank->sets.size(), pairs, n_pairs, bank->desc_bytes, out, n_out, bank}, cross_check != 0,
                                   options, model, found, iterations, trials_run, &pose);
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

int akz_debug_bank_select(akz_ctx* c, const uint8_t* d_src, const float* d_sx, const float* d_sy, uint64_t n_sets, const uint64_t* n,
                          const uint64_t* keep, const uint32_t* indices, uint64_t desc_bytes, uint8_t* d_rows, float* d_x, float* d_y,
                          uint32_t* d_index) {
    const std::string name = "debug_bank_select: ";
    if (desc_bytes == 0 || desc_bytes > 64) return refuse(name + "desc_bytes must be 1..64");
    if (n_sets > 0xfffffff0ull || (n_sets && (!n || !keep))) return refuse(name + "null counts, or too many sets");
    // the table: the caller's sets, their sources packed one behind the other, between two empty records of the hook's own
    std::vector<launch::BankSel> tab = {{nullptr, 0, 0, 0, 0}};
    uint64_t base = 0, rows = 0;
    for (uint64_t s = 0; s < n_sets; ++s) {
        const std::string at = name + "set " + std::to_string(s) + ": ";
        if (keep[s] > n[s] || n[s] > 0xffffffffull) return refuse(at + "keep " + std::to_string(keep[s]) + " of " + std::to_string(n[s]) + " rows");
        if (keep[s] && !indices) return refuse(at + "null indices");
        for (uint64_t t = 0; t < keep[s]; ++t) {
            const uint32_t i = indices[rows + t];
            if (i >= n[s]) return refuse(at + "index " + std::to_string(i) + " reaches the set's " + std::to_string(n[s]) + " rows");
            if (t && i <= indices[rows + t - 1]) return refuse(at + "the indices do not ascend at entry " + std::to_string(t));
        }
        tab.push_back(launch::BankSel{keep[s] ? d_src + base * 64 : nullptr, base, keep[s], rows, rows});
        base += n[s];
        rows += keep[s];
    }
    tab.push_back(launch::BankSel{nullptr, base, 0, rows, rows});
    if (rows > launch::kBankMaxRows || (rows && (!d_src || !d_sx || !d_sy || !d_rows || !d_x || !d_y || !d_index)))
        return refuse(name + "rows need sources and destinations");
    AKZ_TRY(bind(c));
    if (rows == 0) return AKZ_OK;
    // table | indices in pinned memory; the indices pass through the budget's device scratch, where launch::budget leaves its own
    const size_t b_tab = up256(tab.size() * sizeof(launch::BankSel));
    AKZ_TRY(ensure_pinned(c, c->mp_pin_in, b_tab + (size_t)rows * 4));
    AKZ_TRY(ensure(c, c->kb_dev, (size_t)rows * 4));
    uint32_t* h_idx = (uint32_t*)((char*)c->mp_pin_in.p + b_tab);
    std::memcpy(h_idx, indices, (size_t)rows * 4);
    AKZ_HIP_TRY(hipMemcpyAsync(c->kb_dev.p, h_idx, (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
    AKZ_TRY(bank_select_enqueue(c, tab, 0, rows, desc_bytes, (const uint32_t*)c->kb_dev.p, d_sx, d_sy, d_rows, d_x, d_y, d_index));
    AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    return AKZ_OK;
}

}  // extern "C"
