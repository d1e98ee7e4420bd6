// The top-2 rule of descriptor_match (akaze/src/ops/feature_matching.rs:37-81), stated ONCE for every kernel and host form of
// the matcher:
//   * both distances start at the threshold;
//   * updates are strict '<' in ascending row order, so the lowest row wins among equal minima (:41-49);
//   * an equal distance lowers the second;
//   * a record is kept iff (double)min < (double)second * ratio^2 && min < threshold (:61-63).
// The sequential form (feed) is the statement.  The two other forms -- fold, for the records of chunks that come in ascending
// row order, and merge_disjoint, for two states over disjoint row sets in any order -- are proved equal to it at the bottom of
// this header, at compile time, in the host and in the device pass.  What the matrix kernels do per tile (batched updates from
// a tile's two best rows, akz_match.hip) is another algorithm with tests of its own; only its epilogue meets this rule.
// (akz_internal.hpp comes along for MatchRec and akz_match alone; the proof costs every includer one constexpr evaluation
// per pass, a few thousand steps.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "akz_internal.hpp"

#if defined(__HIPCC__)
#define AKZ_RULE __host__ __device__ constexpr
#else
#define AKZ_RULE constexpr
#endif

namespace akz {

// (min, second, argmin) of one query over the rows seen so far; Index: u32 on the device, u64 for the host scans
template <class Index>
struct NearestTwoOf {
    uint32_t min_d, second;
    Index min_j;

    static AKZ_RULE NearestTwoOf start(uint32_t threshold) { return NearestTwoOf{threshold, threshold, 0}; }
    // the next row in ascending order (:41-49)
    AKZ_RULE void feed(uint32_t d, Index j) {
        if (d < min_d) {
            second = min_d;
            min_d = d;
            min_j = j;
        } else if (d < second) {
            second = d;
        }
    }
    // the record of the next chunk in ascending row order: feed of its minimum, then of its second, which can only lower the
    // second (second_d >= min_d of its chunk >= min_d)
    AKZ_RULE void fold(MatchRec r) {
        feed(r.min_d, (Index)r.min_j);
        if (r.second_d < second) second = r.second_d;
    }
    // a state over OTHER rows, in any order: (distance, row) lexicographic minimum; second = the smallest of the rest.  (Rows
    // at the threshold never entered either state: their min_j is no row.)
    AKZ_RULE void merge_disjoint(const NearestTwoOf& o, uint32_t threshold) {
        if (o.min_d < min_d || (o.min_d == min_d && o.min_d < threshold && o.min_j < min_j)) {
            second = o.second < min_d ? o.second : min_d;
            min_d = o.min_d;
            min_j = o.min_j;
        } else {
            second = second < o.min_d ? second : o.min_d;
        }
    }
    // Lowe's ratio test on squared ratio, in f64, and the threshold (:61-63)
    AKZ_RULE bool accepted(double ratio2, uint32_t threshold) const { return (double)min_d < (double)second * ratio2 && min_d < threshold; }
    AKZ_RULE MatchRec record() const { return MatchRec{min_d, second, (uint32_t)min_j, 0u}; }
};
using NearestTwo = NearestTwoOf<uint32_t>;

// ---- host only ------------------------------------------------------------------------------------------------------
// Hamming distance of two rows of desc_bytes bytes
inline uint32_t hamming_bytes(const uint8_t* a, const uint8_t* b, uint64_t desc_bytes) {
    uint32_t d = 0;
    uint64_t t = 0;
    for (; t + 8 <= desc_bytes; t += 8) {
        uint64_t wa, wb;
        std::memcpy(&wa, a + t, 8);
        std::memcpy(&wb, b + t, 8);
        d += (uint32_t)__builtin_popcountll(wa ^ wb);
    }
    for (; t < desc_bytes; ++t) d += (uint32_t)__builtin_popcount((unsigned)(a[t] ^ b[t]));
    return d;
}
// the kernels hold distances and the threshold in 32 bits; no distance reaches 2^31 - 1
inline uint32_t clamp_threshold(uint64_t t) { return (uint32_t)std::min<uint64_t>(t, 0x7fffffffull); }

// descriptor_match on the host: every row of d0 against the rows j of d1 with gate(i, j), in ascending j; the kept records go
// to emit(record) in row order.  A row that fails the gate is a row that is not there.
template <class Gate, class Emit>
void host_match_scan(const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes, uint32_t thr, double ratio2,
                     Gate gate, Emit emit) {
    for (uint64_t i = 0; i < n0; ++i) {
        auto best = NearestTwoOf<uint64_t>::start(thr);
        for (uint64_t j = 0; j < n1; ++j)
            if (gate(i, j)) best.feed(hamming_bytes(d0 + i * desc_bytes, d1 + j * desc_bytes, desc_bytes), j);
        if (best.accepted(ratio2, thr)) emit(akz_match{i, best.min_j, (double)best.min_d});
    }
}

// ---- the proof ------------------------------------------------------------------------------------------------------
// Every sequence of 0..3 rows with distances from {0, 1, 2, thr, thr + 1} at thr = 3 (two and three rows reach the tie clause
// and the triple ties): every cut into up to three ascending chunks, empty ones included, folded with fold, and every
// assignment of the rows to two lanes merged with merge_disjoint in both argument orders give the state of the sequential feed.
namespace rule_proof {
constexpr uint32_t kThr = 3;
AKZ_RULE bool same(const NearestTwo& a, const NearestTwo& b) { return a.min_d == b.min_d && a.second == b.second && a.min_j == b.min_j; }
// sequential feed of the rows lo .. hi - 1 whose bit is set in mask
AKZ_RULE NearestTwo scan(const uint32_t (&d)[3], unsigned lo, unsigned hi, unsigned mask) {
    NearestTwo s = NearestTwo::start(kThr);
    for (unsigned j = lo; j < hi; ++j)
        if ((mask >> j) & 1u) s.feed(d[j], j);
    return s;
}
AKZ_RULE bool holds_for(const uint32_t (&d)[3], unsigned n) {
    const NearestTwo whole = scan(d, 0, n, ~0u);
    for (unsigned c1 = 0; c1 <= n; ++c1)
        for (unsigned c2 = c1; c2 <= n; ++c2) {
            NearestTwo s = NearestTwo::start(kThr);
            s.fold(scan(d, 0, c1, ~0u).record());
            s.fold(scan(d, c1, c2, ~0u).record());
            s.fold(scan(d, c2, n, ~0u).record());
            if (!same(s, whole)) return false;
        }
    for (unsigned mask = 0; mask < (1u << n); ++mask) {
        const NearestTwo a = scan(d, 0, n, mask), b = scan(d, 0, n, ~mask);
        NearestTwo ab = a, ba = b;
        ab.merge_disjoint(b, kThr);
        ba.merge_disjoint(a, kThr);
        if (!same(ab, whole) || !same(ba, whole)) return false;
    }
    return true;
}
AKZ_RULE bool holds() {
    const uint32_t dist[5] = {0, 1, 2, kThr, kThr + 1};
    for (unsigned n = 0, count = 1; n <= 3; ++n, count *= 5)
        for (unsigned code = 0; code < count; ++code) {
            const uint32_t d[3] = {dist[code % 5], dist[code / 5 % 5], dist[code / 25 % 5]};
            if (!holds_for(d, n)) return false;
        }
    return true;
}
static_assert(holds(), "fold and merge_disjoint must equal the sequential feed");
}  // namespace rule_proof

}  // namespace akz

#undef AKZ_RULE
