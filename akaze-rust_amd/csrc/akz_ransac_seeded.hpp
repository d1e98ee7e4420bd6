// The statement of the seeded RANSAC (akz_remove_outliers_seeded, akz_match_features_seeded_pairs; include/akaze_hip.h,
// DESIGN.md 8), shared by the host statement, the orchestration and the trial kernel: a counter-based generator, the sample of
// a trial as a pure function of (seed, stream, trial), and the number of inliers that stops a pair.  Integer arithmetic only
// (u64, wrapping) for everything the device evaluates: host, device and a restatement in another language give the same bits.
#pragma once
#include <cstdint>

#include "akz_fmatrix.hpp"  // AKZ_HD, AKZ_UNROLL

namespace akz {

constexpr uint32_t AKZ_RANSAC_ROUND = 128;         // trials per round; the stopping rule is evaluated after each round
constexpr uint64_t kSeededMaxTrials = 1ull << 24;  // max_trials above it is refused
constexpr uint64_t kSeededGolden = 0x9E3779B97F4A7C15ull;

AKZ_HD uint64_t seeded_mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// k1 of the statement: the part of the key that every stream of a seed shares
AKZ_HD uint64_t seeded_seed_key(uint64_t seed0, uint64_t seed1) {
    const uint64_t k0 = seeded_mix64(seed0 + kSeededGolden);
    return seeded_mix64(seed1 ^ k0);
}
// ks: the key of one stream (pair p of a call: stream_base + p)
AKZ_HD uint64_t seeded_stream_key(uint64_t k1, uint64_t stream) { return seeded_mix64(k1 + kSeededGolden * (stream + 1)); }
// v(t, i): draw i < K of trial t
AKZ_HD uint64_t seeded_draw(uint64_t ks, uint64_t trial, int i) { return seeded_mix64(ks + kSeededGolden * (8 * trial + (uint64_t)i + 1)); }
AKZ_HD uint64_t seeded_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// The sample of trial `trial` over n >= K matches: K distinct indices below n in ascending order.  Floyd's algorithm: exactly K
// draws, no rejection, every K-subset equally likely (up to the 2^-64 bias of the multiply-shift range reduction).
template <int K, class T>
AKZ_HD void seeded_sample(uint64_t ks, uint64_t trial, uint64_t n, T (&out)[K]) {
    uint64_t picked[K];
AKZ_UNROLL
    for (int i = 0; i < K; ++i) {
        const uint64_t j = n - (uint64_t)K + (uint64_t)i;
        uint64_t r = seeded_mulhi(seeded_draw(ks, trial, i), j + 1);  // uniform in 0 .. j
        bool dup = false;
AKZ_UNROLL
        for (int k = 0; k < K; ++k) dup = dup || (k < i && picked[k] == r);
        if (dup) r = j;  // (j is larger than everything picked so far)
        // insertion into the ascending list
        uint64_t carry = r;
AKZ_UNROLL
        for (int k = 0; k < K; ++k)
            if (k < i && picked[k] > carry) {
                const uint64_t t = picked[k];
                picked[k] = carry;
                carry = t;
            }
        picked[i] = carry;
    }
AKZ_UNROLL
    for (int i = 0; i < K; ++i) out[i] = (T)picked[i];
}

#if !defined(__HIP_DEVICE_COMPILE__)
// powi(1 - powi(b / n, K), T) <= 1 - confidence, in f64 without contraction: powi(w, K) by K - 1 successive multiplications,
// powi(q, T) by binary exponentiation
inline bool seeded_enough(uint64_t b, uint64_t n, int K, uint64_t T, double confidence) {
    const double w = (double)b / (double)n;
    double wk = w;
    for (int i = 1; i < K; ++i) wk = wk * w;
    double q = 1.0 - wk, res = 1.0;
    while (T) {
        if (T & 1) res = res * q;
        T >>= 1;
        if (T) q = q * q;
    }
    return res <= 1.0 - confidence;
}
// need(n, K, T, confidence): the smallest b in 1 .. n that is enough after T >= 1 trials, for 0 < confidence < 1 (b = n always
// is: w = 1, q = 0).  Evaluated on the host only -- by the host statement and by the orchestration of the GPU call, which hands
// the device a table of integers.  The test is monotone in b as computed, not only in exact arithmetic: a correctly rounded
// quotient, product or difference is monotone in each non-negative operand, and every step above is one of those on values
// in [0, 1] -- so bisection finds the smallest b of a linear scan.
inline uint64_t seeded_need(uint64_t n, int K, uint64_t T, double confidence) {
    uint64_t lo = 1, hi = n;  // (hi is enough)
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (seeded_enough(mid, n, K, T, confidence)) hi = mid;
        else lo = mid + 1;
    }
    return hi;
}
// The rounds of the statement over n >= K elements, for every model of the family (seeded_host of akz_ransac_seeded.cpp, the
// resection of akz_resection_api.cpp): trial(sample) evaluates the model of a sample and returns its inlier count, below 0 where
// the sample has no model; won() is called when that trial has become the winner -- strictly more inliers than every trial
// before it, from 0.  Rounds of AKZ_RANSAC_ROUND trials; after each round the stopping rule, where confidence > 0.
template <int K, class Trial, class Won>
inline void seeded_rounds(uint64_t n, uint64_t seed0, uint64_t seed1, uint64_t stream, uint64_t max_trials, double confidence, Trial trial,
                          Won won, int64_t& best, uint64_t& trials_run) {
    const uint64_t ks = seeded_stream_key(seeded_seed_key(seed0, seed1), stream);
    best = 0;
    trials_run = 0;
    while (trials_run < max_trials) {
        const uint64_t end = max_trials - trials_run < AKZ_RANSAC_ROUND ? max_trials : trials_run + AKZ_RANSAC_ROUND;
        for (uint64_t t = trials_run; t < end; ++t) {
            uint64_t smp[K];
            seeded_sample<K>(ks, t, n, smp);
            const int64_t inl = trial(smp);
            if (inl > best) {  // (strict: the first trial that reached the count stays the winner)
                best = inl;
                won();
            }
        }
        trials_run = end;
        if (confidence > 0.0 && (uint64_t)best >= seeded_need(n, K, trials_run, confidence)) break;
    }
}
#endif

}  // namespace akz
