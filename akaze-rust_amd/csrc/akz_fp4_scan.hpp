// The FP4 tile walk of the matrix-core Hamming scans, written once: k_match_fp4<COLS> (akz_match.hip: top-2 of every query,
// optionally with the opposite direction's candidates) and k_knn_fp4<K> (akz_knn.hip: the K nearest) are its clients.
//
// Operands are the +-1 images of k_unpack_bits(fp4) / k_unpack_pair_fp4: 256 bytes per row, e2m1 +-1.0 in the 488 columns of
// the 61 descriptor bytes and 0 in the other 24, so <a', b'> = 488 - 2 hamming(a, b), a small integer that is exact in the
// f32 accumulators of v_mfma_scale_f32_32x32x64_f8f6f4 (block scales 1 = E8M0 127; twice the K per instruction and per
// operand byte of the int8 form at the same issue cost).
//
// A workgroup is 1024 threads = 16 waves, four per SIMD; a wave owns 32 queries as the resident B operand (32 registers) and the
// workgroup walks its chunk of the train image in LDS tiles of 128 rows that all waves share.  Operand of lane l (r = l & 31,
// h = l >> 5) at K-step s: bytes 32 s + 16 h .. + 15 of row r, the same function of (l, s) for both operands.  The 32 x 32
// result has its column (query) on the lane and rows lane_row(i) + 4 h in register i: ascending train index inside a lane.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace akz {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

namespace fp4 {

// Threads per workgroup and 32-query blocks per wave are not parameters: 8 waves of 64 queries (every train operand read from
// LDS feeding two matrix instructions) measured 30 % SLOWER at 90 K rows (2.36 against 1.80 ms, profiles/r03_match_variants.txt),
// 12 waves with one or two blocks 2.68 / 2.44 ms, and two 512-thread workgroups per CU no better (profiles/r04_match_mutual.txt):
// the loop is bound by the MFMA pipe and its latency hiding, and wants its 16 waves.
constexpr int NT = 1024;              // threads per workgroup
constexpr int QB = (NT / 64) * 32;    // queries per workgroup
constexpr int SUB = 4;                // 32-row matrix tiles per LDS tile
constexpr int TR = 32 * SUB;          // train rows per LDS tile
constexpr int ROW = 256;              // bytes per unpacked row
constexpr int PITCH = ROW + 16;       // LDS row pitch: 16-byte operand reads of 16 consecutive rows fall into different banks
constexpr int kBits = 488;            // columns that carry +-1 (61 bytes)
constexpr float kPadAcc = -1.0e30f;   // accumulator given to the padding rows of a partial tile (a real one is >= -488)
// Tiles per barrier of the one-direction form (STEP; two LDS buffers of STEP tiles each).  The waves of a workgroup meet at the
// barrier, so a step takes what its slowest wave takes, and what differs between the waves -- exact updates, list insertions --
// averages out over more sub-tiles: 89 816 x 89 816 1596 -> 1557 us, multi-set launch 481 -> 470 us
// (profiles/r04_match_mutual.txt).  The both-direction form keeps one: its limits are a step old when they are used, and two
// tiles cost it 11 spilled registers (8.8 -> 9.6 ms).
constexpr int kStepOneWay = 2;
// Steps staged ahead by the both-direction form (AHEAD; a ring of 2 AHEAD buffers, one barrier per AHEAD steps): the same halving
// of the barriers without the doubled loop body, 7.32 -> 7.17 ms for the all-pairs step of 16 x 4K 5x5 frames
// (profiles/r04_match_mutual.txt); the limits a lane compares with are then two tiles old instead of one.
constexpr int kRingBothWays = 2;

// row of accumulator register i inside a lane's 16 rows of a sub-tile (plus 4 h)
__device__ __forceinline__ unsigned lane_row(int i) { return (unsigned)((i & 3) + 8 * (i >> 2)); }

// A client's chunk: LDS tiles [t_begin, t_end) of the padded train image belong to one set that starts at padded row row0 and
// has n_rows valid rows.
struct Chunk {
    unsigned t_begin, t_end, row0, n_rows;
};

// What a visitor may leave out.  tile_fetch / tile_commit run with the fetch / commit of a tile's first 64-row part (what
// travels with a tile), committed right after the place of a commit (answers of the wave's older memory operations are in).
struct Visitor {
    __device__ __forceinline__ void tile_fetch(unsigned tile, int part) {}
    __device__ __forceinline__ void tile_commit(int buf, int part, unsigned tile) {}
    __device__ __forceinline__ void committed() {}
};

// The resident B operands: the lane's query row q of image q4, eight K-steps of 64 columns, loaded once for the whole chunk.
struct Queries {
    v4i b[8];
};
__device__ __forceinline__ Queries load_queries(const uint8_t* q4, unsigned q, unsigned h) {
    Queries bq;
    const uint8_t* row = q4 + (size_t)q * ROW + 16 * h;
#pragma unroll
    for (int s = 0; s < 8; ++s) bq.b[s] = *reinterpret_cast<const v4i*>(row + 32 * s);
    // pin the operands here: otherwise the waits for these loads are placed at their first use inside the tile loop
#pragma unroll
    for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(bq.b[s]));
    return bq;
}

// Walks chunk ck for the lane's query bq and hands every sub-tile to
//     v.sub_tile(acc, j0, buf, sub)
// acc: 488 - 2 hamming of the lane's query to rows j0 + lane_row(i) of the set (padding rows of a partial tile: kPadAcc);
// buf: the step's LDS buffer, sub: 32-row sub-tile of the step.
// STEP tiles per step and buffer; AHEAD steps staged ahead in a ring of 2 AHEAD buffers, one barrier per AHEAD steps.
template <int STEP, int AHEAD, class V>
__device__ __forceinline__ void walk(const Queries& bq, const uint8_t* t4, const Chunk ck, V& v) {
    static_assert(NT == 1024 && SUB == 4, "staging below: two 64-row parts of 1024 sixteen-byte pieces per 128-row tile");
    constexpr int SUBS = SUB * STEP, NBUF = 2 * AHEAD;
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[NBUF][STEP * TR * PITCH];
    const unsigned tid = threadIdx.x, lane = tid & 63u, r = lane & 31u, h = lane >> 5;
    const unsigned t_begin = ck.t_begin, t_end = ck.t_end, row0 = ck.row0, n1 = ck.n_rows;
    auto op = [](v4i x) { return v8i{x.x, x.y, x.z, x.w, 0, 0, 0, 0}; };  // FP4 operands occupy the first four registers

    // staging: the next step's tiles arrive in 64-row parts (1024 sixteen-byte pieces, one per thread) through one register
    // stage: part p requested before chain 2 p, handed to the other LDS buffer after chain 2 p + 1 has been issued
    const unsigned st_src = (tid >> 4) * ROW + (tid & 15u) * 16u, st_dst = (tid >> 4) * PITCH + (tid & 15u) * 16u;
    uint4 stage;
    auto fetch = [&](unsigned tile, int part) {
        stage = *reinterpret_cast<const uint4*>(t4 + ((size_t)tile * TR + 64u * part) * ROW + st_src);
        if ((part & 1) == 0) v.tile_fetch(tile, part);
    };
    auto commit = [&](int buf, int part, unsigned tile) {
        *reinterpret_cast<uint4*>(&s_tile[buf][64 * part * PITCH + st_dst]) = stage;
        if ((part & 1) == 0) v.tile_commit(buf, part, tile);
    };
#pragma unroll
    for (int ah = 0; ah < AHEAD; ++ah) {
        const unsigned t0 = t_begin + (unsigned)(ah * STEP);
#pragma unroll
        for (int part = 0; part < 2 * STEP; ++part) {
            if (t0 + part / 2 < t_end) {
                fetch(t0, part);
                commit(ah, part, t0);
            }
        }
    }
    __syncthreads();
    for (unsigned tile = t_begin; tile < t_end; tile += STEP) {
        const unsigned step = (tile - t_begin) / STEP;
        const int buf = (int)(step % NBUF), buf_to = (int)((step + AHEAD) % NBUF);
        const unsigned to = tile + AHEAD * STEP;  // the step staged during this one
        // (what exists of a short last step is asked tile by tile against t_end: through min(STEP, t_end - tile) the compiler
        //  keeps a uniform tile counter in a vector register, which costs k_knn_fp4<1> one VGPR: 98 against 97)
#pragma unroll
        for (int sub = 0; sub < SUBS; ++sub) {
            if (sub >= SUB && tile + sub / SUB >= t_end) break;  // (uniform: the last step of a chunk may be short)
            const bool more = to + sub / SUB < t_end;            // part sub / 2 of the step being staged exists
            const bool partial = (tile + (sub / SUB) + 1) * TR - row0 > n1;  // uniform: only the last tile of the set
            if (more && (sub & 1) == 0) fetch(to, sub >> 1);  // in flight under the two chains below
            v16f acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
            const uint8_t* arow = &s_tile[buf][(32 * sub + r) * PITCH + 16 * h];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const v4i a = *reinterpret_cast<const v4i*>(arow + 32 * s);
                acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(op(a), op(bq.b[s]), acc, 4, 4, 0, 127, 0, 127);
            }
            // schedule: three operand reads in flight ahead of the matrix instructions that consume them (an LDS read takes
            // ~100 cycles, an MFMA 32; left alone the scheduler issues read, wait, MFMA, read, wait, ...)
            __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
            for (int s = 0; s < 8 - 3; ++s) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
            // The half tile requested before the previous chain goes to LDS while this chain runs, BEFORE its accumulators
            // are looked at: the wait for the loads is a wait for everything the wave has in flight, the atomics of the
            // opposite direction included (vmcnt counts them for 600..3000 cycles), and here those are a chain or two old.
            // Their answers are in by then too: settled without another wait.
            if ((sub & 1) == 1) {
                if (more) commit(buf_to, sub >> 1, to);
                v.committed();
            }
            const unsigned j0 = tile * TR - row0 + 32 * sub + 4 * h;  // the lane's first row of the sub-tile, inside the set
            if (partial) {  // uniform, the last tile of a set: padding rows never match
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (j0 + lane_row(i) >= n1) acc[i] = kPadAcc;
            }
            v.sub_tile(acc, j0, buf, sub);
        }
        if (AHEAD == 1 || step % AHEAD == AHEAD - 1 || tile + STEP >= t_end) __syncthreads();  // (uniform)
    }
}

}  // namespace fp4
}  // namespace akz
