// One pass over an image plane that leaves ONE row of fp32 sums per block, and the fixed-order sum of those rows: the shape the
// trainer's fused loss and regulariser kernels share (depth_smooth.hip, reproj.hip, train.hip; the host helpers serve exposure.hip,
// mcmc.hip and depth_loss.hip as well).  The tests compare losses and gradients bit for bit; what makes that hold is stated here
// once: every addition has a fixed place in a fixed order, and the grid depends on the shape alone.
//
// GROUPS.  Work is dealt in groups of four consecutive pixels of one row (G = ceil(W / 4) groups per row, the last one ragged when
// W % 4), group q = y G + gx, one group per thread and trip.
// GRID RULE.  blocks = clamp(ceil(groups / threads), 1, max_blocks) (pass_blocks), a grid-stride loop beyond: with 256 threads and
// 1024 blocks a second trip from 262144 groups on.  The grid is a function of the shape alone, so a thread's running sums, a block's
// row and the sum of the rows are the same additions in the same order from call to call.  plane_walk hands block b the chunk of
// groups xcd_remap(b): the rows above and below a group sit in the same XCD's L2.
// VEC.  W % 4 == 0 and every plane pointer 16-byte aligned (aligned16): a group of a plane is one aligned 16-byte access; else four
// scalar accesses.  All loads of a trip are UNCONDITIONAL: an index past a border is clamped to the border and the value dropped by
// a select afterwards, never multiplied by zero, so that the loads are requested together, not one wait each (README round 6; a
// load behind its own `inside ? load : 0` branch waits for the one before it, photo_loss.hip's photo_load20).  After the loads both
// paths run the same arithmetic: the same bits.
// SUMS.  A thread keeps fp32 running sums, left to right.  block_rows adds them over the wave (wave_sum's butterfly) and over the
// block's four waves as (w0 + w1) + (w2 + w3) (block_sum4); they leave as one row per block.  combine_rows adds up to 1024 rows in
// fp64: thread t takes rows t, t + 256, t + 512, t + 768 in that order, then the butterfly and the four waves as above.
// SEPARATE ON PURPOSE: k_exposure_finish (1024 threads, column groups), k_mcmc_reg_finish (1024 threads, waves in sequence),
// k_l1_final and photo_final (a stride-256 loop over more rows than four per thread), dc_block_merge and dl_block_sum (moments, not
// sums) add in other orders; moving them here would change the order of their fp64 additions and with it output bits.
// k_exposure_pass and k_mcmc_reg_pass add in block_rows' order but thread k stores column k of a row that is no float4, and
// exposure.hip walks flat planes with 64-bit indices: they keep their device code, which compiled differently on these helpers.
// CONTRACTION.  These helpers only add, select and move: there is no product next to a sum for the compiler to contract, so they
// give the same bits with and without -ffp-contract=off and need no `#pragma clang fp contract(off)` (common.h's act_* do).  The
// arithmetic a caller runs between load4 and store4 is the caller's: the files above are built without contraction (build.py
// STRICT_FP) or, like depth_loss.hip, use the host helpers alone.
#pragma once
#include "common.h"
#include <utility>

namespace syn3r {

constexpr int kPassThreads = 256;            // block_rows, combine_rows: four waves
constexpr int kPassMaxBlocks = 1024;         // combine_rows: four rows per thread

// ---------------------------------------------------------------------------------------------------------------------- device
// The four values of row y of plane p [H, W] at columns x0 .. x0 + 3 (scalar path: a column past W - 1 reads column W - 1).
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ p, int y, int x0, int W) {
    const float* r = p + (size_t)y * (size_t)W;
    if constexpr (VEC) {
        return *(const float4*)(r + x0);
    } else {
        const int l = W - 1;
        return make_float4(r[x0], r[x0 + 1 < l ? x0 + 1 : l], r[x0 + 2 < l ? x0 + 2 : l], r[x0 + 3 < l ? x0 + 3 : l]);
    }
}
// p[y, x0 + k] = v[k] for every x0 + k < W
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, int y, int x0, int W, float4 v) {
    float* r = p + (size_t)y * (size_t)W + x0;
    if constexpr (VEC) {
        *(float4*)r = v;
    } else {
        r[0] = v.x;
        if (x0 + 1 < W) r[1] = v.y;
        if (x0 + 2 < W) r[2] = v.z;
        if (x0 + 3 < W) r[3] = v.w;
    }
}

// logical block of this physical one, and the group loop: f(y, x0) for every group of the block
template <int THREADS, typename F>
__device__ __forceinline__ void plane_walk(int H, int G, F&& f) {
    const long long total = (long long)H * G, stride = (long long)gridDim.x * THREADS;
    const unsigned lb = xcd_remap(blockIdx.x, gridDim.x);
    for (long long q = (long long)lb * THREADS + threadIdx.x; q < total; q += stride) {
        const int y = (int)(q / G);
        f(y, ((int)(q - (long long)y * G)) << 2);
    }
}

// block_rows(s0, s1, ...): the running sums of a 256-thread block become the block totals, in place, on thread 0 ALONE; true
// there, and the caller writes its row (at xcd_remap(blockIdx) after plane_walk).  wave_sum, the wave totals staged in LDS behind
// ONE barrier, block_sum4.  (The sums are separate arguments and the steps fold expressions, not loops over an array: straight-line
// code, as each site had.  The sites where thread k stores column k - k_exposure_pass, k_mcmc_reg_pass - keep their own tails: on
// a shared staging routine they compiled to other code.)
template <class... T>
__device__ __forceinline__ bool block_rows(T&... s) {
    __shared__ float red[sizeof...(T)][kPassThreads / 64];
    ((s = wave_sum(s)), ...);
    if ((threadIdx.x & 63) == 0) {
        int k = 0;
        ((red[k++][threadIdx.x >> 6] = s), ...);
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    int k = 0;
    ((s = block_sum4(red[k++])), ...);
    return true;
}

// combine_rows(rows, nrows, t0, t1, ...): column k of the block rows added in fp64 into tk, in the same order by every caller, the
// result on EVERY thread: thread t takes rows t, t + 256, t + 512, t + 768 in that order (four unconditional loads; a row past the
// end reads the last one and counts as zero), then the wave tree and the four waves in the fixed order.  Two barriers: the LDS
// staging may be reused right after it returns.  (C...: the column numbers 0 .. N - 1 as constants, so that the body is the
// straight-line code of one sum written N times.)
__device__ __forceinline__ float row_get(const float4& v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)); }
template <int... C, class... T>
__device__ __forceinline__ void combine_rows(const float4* rows, int nrows, std::integer_sequence<int, C...>, T&... t) {
    static_assert(kPassMaxBlocks == 4 * kPassThreads, "combine_rows: four rows per thread");
    static_assert(sizeof...(T) >= 1 && sizeof...(T) <= 4, "combine_rows: the columns of a float4");
    __shared__ double red[sizeof...(T)][kPassThreads / 64];
    float4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = (int)threadIdx.x + k * kPassThreads;
        v[k] = rows[r < nrows ? r : nrows - 1];
    }
    double a[sizeof...(T)] = {};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool ok = (int)threadIdx.x + k * kPassThreads < nrows;
        ((a[C] += ok ? (double)row_get(v[k], C) : 0.0), ...);
    }
    ((a[C] = wave_sum_d(a[C])), ...);
    if ((threadIdx.x & 63) == 0) ((red[C][threadIdx.x >> 6] = a[C]), ...);
    __syncthreads();
    ((t = block_sum4(red[C])), ...);
    __syncthreads();
}
template <class... T>
__device__ __forceinline__ void combine_rows(const float4* rows, int nrows, T&... t) {
    combine_rows(rows, nrows, std::make_integer_sequence<int, (int)sizeof...(T)>{}, t...);
}

// ------------------------------------------------------------------------------------------------------------------------ host
inline int groups_per_row(int W) { return (W + 3) >> 2; }

// GRID RULE: one group (or item) per thread and trip, between 1 and max_blocks blocks
inline int pass_blocks(long long groups, int threads, int max_blocks) {
    long long b = (groups + threads - 1) / threads;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (int)b;
}

// every pointer 16-byte aligned (a null pointer counts as aligned)
template <class... P>
inline bool aligned16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }

// what every entry asks of a gradient it writes or adds to; the alias checks differ from entry to entry and stay with them
inline int check_grad_target(const char* who, const void* grad, int accumulate, const char* name) {
    SYN3R_REQUIRE(grad, "%s: null pointer", who);
    SYN3R_REQUIRE(accumulate == 0 || accumulate == 1, "%s: %s=%d must be 0 or 1", who, name, accumulate);
    return SYN3R_OK;
}

}  // namespace syn3r
