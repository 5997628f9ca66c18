// Per-camera affine exposure compensation (EXTENSION, include/syn3r_hip.h): the colour transform between a render and the loss,
//   E_c(p) = A[c][0] I_0(p) + A[c][1] I_1(p) + A[c][2] I_2(p) + A[c][3]        A: 3 x 4 fp32, row-major, DEVICE memory
// and its backward
//   grad_image_k(p) = sum_c A[c][k] grad_out_c(p);   grad_A[c][k] = sum_p grad_out_c(p) I_k(p);   grad_A[c][3] = sum_p grad_out_c(p)
// HBM-bound: apply reads three planes and writes three (24 B / pixel), the backward reads six and writes three (36 B / pixel).
//
// The backward is two launches without atomics.  The pass kernel reads the six planes once, writes grad_image and keeps the twelve
// sums of grad_A as fp32 running sums in registers; they are added over the wave (wave_sum), over the block's four waves through
// LDS in a fixed order, and leave as ONE row of twelve partials per block.  The one-block finish kernel adds the rows in a fixed
// order in fp64.  The grid is a function of H * W alone, so the result is the same bits from call to call for a given shape.
//
// The planes are walked flat (n = H * W pixels as one row) in groups of four, at most kExpMaxBlocks blocks; groups, the grid rule,
// VEC (here: n % 4 == 0) and the unconditional loads: plane_pass.h.  The device code keeps its own group load / store and row tail:
// on plane_pass.h's load4 / store4 / block_rows_column both kernels compile to other code (k_exposure_pass<false> to two VGPRs more).
// Built without fma contraction (build.py STRICT_FP): the sums are evaluated left to right as written above.
#include "plane_pass.h"

using namespace syn3r;

namespace {

constexpr int kExpThreads = 256;
constexpr int kExpMaxBlocks = 2048;       // the cap of train.hip's grids (kMaxBlocks)
constexpr int kExpRow = 12;               // floats of A, of grad_A and of a block's row of partials
constexpr int kFinishThreads = 1024, kFinishCols = 16, kFinishGroups = kFinishThreads / kFinishCols;

struct ExpA { float a[kExpRow]; };

__device__ __forceinline__ ExpA exp_load_A(const float* __restrict__ A) {
    ExpA r;
#pragma unroll
    for (int k = 0; k < kExpRow; ++k) r.a[k] = A[k];
    return r;
}

// the four values of plane `p` (n pixels) that group `g` covers; `valid` of them lie inside the plane (4 except in the last group of
// the scalar path).  Scalar path: unconditional loads, indices past the end read the last pixel
template <bool VEC>
__device__ __forceinline__ float4 exp_load4(const float* __restrict__ p, long long g, long long n) {
    if constexpr (VEC) {
        return *(const float4*)(p + g * 4);
    } else {
        const long long e = g * 4, last = n - 1;
        return make_float4(p[e], p[e + 1 < last ? e + 1 : last], p[e + 2 < last ? e + 2 : last], p[e + 3 < last ? e + 3 : last]);
    }
}
template <bool VEC>
__device__ __forceinline__ void exp_store4(float* __restrict__ p, long long g, int valid, float4 v) {
    if constexpr (VEC) {
        *(float4*)(p + g * 4) = v;
    } else {
        const long long e = g * 4;
        p[e] = v.x;
        if (valid > 1) p[e + 1] = v.y;
        if (valid > 2) p[e + 2] = v.z;
        if (valid > 3) p[e + 3] = v.w;
    }
}

__device__ __forceinline__ float exp_apply1(const float* a /*one row of A*/, float i0, float i1, float i2) {
    return a[0] * i0 + a[1] * i1 + a[2] * i2 + a[3];
}

template <bool VEC>
__global__ void __launch_bounds__(kExpThreads) k_exposure_apply(const float* __restrict__ image, const float* __restrict__ A,
                                                               long long n, float* __restrict__ out) {
    const ExpA m = exp_load_A(A);
    const long long groups = (n + 3) >> 2;
    for (long long g = (long long)blockIdx.x * kExpThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kExpThreads) {
        const float4 i0 = exp_load4<VEC>(image, g, n), i1 = exp_load4<VEC>(image + n, g, n), i2 = exp_load4<VEC>(image + 2 * n, g, n);
        const long long left = n - g * 4;
        const int valid = left < 4 ? (int)left : 4;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* a = m.a + 4 * c;
            exp_store4<VEC>(out + c * n, g, valid, make_float4(exp_apply1(a, i0.x, i1.x, i2.x), exp_apply1(a, i0.y, i1.y, i2.y),
                                                               exp_apply1(a, i0.z, i1.z, i2.z), exp_apply1(a, i0.w, i1.w, i2.w)));
        }
    }
}

// one pixel of the backward: its three grad_image values, and its terms added to the twelve running sums
__device__ __forceinline__ void exp_bwd1(const ExpA& m, float (&s)[kExpRow], float i0, float i1, float i2, float g0, float g1, float g2,
                                         float& d0, float& d1, float& d2) {
    d0 = m.a[0] * g0 + m.a[4] * g1 + m.a[8] * g2;
    d1 = m.a[1] * g0 + m.a[5] * g1 + m.a[9] * g2;
    d2 = m.a[2] * g0 + m.a[6] * g1 + m.a[10] * g2;
    s[0] += g0 * i0; s[1] += g0 * i1; s[2] += g0 * i2; s[3] += g0;
    s[4] += g1 * i0; s[5] += g1 * i1; s[6] += g1 * i2; s[7] += g1;
    s[8] += g2 * i0; s[9] += g2 * i1; s[10] += g2 * i2; s[11] += g2;
}

template <bool VEC>
__global__ void __launch_bounds__(kExpThreads) k_exposure_pass(const float* __restrict__ image, const float* __restrict__ A,
                                                              const float* __restrict__ grad_out, long long n,
                                                              float* __restrict__ grad_image, float* __restrict__ rows) {
    const ExpA m = exp_load_A(A);
    float s[kExpRow];
#pragma unroll
    for (int k = 0; k < kExpRow; ++k) s[k] = 0.0f;
    const long long groups = (n + 3) >> 2;
    for (long long g = (long long)blockIdx.x * kExpThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kExpThreads) {
        float4 i0 = exp_load4<VEC>(image, g, n), i1 = exp_load4<VEC>(image + n, g, n), i2 = exp_load4<VEC>(image + 2 * n, g, n);
        float4 g0 = exp_load4<VEC>(grad_out, g, n), g1 = exp_load4<VEC>(grad_out + n, g, n), g2 = exp_load4<VEC>(grad_out + 2 * n, g, n);
        const long long left = n - g * 4;
        const int valid = left < 4 ? (int)left : 4;
        if constexpr (!VEC) {                // pixels past the end: zero terms (their loads read the last pixel)
            if (valid < 2) { i0.y = i1.y = i2.y = g0.y = g1.y = g2.y = 0.0f; }
            if (valid < 3) { i0.z = i1.z = i2.z = g0.z = g1.z = g2.z = 0.0f; }
            if (valid < 4) { i0.w = i1.w = i2.w = g0.w = g1.w = g2.w = 0.0f; }
        }
        float4 d0, d1, d2;
        exp_bwd1(m, s, i0.x, i1.x, i2.x, g0.x, g1.x, g2.x, d0.x, d1.x, d2.x);
        exp_bwd1(m, s, i0.y, i1.y, i2.y, g0.y, g1.y, g2.y, d0.y, d1.y, d2.y);
        exp_bwd1(m, s, i0.z, i1.z, i2.z, g0.z, g1.z, g2.z, d0.z, d1.z, d2.z);
        exp_bwd1(m, s, i0.w, i1.w, i2.w, g0.w, g1.w, g2.w, d0.w, d1.w, d2.w);
        exp_store4<VEC>(grad_image, g, valid, d0);
        exp_store4<VEC>(grad_image + n, g, valid, d1);
        exp_store4<VEC>(grad_image + 2 * n, g, valid, d2);
    }
    __shared__ float part[kExpThreads / 64][kExpRow];
#pragma unroll
    for (int k = 0; k < kExpRow; ++k) {
        const float w = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < kExpRow) {
        const int k = threadIdx.x;
        rows[(size_t)blockIdx.x * kExpRow + k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
    }
}

// one block: column k of the block rows in a fixed order, in fp64 (thread group q takes rows q, q + kFinishGroups, ...; the groups
// are then added in ascending order).  Eight rows per trip, their loads unconditional (a row past the end reads the last row and
// counts as zero) so that they issue together: one dependent load per trip made this kernel 31 us at 1080p, twice the pass kernel
__global__ void __launch_bounds__(kFinishThreads) k_exposure_finish(int nrows, const float* __restrict__ rows, float* __restrict__ grad_A,
                                                                   int accumulate) {
    __shared__ double part[kFinishGroups][kFinishCols];
    const int col = threadIdx.x % kFinishCols, grp = threadIdx.x / kFinishCols;
    double acc = 0.0;
    if (col < kExpRow)
        for (int r = grp; r < nrows; r += 8 * kFinishGroups) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int rr = r + k * kFinishGroups;
                v[k] = rows[(size_t)(rr < nrows ? rr : nrows - 1) * kExpRow + col];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) acc += r + k * kFinishGroups < nrows ? (double)v[k] : 0.0;
        }
    part[grp][col] = acc;
    __syncthreads();
    if (threadIdx.x >= kExpRow) return;
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < kFinishGroups; ++q) t += part[q][threadIdx.x];
    grad_A[threadIdx.x] = accumulate ? grad_A[threadIdx.x] + (float)t : (float)t;
}

// blocks of both grids: a function of the pixel count alone
int exp_blocks(long long n) { return pass_blocks((n + 3) / 4, kExpThreads, kExpMaxBlocks); }

}  // namespace

extern "C" int syn3r_exposure_apply(const float* image, const float* A, int H, int W, float* out, void* stream_) {
    SYN3R_REQUIRE(SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W), "exposure_apply: H=%d, W=%d must be in [1, 2^15]", H, W);
    SYN3R_REQUIRE(image && A && out, "exposure_apply: null pointer");
    SYN3R_REQUIRE((((uintptr_t)image | (uintptr_t)A | (uintptr_t)out) & 3) == 0, "exposure_apply: pointers must be 4-byte aligned");
    const long long n = (long long)H * W;
    const size_t bytes = (size_t)n * 3 * sizeof(float), a_bytes = kExpRow * sizeof(float);
    SYN3R_REQUIRE(!ranges_overlap(out, bytes, image, bytes) && !ranges_overlap(out, bytes, A, a_bytes), "exposure_apply: out aliases an input");
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)exp_blocks(n));
    with_bools([&](auto vec) {
        SYN3R_LAUNCH_NAMED("k_exposure_apply", k_exposure_apply<decltype(vec)::value>, grid, dim3(kExpThreads), 0, stream, image, A, n, out);
    }, n % 4 == 0 && aligned16(image, out));
    SYN3R_LAUNCH_CHECK("exposure_apply launch");
    return SYN3R_OK;
}

extern "C" size_t syn3r_exposure_backward_workspace_bytes(int H, int W) {
    if (!SYN3R_SIDE_OK(H) || !SYN3R_SIDE_OK(W)) return 0;
    return (((size_t)exp_blocks((long long)H * W) * kExpRow * sizeof(float) + 255) / 256) * 256;
}

extern "C" int syn3r_exposure_backward(const float* image, const float* A, const float* grad_out, int H, int W, float* grad_image,
                                       float* grad_A, int accumulate, void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W), "exposure_backward: H=%d, W=%d must be in [1, 2^15]", H, W);
    SYN3R_REQUIRE(image && A && grad_out && grad_image && grad_A && ws, "exposure_backward: null pointer");
    SYN3R_REQUIRE((((uintptr_t)image | (uintptr_t)A | (uintptr_t)grad_out | (uintptr_t)grad_image | (uintptr_t)grad_A) & 3) == 0,
                  "exposure_backward: pointers must be 4-byte aligned");
    if (const int rc = check_workspace("exposure_backward", ws, ws_bytes, syn3r_exposure_backward_workspace_bytes(H, W),
                                       "syn3r_exposure_backward_workspace_bytes")) return rc;
    const long long n = (long long)H * W;
    const size_t bytes = (size_t)n * 3 * sizeof(float), a_bytes = kExpRow * sizeof(float);
    SYN3R_REQUIRE(!ranges_overlap(grad_image, bytes, image, bytes) && !ranges_overlap(grad_image, bytes, grad_out, bytes) &&
                  !ranges_overlap(grad_image, bytes, A, a_bytes), "exposure_backward: grad_image aliases an input");
    hipStream_t stream = (hipStream_t)stream_;
    const int nb = exp_blocks(n);
    float* rows = (float*)ws;
    with_bools([&](auto vec) {
        SYN3R_LAUNCH_NAMED("k_exposure_pass", k_exposure_pass<decltype(vec)::value>, dim3((unsigned)nb), dim3(kExpThreads), 0, stream, image, A,
                           grad_out, n, grad_image, rows);
    }, n % 4 == 0 && aligned16(image, grad_out, grad_image));
    SYN3R_LAUNCH(k_exposure_finish, dim3(1), dim3(kFinishThreads), 0, stream, nb, (const float*)rows, grad_A, accumulate);
    SYN3R_LAUNCH_CHECK("exposure_backward launch");
    return SYN3R_OK;
}
