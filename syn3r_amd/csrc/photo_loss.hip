// The fused L1 + SSIM photometric loss of the trainer (syn3r_photo_loss*, with and without a per-pixel weight map): the tile
// kernels k_photo_fwd / k_photo_bwd, the fixed-order final sum, and one host path per kind (forward, backward, step) behind
// the six entries.  Compiled without fma contraction (build.py STRICT_FP): tests/test_photo_elementwise_*.py count its roundings.
#include "common.h"

using namespace syn3r;

namespace {

// Photometric loss of the published 3DGS trainer, fused:  L = w * [(1 - lambda) * mean|I - G| + lambda * (1 - SSIM(I, G))]
// with SSIM as published (11x11 Gaussian window, sigma 1.5, zero padding 5, C1 = 0.01^2, C2 = 0.03^2, mean over
// all channels and pixels).  Forward: one pass over 32x32 tiles, separable window (horizontal then vertical) on the five
// moments; it also stores the three per-pixel derivative maps (d ssim / d mu1 [total], / d sigma1^2, / d sigma12) the
// backward needs.  Backward: the same separable window on those three maps, combined with the L1 sign term, one write of
// the image gradient.
// Round 5 form (the 16x16-tile, one-output-per-thread kernels ran 96 + 67 us at 1080p, half of it vector issue): a thread
// owns FOUR adjacent outputs in each pass - a row run in the horizontal pass, whose 14 inputs come straight from global
// memory as aligned 16-byte loads (no staging tile, one barrier less), a column run in the vertical pass - so the inputs'
// squares and products are formed once per input instead of once per tap, and the moments travel in pairs on packed fp32
// FMAs: (mu1, mu2) and (E[p^2], E[q^2]) are one v_pk_fma_f32 per tap each, E[pq] a v_fma_f32 (3 instructions per tap and
// output where the unpacked, uncontracted form issued 10).  The taps of an output are accumulated in ascending order.
constexpr int kWin = 11, kHalo = 5, kTile = 32, kReg = kTile + 2 * kHalo;   // 42
constexpr int kRun = 4, kSpan = kRun + kWin - 1;   // 4 outputs per thread and pass, 14 inputs
constexpr int kLead = 8 - kHalo;                   // a row run is loaded from 8 columns left of its first output: 16-byte aligned
constexpr int kPhotoItems = kReg * (kTile / kRun);   // 336 horizontal items per tile
constexpr int kPhotoThreads = 256;                 // the vertical pass' 32 columns x 8 row runs (384 threads = one round of horizontal items: +17 % forward)
struct SsimWindow { float g[kWin]; };
// Tile of block b (xcd_remap): XCD x takes the x-th contiguous eighth of the row-major tile list - neighbouring tiles (which share
// 10 of 42 halo rows and 16 of 48 loaded columns) meet in one L2 instead of being fetched by two.
struct PhotoTile { int c, x0, y0; unsigned id; };
__device__ __forceinline__ PhotoTile photo_tile(int gx, int gy) {
    const unsigned t = xcd_remap(blockIdx.x, gridDim.x);
    PhotoTile o;
    o.id = t;
    o.c = (int)(t / (unsigned)(gx * gy));
    const unsigned rem = t - (unsigned)o.c * (unsigned)(gx * gy);
    o.y0 = (int)(rem / (unsigned)gx) * kTile;
    o.x0 = (int)(rem % (unsigned)gx) * kTile;
    return o;
}
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

__device__ __forceinline__ float block_sum_photo(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float t = block_sum4(red);
    __syncthreads();
    return t;
}

// 20 consecutive values of image row y from column x (x % 4 == 0; zero outside the image).  VEC: W % 4 == 0 and the plane is
// 16-byte aligned, so a group of four is inside the image or outside it as a whole.  Every load is UNCONDITIONAL from an address
// clamped into the plane and the zero is a select afterwards: a load behind its own `inside ? load : 0` branch waits for the one
// before it (hipcc does not move loads across the exec-mask branches: the ten loads of a row run were a chain of ten latencies).
template <bool VEC>
__device__ __forceinline__ void photo_load20(float (&v)[20], const float* __restrict__ plane, int y, int x, int H, int W) {
    const bool row = y >= 0 && y < H;
    const float* src = plane + (size_t)min(max(y, 0), H - 1) * W;
    if constexpr (VEC) {
        float4 t[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) t[q] = *(const float4*)(src + min(max(x + 4 * q, 0), W - 4));
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const bool in = row && x + 4 * q >= 0 && x + 4 * q < W;
            v[4 * q] = in ? t[q].x : 0.0f; v[4 * q + 1] = in ? t[q].y : 0.0f; v[4 * q + 2] = in ? t[q].z : 0.0f; v[4 * q + 3] = in ? t[q].w : 0.0f;
        }
    } else {
        float t[20];
#pragma unroll
        for (int e = 0; e < 20; ++e) t[e] = src[min(max(x + e, 0), W - 1)];
#pragma unroll
        for (int e = 0; e < 20; ++e) v[e] = (row && x + e >= 0 && x + e < W) ? t[e] : 0.0f;
    }
}

// The weights of an item's own four pixels (row y, columns x .. x + 3; x % 4 == 0): photo_load20's rule - an unconditional load
// from a clamped address, zero outside the image by a select afterwards.
template <bool VEC>
__device__ __forceinline__ void photo_load4(float (&v)[kRun], const float* __restrict__ plane, int y, int x, int H, int W) {
    const bool row = y >= 0 && y < H;
    const float* src = plane + (size_t)min(max(y, 0), H - 1) * W;
    if constexpr (VEC) {
        const float4 t = *(const float4*)(src + min(x, W - 4));
        const bool in = row && x < W;
        v[0] = in ? t.x : 0.0f; v[1] = in ? t.y : 0.0f; v[2] = in ? t.z : 0.0f; v[3] = in ? t.w : 0.0f;
    } else {
        float t[kRun];
#pragma unroll
        for (int e = 0; e < kRun; ++e) t[e] = src[min(x + e, W - 1)];
#pragma unroll
        for (int e = 0; e < kRun; ++e) v[e] = (row && x + e < W) ? t[e] : 0.0f;
    }
}

// MAP: the per-pixel weight map `wmap` [H,W] of syn3r_photo_loss_map (one map for all channels) multiplies the L1 term and the SSIM
// map VALUE at the output pixel - so the three stored derivative maps carry it and the backward's window needs nothing new -; it
// does not enter the window moments.  The tile's sums become (sum m|d|, sum m ssim, sum m): 3 floats per tile instead of 2.
// MAP = false is the kernel without a map: `wmap` is never read, no branch is added.
template <bool VEC, bool MAP>
__global__ void __launch_bounds__(kPhotoThreads) k_photo_fwd(const float* __restrict__ img, const float* __restrict__ gt, int H,
                                                   int W, int C, SsimWindow win, float* __restrict__ maps,
                                                   float* __restrict__ partial, const float* __restrict__ wmap) {
    __shared__ __attribute__((aligned(16))) f2 hA[kReg][kTile], hB[kReg][kTile];   // (mu1, mu2), (E[p^2], E[q^2]) after the horizontal pass
    __shared__ __attribute__((aligned(16))) float hC[kReg][kTile];                 // E[pq]
    __shared__ float red[kPhotoThreads / 64];
    const PhotoTile tl_ = photo_tile((W + kTile - 1) / kTile, (H + kTile - 1) / kTile);
    const int c = tl_.c, x0 = tl_.x0, y0 = tl_.y0;
    const size_t plane = (size_t)H * W;
    const float* a = img + c * plane;
    const float* b = gt + c * plane;
    float l1_sum = 0.f;
    // MAP: the weights of the vertical pass' own pixels (column tx, rows ty .. ty + 3), requested before the horizontal pass
    float mv[kRun];
    if constexpr (MAP) {
#pragma unroll
        for (int j = 0; j < kRun; ++j)
            mv[j] = wmap[(size_t)min(y0 + (int)(threadIdx.x >> 5) * kRun + j, H - 1) * W + min(x0 + (int)(threadIdx.x & (kTile - 1)), W - 1)];     // (clamped: rows / columns past the image are not summed)
    }
    // horizontal pass: item = (halo row, run of 4 columns)
    for (int i = threadIdx.x; i < kPhotoItems; i += kPhotoThreads) {
        const int ry = i / (kTile / kRun), tx = (i - ry * (kTile / kRun)) * kRun;
        const int y = y0 + ry - kHalo;
        float p[20], q[20];
        photo_load20<VEC>(p, a, y, x0 + tx - 8, H, W);
        photo_load20<VEC>(q, b, y, x0 + tx - 8, H, W);
        float mh[kRun];
        if constexpr (MAP) photo_load4<VEC>(mh, wmap, y, x0 + tx, H, W);
        f2 pq[kSpan], sq[kSpan];
        float pr[kSpan];
#pragma unroll
        for (int t = 0; t < kSpan; ++t) {
            pq[t] = (f2){p[kLead + t], q[kLead + t]};
            sq[t] = pq[t] * pq[t];
            pr[t] = pq[t].x * pq[t].y;
        }
        f2 mA[kRun], mB[kRun];
        float mC[kRun];
#pragma unroll
        for (int j = 0; j < kRun; ++j) { mA[j] = (f2){0.f, 0.f}; mB[j] = (f2){0.f, 0.f}; mC[j] = 0.f; }
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const f2 w2 = (f2){win.g[k], win.g[k]};
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                mA[j] = fma2(w2, pq[j + k], mA[j]);
                mB[j] = fma2(w2, sq[j + k], mB[j]);
                mC[j] = __builtin_fmaf(win.g[k], pr[j + k], mC[j]);
            }
        }
        *(float4*)&hA[ry][tx] = make_float4(mA[0].x, mA[0].y, mA[1].x, mA[1].y);
        *(float4*)&hA[ry][tx + 2] = make_float4(mA[2].x, mA[2].y, mA[3].x, mA[3].y);
        *(float4*)&hB[ry][tx] = make_float4(mB[0].x, mB[0].y, mB[1].x, mB[1].y);
        *(float4*)&hB[ry][tx + 2] = make_float4(mB[2].x, mB[2].y, mB[3].x, mB[3].y);
        *(float4*)&hC[ry][tx] = make_float4(mC[0], mC[1], mC[2], mC[3]);
        if (ry >= kHalo && ry < kHalo + kTile && y < H) {      // an output row: its L1 terms (the run's own pixels are inputs kHalo .. kHalo + 3)
#pragma unroll
            for (int j = 0; j < kRun; ++j)
                if (x0 + tx + j < W) {
                    if constexpr (MAP) l1_sum += mh[j] * fabsf(pq[kHalo + j].x - pq[kHalo + j].y);
                    else l1_sum += fabsf(pq[kHalo + j].x - pq[kHalo + j].y);
                }
        }
    }
    __syncthreads();
    // vertical pass: thread = (column, run of 4 rows)
    const int tx = threadIdx.x & (kTile - 1), ty = (threadIdx.x >> 5) * kRun;
    const int x = x0 + tx;
    f2 mA[kRun], mB[kRun];
    float mC[kRun];
    {
        f2 vA[kSpan], vB[kSpan];
        float vC[kSpan];
#pragma unroll
        for (int t = 0; t < kSpan; ++t) { vA[t] = hA[ty + t][tx]; vB[t] = hB[ty + t][tx]; vC[t] = hC[ty + t][tx]; }
#pragma unroll
        for (int j = 0; j < kRun; ++j) { mA[j] = (f2){0.f, 0.f}; mB[j] = (f2){0.f, 0.f}; mC[j] = 0.f; }
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const f2 w2 = (f2){win.g[k], win.g[k]};
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                mA[j] = fma2(w2, vA[j + k], mA[j]);
                mB[j] = fma2(w2, vB[j + k], mB[j]);
                mC[j] = __builtin_fmaf(win.g[k], vC[j + k], mC[j]);
            }
        }
    }
    float ssim_sum = 0.f, m_sum = 0.f;
    const size_t n = (size_t)C * plane;
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
        const int y = y0 + ty + j;
        if (x < W && y < H) {
            const float mu1 = mA[j].x, mu2 = mA[j].y, e11 = mB[j].x, e22 = mB[j].y, e12 = mC[j];
            const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
            const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
            const float sg1 = e11 - mu1s, sg2 = e22 - mu2s, sg12 = e12 - mu12;
            const float A = 2.f * mu12 + C1, B = 2.f * sg12 + C2, Cc = mu1s + mu2s + C1, D = sg1 + sg2 + C2;
            // Cc >= C1, D >= C2 - rounding: both positive and far from the denormals; v_rcp_f32 is a 1-ulp reciprocal
            // (an IEEE division is ~10 instructions, three of them were a third of this pass)
            const float invC = __builtin_amdgcn_rcpf(Cc), invD = __builtin_amdgcn_rcpf(D);
            const float inv = invC * invD;
            const float ssim = A * B * inv;
            // partial derivatives of the map value (gt is constant)
            const float d_sg1 = -ssim * invD;              // d/d sigma1^2
            const float d_sg12 = 2.f * A * inv;            // d/d sigma12
            const float d_mu1 = (2.f * mu2 * B * Cc - 2.f * mu1 * A * B) * inv * invC    // explicit
                                - 2.f * mu1 * d_sg1 - mu2 * d_sg12;                      // through sigma1^2, sigma12
            const size_t o = (size_t)c * plane + (size_t)y * W + x;
            if constexpr (MAP) {
                const float m = mv[j];
                maps[o] = m * d_mu1; maps[n + o] = m * d_sg1; maps[2 * n + o] = m * d_sg12;
                ssim_sum += m * ssim;
                m_sum += m;
            } else {
                maps[o] = d_mu1; maps[n + o] = d_sg1; maps[2 * n + o] = d_sg12;
                ssim_sum += ssim;
            }
        }
    }
    const float ts = block_sum_photo(ssim_sum, red);
    const float tl = block_sum_photo(l1_sum, red);
    if constexpr (MAP) {
        const float tm = block_sum_photo(m_sum, red);
        if (threadIdx.x == 0) {
            const size_t bid = tl_.id;
            partial[3 * bid] = tl;
            partial[3 * bid + 1] = ts;
            partial[3 * bid + 2] = tm;
        }
    } else if (threadIdx.x == 0) {
        const size_t bid = tl_.id;
        partial[2 * bid] = tl;
        partial[2 * bid + 1] = ts;
    }
}

// loss[0] = w*((1-lam)*L1 + lam*(1-SSIM)), loss[1] = L1, loss[2] = SSIM  (fixed-order double sums; a block of 256 threads)
// MAP (3 floats per tile, 4 outputs): loss[1] = mean(m|d|), loss[2] = mean(m ssim), loss[3] = mean(m),
// loss[0] = w*((1-lam)*loss[1] + lam*(loss[3] - loss[2])) - all means over the C*H*W elements
struct PhotoFinal { const float* partial; long long nblocks; double inv_n; float lam, weight; float* loss; };
template <bool MAP>
__device__ __forceinline__ void photo_final(const PhotoFinal f) {
    static_assert(kPhotoThreads == 256, "photo_final: one sum per thread of a 256-thread block");
    constexpr int kPer = MAP ? 3 : 2;
    double sl = 0.0, ss = 0.0, sm = 0.0;
    for (long long i = threadIdx.x; i < f.nblocks; i += 256) {
        sl += (double)f.partial[kPer * i]; ss += (double)f.partial[kPer * i + 1];
        if constexpr (MAP) sm += (double)f.partial[kPer * i + 2];
    }
    sl = wave_sum_d(sl); ss = wave_sum_d(ss);
    if constexpr (MAP) sm = wave_sum_d(sm);
    __shared__ double w1[4], w2[4];
    double* w3 = nullptr;
    if constexpr (MAP) { __shared__ double w3s[4]; w3 = w3s; }
    if ((threadIdx.x & 63) == 0) {
        w1[threadIdx.x >> 6] = sl; w2[threadIdx.x >> 6] = ss;
        if constexpr (MAP) w3[threadIdx.x >> 6] = sm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double l1 = block_sum4(w1) * f.inv_n, ssim = block_sum4(w2) * f.inv_n;
        if constexpr (MAP) {
            const double mm = block_sum4(w3) * f.inv_n;
            f.loss[0] = (float)((double)f.weight * ((1.0 - (double)f.lam) * l1 + (double)f.lam * (mm - ssim)));
            f.loss[3] = (float)mm;
        } else {
            f.loss[0] = (float)((double)f.weight * ((1.0 - (double)f.lam) * l1 + (double)f.lam * (1.0 - ssim)));
        }
        f.loss[1] = (float)l1;
        f.loss[2] = (float)ssim;
    }
}
__global__ void __launch_bounds__(256) k_photo_final(PhotoFinal f) { photo_final<false>(f); }
__global__ void __launch_bounds__(256) k_photo_final_map(PhotoFinal f) { photo_final<true>(f); }

// MAP: the L1 sign term takes the weight m(q) of its own pixel; the windowed part reads derivative maps that already carry it
template <bool VEC, bool MAP>
__global__ void __launch_bounds__(kPhotoThreads) k_photo_bwd(const float* __restrict__ img, const float* __restrict__ gt, int H,
                                                   int W, int C, SsimWindow win, const float* __restrict__ maps, float c_l1,
                                                   float c_ssim, const float* __restrict__ go,
                                                   float* __restrict__ grad, PhotoFinal fin, const float* __restrict__ wmap) {
    __shared__ __attribute__((aligned(16))) f2 hA[kReg][kTile];      // windowed (d_mu1, d_sigma1^2) after the horizontal pass
    // syn3r_photo_loss_step: the forward's per-tile sums become loss3 HERE (k_photo_final's fixed-order double sums, by the block
    // that is dispatched first) instead of in a single-block launch between the two passes: the gradient does not read the loss
    if (fin.partial && blockIdx.x == 0) photo_final<MAP>(fin);
    __shared__ __attribute__((aligned(16))) float hC[kReg][kTile];   // windowed d_sigma12
    const PhotoTile tl_ = photo_tile((W + kTile - 1) / kTile, (H + kTile - 1) / kTile);
    const int c = tl_.c, x0 = tl_.x0, y0 = tl_.y0;
    const size_t plane = (size_t)H * W, n = (size_t)C * plane;
    const float* m0 = maps + c * plane;
    // the vertical pass' own pixels (column tx, rows ty .. ty + 3), requested before the horizontal pass
    const int vtx = threadIdx.x & (kTile - 1), vty = (threadIdx.x >> 5) * kRun;
    float pv[kRun], qv[kRun], mv[kRun];
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
        const size_t o = (size_t)c * plane + (size_t)min(y0 + vty + j, H - 1) * W + min(x0 + vtx, W - 1);     // (clamped: rows / columns past the image are not written)
        pv[j] = img[o];
        qv[j] = gt[o];
        if constexpr (MAP) mv[j] = wmap[o - (size_t)c * plane];
    }
    for (int i = threadIdx.x; i < kPhotoItems; i += kPhotoThreads) {
        const int ry = i / (kTile / kRun), tx = (i - ry * (kTile / kRun)) * kRun;
        const int y = y0 + ry - kHalo;
        float u0[20], u1[20], u2[20];
        photo_load20<VEC>(u0, m0, y, x0 + tx - 8, H, W);
        photo_load20<VEC>(u1, m0 + n, y, x0 + tx - 8, H, W);
        photo_load20<VEC>(u2, m0 + 2 * n, y, x0 + tx - 8, H, W);
        f2 mA[kRun];
        float mC[kRun];
#pragma unroll
        for (int j = 0; j < kRun; ++j) { mA[j] = (f2){0.f, 0.f}; mC[j] = 0.f; }
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const f2 w2 = (f2){win.g[k], win.g[k]};
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                mA[j] = fma2(w2, (f2){u0[kLead + j + k], u1[kLead + j + k]}, mA[j]);
                mC[j] = __builtin_fmaf(win.g[k], u2[kLead + j + k], mC[j]);
            }
        }
        *(float4*)&hA[ry][tx] = make_float4(mA[0].x, mA[0].y, mA[1].x, mA[1].y);
        *(float4*)&hA[ry][tx + 2] = make_float4(mA[2].x, mA[2].y, mA[3].x, mA[3].y);
        *(float4*)&hC[ry][tx] = make_float4(mC[0], mC[1], mC[2], mC[3]);
    }
    __syncthreads();
    const int tx = vtx, ty = vty;
    const int x = x0 + tx;
    f2 gA[kRun];
    float gC[kRun];
    {
        f2 vA[kSpan];
        float vC[kSpan];
#pragma unroll
        for (int t = 0; t < kSpan; ++t) { vA[t] = hA[ty + t][tx]; vC[t] = hC[ty + t][tx]; }
#pragma unroll
        for (int j = 0; j < kRun; ++j) { gA[j] = (f2){0.f, 0.f}; gC[j] = 0.f; }
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const f2 w2 = (f2){win.g[k], win.g[k]};
#pragma unroll
            for (int j = 0; j < kRun; ++j) {
                gA[j] = fma2(w2, vA[j + k], gA[j]);
                gC[j] = __builtin_fmaf(win.g[k], vC[j + k], gC[j]);
            }
        }
    }
    const float up = go ? *go : 1.0f;
#pragma unroll
    for (int j = 0; j < kRun; ++j) {
        const int y = y0 + ty + j;
        if (x >= W || y >= H) continue;
        const size_t o = (size_t)c * plane + (size_t)y * W + x;
        const float p = pv[j], q = qv[j], d = p - q;
        const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
        if constexpr (MAP) grad[o] = up * (c_l1 * (mv[j] * sgn) - c_ssim * (gA[j].x + 2.0f * p * gA[j].y + q * gC[j]));
        else grad[o] = up * (c_l1 * sgn - c_ssim * (gA[j].x + 2.0f * p * gA[j].y + q * gC[j]));
    }
}

}  // namespace

static SsimWindow make_window() {
    SsimWindow w;
    double g[kWin], sum = 0.0;
    for (int i = 0; i < kWin; ++i) { g[i] = exp(-(double)((i - kWin / 2) * (i - kWin / 2)) / (2.0 * 1.5 * 1.5)); sum += g[i]; }
    for (int i = 0; i < kWin; ++i) w.g[i] = (float)(g[i] / sum);
    return w;
}

// Blocks of k_photo_fwd / k_photo_bwd, one per 32x32 tile and channel; 0: a size is out of range
static long long photo_tiles(int C, int H, int W) {
    if (C <= 0 || C > 65535 || !SYN3R_SIDE_OK(H) || !SYN3R_SIDE_OK(W)) return 0;
    return (long long)((W + kTile - 1) / kTile) * ((H + kTile - 1) / kTile) * C;
}

// the three derivative maps, then `per_tile` floats of sums per tile
static size_t photo_workspace_bytes(int C, int H, int W, size_t per_tile) {
    const size_t blocks = (size_t)photo_tiles(C, H, W);
    if (!blocks) return 0;
    const size_t n = (size_t)C * H * W;
    return 3 * n * sizeof(float) + ((per_tile * blocks * sizeof(float) + 255) / 256) * 256;
}
extern "C" size_t syn3r_photo_loss_workspace_bytes(int C, int H, int W) { return photo_workspace_bytes(C, H, W, 2); }
extern "C" size_t syn3r_photo_loss_map_workspace_bytes(int C, int H, int W) { return photo_workspace_bytes(C, H, W, 3); }

// what kernel_trace calls the tile kernels: [backward][MAP][VEC]
static const char* const kPhotoNames[2][2][2] = {{{"k_photo_fwd<false>", "k_photo_fwd<true>"}, {"k_photo_fwd_map<false>", "k_photo_fwd_map<true>"}},
                                                 {{"k_photo_bwd<false>", "k_photo_bwd<true>"}, {"k_photo_bwd_map<false>", "k_photo_bwd_map<true>"}}};

// Forward pass (k_photo_fwd) behind the loss and the step entries.  `map` (the syn3r_photo_loss_map entries; null: none): 3 sums per
// tile and 4 floats in loss3.  `fin` null: loss3 by k_photo_final here; else the final sum is handed back for the backward's launch.
static int photo_forward(const char* who, const float* image, const float* target, const float* map, int C, int H, int W, float lambda_dssim,
                         float weight, float* loss3, void* ws, size_t ws_bytes, hipStream_t stream, PhotoFinal* fin) {
    const long long tiles = photo_tiles(C, H, W);
    SYN3R_REQUIRE(tiles > 0, "%s: bad sizes C=%d H=%d W=%d", who, C, H, W);
    SYN3R_REQUIRE(image && target && loss3 && ws, "%s: null pointer", who);
    SYN3R_REQUIRE(lambda_dssim >= 0.0f && lambda_dssim <= 1.0f, "%s: lambda_dssim must be in [0, 1]", who);
    SYN3R_REQUIRE(ws_bytes >= photo_workspace_bytes(C, H, W, map ? 3 : 2), "%s: workspace too small", who);
    SYN3R_REQUIRE(tiles < (1ll << 31), "%s: %lld tiles exceed the grid limit", who, tiles);
    const size_t n = (size_t)C * H * W;
    float* maps = (float*)ws;
    float* partial = maps + 3 * n;
    const bool vec = W % 4 == 0 && (((uintptr_t)image | (uintptr_t)target | (uintptr_t)map) & 15) == 0;      // aligned 16-byte row runs
    with_bools([&](auto V, auto M) {
        constexpr bool VEC = decltype(V)::value, MAP = decltype(M)::value;
        SYN3R_LAUNCH_NAMED(kPhotoNames[0][MAP][VEC], (k_photo_fwd<VEC, MAP>), dim3((unsigned)tiles), dim3(kPhotoThreads), 0, stream, image, target,
                           H, W, C, make_window(), maps, partial, map);
    }, vec, map != nullptr);
    const PhotoFinal f{partial, tiles, 1.0 / (double)n, lambda_dssim, weight, loss3};
    if (fin) *fin = f;
    else if (map) SYN3R_LAUNCH(k_photo_final_map, dim3(1), dim3(256), 0, stream, f);
    else SYN3R_LAUNCH(k_photo_final, dim3(1), dim3(256), 0, stream, f);
    return check_launch(who);
}

// Backward pass (k_photo_bwd) behind the backward and the step entries; `fin` of the step: photo_forward's, else empty
static int photo_backward(const char* who, const float* image, const float* target, const float* map, int C, int H, int W, float lambda_dssim,
                          float weight, const float* grad_loss, const void* ws, float* grad_image, hipStream_t stream, PhotoFinal fin) {
    const long long tiles = photo_tiles(C, H, W);
    SYN3R_REQUIRE(tiles > 0, "%s: bad sizes", who);
    SYN3R_REQUIRE(image && target && ws && grad_image, "%s: null pointer", who);
    SYN3R_REQUIRE(tiles < (1ll << 31), "%s: %lld tiles exceed the grid limit", who, tiles);
    const double n = (double)C * H * W;
    const bool vec = W % 4 == 0 && ((uintptr_t)ws & 15) == 0;
    const float c_l1 = (float)((double)weight * (1.0 - (double)lambda_dssim) / n), c_ssim = (float)((double)weight * (double)lambda_dssim / n);
    with_bools([&](auto V, auto M) {
        constexpr bool VEC = decltype(V)::value, MAP = decltype(M)::value;
        SYN3R_LAUNCH_NAMED(kPhotoNames[1][MAP][VEC], (k_photo_bwd<VEC, MAP>), dim3((unsigned)tiles), dim3(kPhotoThreads), 0, stream, image, target,
                           H, W, C, make_window(), (const float*)ws, c_l1, c_ssim, grad_loss, grad_image, fin, map);
    }, vec, map != nullptr);
    return check_launch(who);
}

static int photo_step(const char* who, const float* image, const float* target, const float* map, int C, int H, int W, float lambda_dssim,
                      float weight, const float* grad_loss, float* loss3, float* grad_image, void* ws, size_t ws_bytes, hipStream_t stream) {
    PhotoFinal fin{};
    const int rc = photo_forward(who, image, target, map, C, H, W, lambda_dssim, weight, loss3, ws, ws_bytes, stream, &fin);
    if (rc) return rc;
    return photo_backward(who, image, target, map, C, H, W, lambda_dssim, weight, grad_loss, ws, grad_image, stream, fin);
}

extern "C" int syn3r_photo_loss(const float* image, const float* target, int C, int H, int W, float lambda_dssim,
                                float weight, float* loss3, void* ws, size_t ws_bytes, void* stream_) {
    return photo_forward("photo_loss", image, target, nullptr, C, H, W, lambda_dssim, weight, loss3, ws, ws_bytes, (hipStream_t)stream_, nullptr);
}

extern "C" int syn3r_photo_loss_backward(const float* image, const float* target, int C, int H, int W,
                                         float lambda_dssim, float weight, const float* grad_loss, const void* ws,
                                         float* grad_image, void* stream_) {
    return photo_backward("photo_loss_backward", image, target, nullptr, C, H, W, lambda_dssim, weight, grad_loss, ws, grad_image,
                          (hipStream_t)stream_, PhotoFinal{});
}

extern "C" int syn3r_photo_loss_step(const float* image, const float* target, int C, int H, int W, float lambda_dssim,
                                     float weight, const float* grad_loss, float* loss3, float* grad_image, void* ws,
                                     size_t ws_bytes, void* stream_) {
    return photo_step("photo_loss_step", image, target, nullptr, C, H, W, lambda_dssim, weight, grad_loss, loss3, grad_image, ws, ws_bytes,
                      (hipStream_t)stream_);
}

// ---- the same three entries with a per-pixel weight map (an extension: include/syn3r_hip.h)
extern "C" int syn3r_photo_loss_map(const float* image, const float* target, const float* map, int C, int H, int W, float lambda_dssim,
                                    float weight, float* loss4, void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(map, "photo_loss_map: null map");
    return photo_forward("photo_loss_map", image, target, map, C, H, W, lambda_dssim, weight, loss4, ws, ws_bytes, (hipStream_t)stream_, nullptr);
}

extern "C" int syn3r_photo_loss_map_backward(const float* image, const float* target, const float* map, int C, int H, int W,
                                             float lambda_dssim, float weight, const float* grad_loss, const void* ws,
                                             float* grad_image, void* stream_) {
    SYN3R_REQUIRE(map, "photo_loss_map_backward: null map");
    return photo_backward("photo_loss_map_backward", image, target, map, C, H, W, lambda_dssim, weight, grad_loss, ws, grad_image,
                          (hipStream_t)stream_, PhotoFinal{});
}

extern "C" int syn3r_photo_loss_map_step(const float* image, const float* target, const float* map, int C, int H, int W,
                                         float lambda_dssim, float weight, const float* grad_loss, float* loss4, float* grad_image,
                                         void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(map, "photo_loss_map_step: null map");
    return photo_step("photo_loss_map_step", image, target, map, C, H, W, lambda_dssim, weight, grad_loss, loss4, grad_image, ws, ws_bytes,
                      (hipStream_t)stream_);
}
