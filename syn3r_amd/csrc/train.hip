// Trainer-loop pieces adjacent to the rasteriser: the L1 / MSE reductions with the L1 gradient (with and
// without a per-pixel weight map), the Adam update of the Gaussian parameters (one tensor, a table of tensors, two rates inside a
// row), the parameter activations and the densification statistics.  The fused L1 + SSIM loss is photo_loss.hip.
//
// The reference runs these inside FSGS' gsTrainer.training()/finetune() (call sites model/diffusionGS.py:139,
// 1640; un-vendored) as chains of torch elementwise kernels: the published 3DGS step is
// `Ll1 = |render - gt|.mean()` followed by torch.optim.Adam(eps=1e-15).  Here each is one pass over memory:
//   L1 forward   reads image + target once, deterministic two-level sum (no float atomics);
//   L1 backward  reads image + target once, writes w * go / n * sign(image - target) (go read on the device);
//   Adam         one kernel per parameter tensor, torch.optim.Adam's operation order (lerp / addcmul / addcdiv)
//                so the result matches the torch optimiser to rounding.
// HBM-bound: 8 B/element (forward), 12 B/element (backward), 28 B/element (Adam).
#include "plane_pass.h"

using namespace syn3r;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;

// SQ = false: sum |a - b| (L1); SQ = true: sum (a - b)^2 (the MSE behind the PSNR of the metric record)
template <bool SQ>
__device__ __forceinline__ float dist_term(float d) { return SQ ? d * d : fabsf(d); }

template <bool SQ>
__global__ void __launch_bounds__(kThreads) k_l1_partial(const float* __restrict__ a, const float* __restrict__ b,
                                                        long long n, float* __restrict__ partial) {
    float s = 0.0f;
    const long long n4 = n >> 2;
    const float4* a4 = (const float4*)a;
    const float4* b4 = (const float4*)b;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kThreads) {
        float4 x = a4[i], y = b4[i];
        s += (dist_term<SQ>(x.x - y.x) + dist_term<SQ>(x.y - y.y)) + (dist_term<SQ>(x.z - y.z) + dist_term<SQ>(x.w - y.w));
    }
    if (blockIdx.x == 0) {
        long long i = (n4 << 2) + threadIdx.x;
        if (i < n) s += dist_term<SQ>(a[i] - b[i]);
    }
    if (block_rows(s)) partial[blockIdx.x] = s;
}

// one block: fixed-order sum of the block partials (bitwise reproducible run to run)
__global__ void __launch_bounds__(kThreads) k_l1_final(const float* __restrict__ partial, int nblocks, float scale,
                                                      float* __restrict__ loss) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += kThreads) s += (double)partial[i];
    s = wave_sum_d(s);
    __shared__ double ws[kThreads / 64];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *loss = (float)(block_sum4(ws) * (double)scale);
}

__global__ void __launch_bounds__(kThreads) k_l1_grad(const float* __restrict__ a, const float* __restrict__ b,
                                                     long long n, float scale, const float* __restrict__ go,
                                                     float* __restrict__ grad) {
    const float g = scale * (go ? *go : 1.0f);
    auto sgn = [g](float d) { return d > 0.0f ? g : (d < 0.0f ? -g : 0.0f); };   // torch.sign: 0 at 0
    const long long n4 = n >> 2;
    const float4* a4 = (const float4*)a;
    const float4* b4 = (const float4*)b;
    float4* g4 = (float4*)grad;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kThreads) {
        float4 x = a4[i], y = b4[i];
        g4[i] = make_float4(sgn(x.x - y.x), sgn(x.y - y.y), sgn(x.z - y.z), sgn(x.w - y.w));
    }
    if (blockIdx.x == 0) {
        long long i = (n4 << 2) + threadIdx.x;
        if (i < n) grad[i] = sgn(a[i] - b[i]);
    }
}

// The L1 pair with a per-pixel weight map m [plane] shared by the n / plane channels (syn3r_l1_loss_map: an extension, see the
// header): element i belongs to pixel i % plane.  A thread's group of four starts at pixel `pix`, found with ONE 64-bit
// remainder before the grid-stride loop and advanced by the stride's remainder afterwards.  VEC: plane % 4 == 0 and m 16-byte
// aligned, so the four weights are one aligned 16-byte load; else four loads whose pixel wraps at the plane's end.
// i % plane for 0 <= i < 2^52, plane > 0: the quotient from one fp64 division (off by one at most, corrected) - a 64-bit integer
// remainder is ~150 instructions, three of them were most of these kernels
__device__ __forceinline__ long long l1_map_rem(long long i, long long plane) {
    long long r = i - (long long)((double)i / (double)plane) * plane;
    if (r < 0) r += plane;
    if (r >= plane) r -= plane;
    return r;
}
struct L1MapWalk { long long pix, step; };
__device__ __forceinline__ L1MapWalk l1_map_walk(long long plane) {
    L1MapWalk w;
    w.pix = l1_map_rem(((long long)blockIdx.x * kThreads + threadIdx.x) * 4, plane);
    w.step = l1_map_rem((long long)gridDim.x * kThreads * 4, plane);
    return w;
}
template <bool VEC>
__device__ __forceinline__ float4 l1_map_load4(const float* __restrict__ m, long long pix, long long plane) {
    if constexpr (VEC) {
        return *(const float4*)(m + pix);
    } else {
        long long p[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) { p[e] = pix + e; if (p[e] >= plane) p[e] = l1_map_rem(p[e], plane); }
        return make_float4(m[p[0]], m[p[1]], m[p[2]], m[p[3]]);
    }
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) k_l1_partial_map(const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ m, long long n, long long plane,
                                                            float* __restrict__ partial) {
    float s = 0.0f;
    const long long n4 = n >> 2;
    const float4* a4 = (const float4*)a;
    const float4* b4 = (const float4*)b;
    L1MapWalk wk = l1_map_walk(plane);
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kThreads) {
        float4 x = a4[i], y = b4[i];
        const float4 w = l1_map_load4<VEC>(m, wk.pix, plane);
        s += (w.x * fabsf(x.x - y.x) + w.y * fabsf(x.y - y.y)) + (w.z * fabsf(x.z - y.z) + w.w * fabsf(x.w - y.w));
        wk.pix += wk.step;
        if (wk.pix >= plane) wk.pix -= plane;
    }
    if (blockIdx.x == 0) {
        long long i = (n4 << 2) + threadIdx.x;
        if (i < n) s += m[l1_map_rem(i, plane)] * fabsf(a[i] - b[i]);
    }
    if (block_rows(s)) partial[blockIdx.x] = s;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads) k_l1_grad_map(const float* __restrict__ a, const float* __restrict__ b,
                                                         const float* __restrict__ m, long long n, long long plane, float scale,
                                                         const float* __restrict__ go, float* __restrict__ grad) {
    const float g = scale * (go ? *go : 1.0f);
    auto sgn = [g](float d) { return d > 0.0f ? g : (d < 0.0f ? -g : 0.0f); };   // torch.sign: 0 at 0
    const long long n4 = n >> 2;
    const float4* a4 = (const float4*)a;
    const float4* b4 = (const float4*)b;
    float4* g4 = (float4*)grad;
    L1MapWalk wk = l1_map_walk(plane);
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (long long)gridDim.x * kThreads) {
        float4 x = a4[i], y = b4[i];
        const float4 w = l1_map_load4<VEC>(m, wk.pix, plane);
        g4[i] = make_float4(w.x * sgn(x.x - y.x), w.y * sgn(x.y - y.y), w.z * sgn(x.z - y.z), w.w * sgn(x.w - y.w));
        wk.pix += wk.step;
        if (wk.pix >= plane) wk.pix -= plane;
    }
    if (blockIdx.x == 0) {
        long long i = (n4 << 2) + threadIdx.x;
        if (i < n) grad[i] = m[l1_map_rem(i, plane)] * sgn(a[i] - b[i]);
    }
}

// torch.optim.Adam (_single_tensor_adam / _multi_tensor_adam, no weight decay, no amsgrad, not maximize):
//   exp_avg.lerp_(grad, 1 - beta1);  exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
//   denom = exp_avg_sq.sqrt() / sqrt(1 - beta2^t) + eps;  param.addcdiv_(exp_avg, denom, value = -lr / (1 - beta1^t))
__global__ void __launch_bounds__(kThreads) k_adam(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ m, float* __restrict__ v, long long n,
                                                  float w1 /*1-beta1*/, float beta2, float w2 /*1-beta2*/,
                                                  float bc2_sqrt, float eps, float neg_step) {
    long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    float mi = m[i], vi = v[i];
    mi = mi + w1 * (gi - mi);                    // lerp with weight < 0.5
    vi = vi * beta2 + (w2 * gi) * gi;            // addcmul: value * t1 * t2
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = p[i] + neg_step * (mi / denom);       // addcdiv: value * (t1 / t2)
    m[i] = mi;
    v[i] = vi;
}

// The same update for up to kAdamMulti tensors in ONE launch (round 6): a descriptor table travels as the kernel
// argument, a block finds its tensor by the table's block offsets.  Element for element the arithmetic of k_adam (bit-identical);
// what it saves is the launches (the trainer's five / six parameter groups: 60 us of HBM-bound work in 5 launches - the bytes
// stay, 330 MB per step at 200 000 Gaussians).
constexpr int kAdamMulti = 8;
struct AdamTable {
    float* p[kAdamMulti]; const float* g[kAdamMulti]; float* m[kAdamMulti]; float* v[kAdamMulti];
    long long n[kAdamMulti];
    float neg_step[kAdamMulti], eps[kAdamMulti], bc2_sqrt[kAdamMulti];
    unsigned blk0[kAdamMulti + 1];
    int count;
    float w1, beta2, w2;
};
__global__ void __launch_bounds__(kThreads) k_adam_multi(AdamTable t) {
    int k = 0;
#pragma unroll
    for (int q = 1; q < kAdamMulti; ++q) k += (q < t.count && blockIdx.x >= t.blk0[q]) ? 1 : 0;
    const long long i = (long long)(blockIdx.x - t.blk0[k]) * kThreads + threadIdx.x;
    if (i >= t.n[k]) return;
    float* __restrict__ p = t.p[k]; const float* __restrict__ g = t.g[k]; float* __restrict__ m = t.m[k]; float* __restrict__ v = t.v[k];
    const float gi = g[i];
    float mi = m[i], vi = v[i];
    mi = mi + t.w1 * (gi - mi);
    vi = vi * t.beta2 + (t.w2 * gi) * gi;
    const float denom = sqrtf(vi) / t.bc2_sqrt[k] + t.eps[k];
    p[i] = p[i] + t.neg_step[k] * (mi / denom);
    m[i] = mi;
    v[i] = vi;
}

// k_adam_multi with TWO learning rates inside a row of a tensor (the published 3DGS optimiser: f_dc at feature_lr, f_rest at
// feature_lr / 20, here ONE contiguous [N, M, 3] tensor because the rasteriser takes one `shs` pointer): element i of tensor k takes
// neg_step[k] when i % row_len[k] < head_len[k], neg_step_tail[k] otherwise; row_len[k] == 0 is a plain tensor (no column arithmetic:
// the branch is on a table entry, uniform per block).  Otherwise element for element k_adam_multi (bit-identical with equal rates).
// The split costs no bytes.  256 threads do not divide a 48-float row, so the column of a block's first element differs per block:
//   col0 = (block's first element) % row_len   scalar unit only: Lemire / Kaser / Kurz 2019 ("Faster remainder by direct
//          computation"), a % d = mulhi64(M * a mod 2^64, d) with M = floor((2^64 - 1) / d) + 1, exact for every 32-bit a and d >= 1
//          (the entry refuses a split tensor of 2^31 elements or more);
//   tcol = thread % row_len = thread - ((thread * ceil(2^16 / row_len)) >> 16) * row_len: exact for thread < 256 and row_len <= 255
//          (the error of the quotient is thread * (magic * row_len - 2^16) / 2^16 < 255 * 255 / 2^16 < 1); row_len >= 256 has magic 0;
//   col  = min(x, x - row_len) in unsigned arithmetic with x = col0 + tcol < 2 row_len (x - row_len wraps above x when x < row_len).
struct AdamRowsTable {
    AdamTable t;
    float neg_step_tail[kAdamMulti];
    unsigned row_len[kAdamMulti], head_len[kAdamMulti], tid_magic[kAdamMulti];
    unsigned long long row_magic[kAdamMulti];
};
__global__ void __launch_bounds__(kThreads) k_adam_multi_rows(AdamRowsTable r) {
    const AdamTable& t = r.t;
    int k = 0;
#pragma unroll
    for (int q = 1; q < kAdamMulti; ++q) k += (q < t.count && blockIdx.x >= t.blk0[q]) ? 1 : 0;
    const unsigned blk = blockIdx.x - t.blk0[k];
    const long long i = (long long)blk * kThreads + threadIdx.x;
    if (i >= t.n[k]) return;
    float neg_step = t.neg_step[k];
    const unsigned row = r.row_len[k];
    if (row != 0) {
        const unsigned col0 = (unsigned)__umul64hi(r.row_magic[k] * (unsigned long long)(blk * (unsigned)kThreads), (unsigned long long)row);
        const unsigned x = col0 + threadIdx.x - __umul24(__umul24(threadIdx.x, r.tid_magic[k]) >> 16, row);
        const float tail = r.neg_step_tail[k];             // read before the select: a load in one arm of ?: is a divergent branch
        neg_step = min(x, x - row) < r.head_len[k] ? neg_step : tail;
    }
    float* __restrict__ p = t.p[k]; const float* __restrict__ g = t.g[k]; float* __restrict__ m = t.m[k]; float* __restrict__ v = t.v[k];
    const float gi = g[i];
    float mi = m[i], vi = v[i];
    mi = mi + t.w1 * (gi - mi);
    vi = vi * t.beta2 + (t.w2 * gi) * gi;
    const float denom = sqrtf(vi) / t.bc2_sqrt[k] + t.eps[k];
    p[i] = p[i] + neg_step * (mi / denom);
    m[i] = mi;
    v[i] = vi;
}

// ---------------------------------------------------------------------------------------------
// The published 3DGS parameter activations (GaussianModel.get_scaling / get_rotation / get_opacity: exp, normalize, sigmoid;
// FSGS' trainer behind gsTrainer.training() / finetune(), model/diffusionGS.py:139,1640) as ONE launch forward and ONE launch
// for the chain rule backward, instead of three torch operators + their ~10 autograd kernels per training iteration.
// torch's formulas: normalize = x / max(|x|_2, 1e-12); d/dx = (g - xhat (xhat . g)) / max(|x|, eps);
// sigmoid' = s (1 - s); exp' = e.
__global__ void __launch_bounds__(kThreads) k_activate(int N, const float* __restrict__ log_scale, const float* __restrict__ rot,
                                                       const float* __restrict__ logit, float* __restrict__ scale,
                                                       float* __restrict__ rot_n, float* __restrict__ opacity) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) scale[3 * i + c] = act_exp(log_scale[3 * i + c]);
    const float4 q = *(const float4*)(rot + 4 * i);
    *(float4*)(rot_n + 4 * i) = act_quat(q, act_quat_inv_norm(q));
    opacity[i] = act_sigmoid(logit[i]);
}

__global__ void __launch_bounds__(kThreads) k_activate_bwd(int N, const float* __restrict__ rot, const float* __restrict__ scale,
                                                           const float* __restrict__ rot_n, const float* __restrict__ opacity,
                                                           const float* __restrict__ d_scale, const float* __restrict__ d_rot_n,
                                                           const float* __restrict__ d_opacity, float* __restrict__ d_log_scale,
                                                           float* __restrict__ d_rot, float* __restrict__ d_logit) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) d_log_scale[3 * i + c] = d_scale[3 * i + c] * scale[3 * i + c];
    const float4 q = *(const float4*)(rot + 4 * i), h = *(const float4*)(rot_n + 4 * i), g = *(const float4*)(d_rot_n + 4 * i);
    *(float4*)(d_rot + 4 * i) = act_quat_bwd(h, g, act_quat_inv_norm(q));
    d_logit[i] = act_sigmoid_bwd(opacity[i], d_opacity[i]);
}

// GaussianModel.add_densification_stats of the published trainer for the visible Gaussians (radii > 0): torch.norm(grad[:, :2]) is
// sqrt(gx*gx + gy*gy) in fp32 (this file compiles without fma contraction).  ABS (syn3r_densification_stats_abs): the same norm of
// the rasteriser's absolute screen-space gradient ([N,2]) goes into a second accumulator, the statistic AbsGS splits on.
template <bool ABS>
__device__ __forceinline__ void densify_stats(int N, const int* __restrict__ radii, const float* __restrict__ vgrad,
                                              const float* __restrict__ agrad, float* __restrict__ accum,
                                              float* __restrict__ accum_abs, float* __restrict__ denom, float* __restrict__ max_radii) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    const int r = radii[i];
    if (r <= 0) return;
    const float gx = vgrad[3 * i], gy = vgrad[3 * i + 1];
    accum[i] += sqrtf(gx * gx + gy * gy);
    if constexpr (ABS) {
        const float ax = agrad[2 * i], ay = agrad[2 * i + 1];
        accum_abs[i] += sqrtf(ax * ax + ay * ay);
    }
    denom[i] += 1.0f;
    max_radii[i] = fmaxf(max_radii[i], (float)r);
}
__global__ void __launch_bounds__(kThreads) k_densify_stats(int N, const int* __restrict__ radii, const float* __restrict__ vgrad,
                                                           float* __restrict__ accum, float* __restrict__ denom,
                                                           float* __restrict__ max_radii) {
    densify_stats<false>(N, radii, vgrad, nullptr, accum, nullptr, denom, max_radii);
}
__global__ void __launch_bounds__(kThreads) k_densify_stats_abs(int N, const int* __restrict__ radii, const float* __restrict__ vgrad,
                                                               const float* __restrict__ agrad, float* __restrict__ accum,
                                                               float* __restrict__ accum_abs, float* __restrict__ denom,
                                                               float* __restrict__ max_radii) {
    densify_stats<true>(N, radii, vgrad, agrad, accum, accum_abs, denom, max_radii);
}

// grid of the L1 kernels: `per_thread` groups of four elements per thread, between 1 and `cap` blocks (grid-stride beyond)
int l1_blocks(long long n, int per_thread, int cap) {
    long long b = (n / 4 + kThreads * per_thread - 1) / (kThreads * per_thread);
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// one 16-byte load of four weights: the plane is whole groups of four and the map is aligned
bool l1_map_vec(const float* map, long long plane) { return plane % 4 == 0 && ((uintptr_t)map & 15) == 0; }

}  // namespace

extern "C" size_t syn3r_l1_loss_workspace_bytes(long long n) { return n > 0 ? (size_t)kMaxBlocks * sizeof(float) : 0; }

// *out = weight / n * sum of the (weighted) terms: syn3r_l1_loss (sq false), syn3r_image_mse (sq true, no map) and
// syn3r_l1_loss_map (`map` [plane]; null: none)
static int l1_forward(const char* who, bool sq, const float* image, const float* target, const float* map, long long n, long long plane,
                      float weight, float* out, void* ws, size_t ws_bytes, hipStream_t stream) {
    SYN3R_REQUIRE(n > 0, "%s: n must be positive", who);
    SYN3R_REQUIRE(image && target && out && ws, "%s: null pointer", who);
    SYN3R_REQUIRE(ws_bytes >= syn3r_l1_loss_workspace_bytes(n), "%s: workspace too small", who);
    SYN3R_REQUIRE((((uintptr_t)image | (uintptr_t)target) & 15) == 0, "%s: image/target must be 16-byte aligned", who);
    const int nb = l1_blocks(n, 8, kMaxBlocks);
    const dim3 grid(nb), block(kThreads);
    if (sq) SYN3R_LAUNCH(k_l1_partial<true>, grid, block, 0, stream, image, target, n, (float*)ws);
    else if (!map) SYN3R_LAUNCH(k_l1_partial<false>, grid, block, 0, stream, image, target, n, (float*)ws);
    else if (l1_map_vec(map, plane)) SYN3R_LAUNCH(k_l1_partial_map<true>, grid, block, 0, stream, image, target, map, n, plane, (float*)ws);
    else SYN3R_LAUNCH(k_l1_partial_map<false>, grid, block, 0, stream, image, target, map, n, plane, (float*)ws);
    SYN3R_LAUNCH(k_l1_final, dim3(1), dim3(kThreads), 0, stream, (const float*)ws, nb, weight / (float)n, out);
    return check_launch(who);
}

static int l1_backward(const char* who, const float* image, const float* target, const float* map, long long n, long long plane,
                       float weight, const float* grad_loss, float* grad_image, hipStream_t stream) {
    SYN3R_REQUIRE(n > 0, "%s: n must be positive", who);
    SYN3R_REQUIRE(image && target && grad_image, "%s: null pointer", who);
    SYN3R_REQUIRE((((uintptr_t)image | (uintptr_t)target | (uintptr_t)grad_image) & 15) == 0, "%s: buffers must be 16-byte aligned", who);
    const int nb = l1_blocks(n, 4, 4 * kMaxBlocks);
    const dim3 grid(nb), block(kThreads);
    const float scale = weight / (float)n;
    if (!map) SYN3R_LAUNCH(k_l1_grad, grid, block, 0, stream, image, target, n, scale, grad_loss, grad_image);
    else if (l1_map_vec(map, plane)) SYN3R_LAUNCH(k_l1_grad_map<true>, grid, block, 0, stream, image, target, map, n, plane, scale, grad_loss, grad_image);
    else SYN3R_LAUNCH(k_l1_grad_map<false>, grid, block, 0, stream, image, target, map, n, plane, scale, grad_loss, grad_image);
    return check_launch(who);
}

extern "C" int syn3r_l1_loss(const float* image, const float* target, long long n, float weight, float* loss,
                             void* ws, size_t ws_bytes, void* stream_) {
    return l1_forward("l1_loss", false, image, target, nullptr, n, 0, weight, loss, ws, ws_bytes, (hipStream_t)stream_);
}

extern "C" int syn3r_image_mse(const float* image, const float* target, long long n, float* mse, void* ws,
                               size_t ws_bytes, void* stream_) {
    return l1_forward("image_mse", true, image, target, nullptr, n, 0, 1.0f, mse, ws, ws_bytes, (hipStream_t)stream_);
}

extern "C" int syn3r_l1_loss_backward(const float* image, const float* target, long long n, float weight,
                                      const float* grad_loss, float* grad_image, void* stream_) {
    return l1_backward("l1_loss_backward", image, target, nullptr, n, 0, weight, grad_loss, grad_image, (hipStream_t)stream_);
}

extern "C" int syn3r_l1_loss_map(const float* image, const float* target, const float* map, long long n, long long plane,
                                 float weight, float* loss, void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(n > 0 && plane > 0 && n % plane == 0, "l1_loss_map: n and plane must be positive, n a multiple of plane");
    SYN3R_REQUIRE(map, "l1_loss_map: null map");
    return l1_forward("l1_loss_map", false, image, target, map, n, plane, weight, loss, ws, ws_bytes, (hipStream_t)stream_);
}

extern "C" int syn3r_l1_loss_map_backward(const float* image, const float* target, const float* map, long long n, long long plane,
                                          float weight, const float* grad_loss, float* grad_image, void* stream_) {
    SYN3R_REQUIRE(n > 0 && plane > 0 && n % plane == 0, "l1_loss_map_backward: n and plane must be positive, n a multiple of plane");
    SYN3R_REQUIRE(map, "l1_loss_map_backward: null map");
    return l1_backward("l1_loss_map_backward", image, target, map, n, plane, weight, grad_loss, grad_image, (hipStream_t)stream_);
}

// torch's scalar factors of step `step` (1-based), computed as torch does: in double on the host
struct AdamBias { float neg_step /* -lr / (1 - beta1^t) */, bc2_sqrt /* sqrt(1 - beta2^t) */; };
static AdamBias adam_bias(float beta1, float beta2, int step, float lr) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    return {(float)(-((double)lr / bc1)), (float)sqrt(bc2)};
}

extern "C" int syn3r_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n,
                               float lr, float beta1, float beta2, float eps, int step, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SYN3R_REQUIRE(n > 0, "adam_step: n must be positive");
    SYN3R_REQUIRE(param && grad && exp_avg && exp_avg_sq, "adam_step: null pointer");
    SYN3R_REQUIRE(step >= 1, "adam_step: step is 1-based");
    SYN3R_REQUIRE(beta1 >= 0.5f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f, "adam_step: betas out of range");
    const AdamBias bias = adam_bias(beta1, beta2, step, lr);
    long long b = (n + kThreads - 1) / kThreads;
    SYN3R_REQUIRE(b < (1ll << 31), "adam_step: tensor too large");
    SYN3R_LAUNCH(k_adam, dim3((unsigned)b), dim3(kThreads), 0, stream, param, grad, exp_avg, exp_avg_sq, n,
                 (float)(1.0 - (double)beta1), beta2, (float)(1.0 - (double)beta2), bias.bc2_sqrt, eps, bias.neg_step);
    SYN3R_LAUNCH_CHECK("adam_step launch");
    return SYN3R_OK;
}

// The descriptor table of both multi-tensor entries from the ABI's arrays: every check the two share, the scalar factors per tensor,
// the block offsets (padded past `count`: the kernels' search reads all of blk0).  Returns the grid size, or a (negative) status.
static long long adam_fill(const char* who, AdamTable& t, int count, float* const* params, const float* const* grads,
                           float* const* exp_avgs, float* const* exp_avg_sqs, const long long* numels, const float* lrs, float beta1,
                           float beta2, const float* epss, const int* steps) {
    SYN3R_REQUIRE(count >= 1 && count <= kAdamMulti, "%s: count=%d must be 1..%d", who, count, kAdamMulti);
    SYN3R_REQUIRE(params && grads && exp_avgs && exp_avg_sqs && numels && lrs && epss && steps, "%s: null table", who);
    SYN3R_REQUIRE(beta1 >= 0.5f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f, "%s: betas out of range", who);
    t.count = count;
    t.w1 = (float)(1.0 - (double)beta1); t.beta2 = beta2; t.w2 = (float)(1.0 - (double)beta2);
    long long blocks = 0;
    for (int k = 0; k < count; ++k) {
        SYN3R_REQUIRE(params[k] && grads[k] && exp_avgs[k] && exp_avg_sqs[k], "%s: null pointer in tensor %d", who, k);
        SYN3R_REQUIRE(numels[k] > 0 && steps[k] >= 1, "%s: tensor %d: n must be positive, step 1-based", who, k);
        const AdamBias bias = adam_bias(beta1, beta2, steps[k], lrs[k]);
        t.p[k] = params[k]; t.g[k] = grads[k]; t.m[k] = exp_avgs[k]; t.v[k] = exp_avg_sqs[k]; t.n[k] = numels[k];
        t.neg_step[k] = bias.neg_step; t.bc2_sqrt[k] = bias.bc2_sqrt; t.eps[k] = epss[k];
        t.blk0[k] = (unsigned)blocks;
        blocks += (numels[k] + kThreads - 1) / kThreads;
        SYN3R_REQUIRE(blocks < (1ll << 31), "%s: tensors too large", who);
    }
    for (int k = count; k <= kAdamMulti; ++k) t.blk0[k] = (unsigned)blocks;
    return blocks;
}

extern "C" int syn3r_adam_step_multi(int count, float* const* params, const float* const* grads, float* const* exp_avgs,
                                     float* const* exp_avg_sqs, const long long* numels, const float* lrs, float beta1, float beta2,
                                     const float* epss, const int* steps, void* stream_) {
    AdamTable t{};
    const long long blocks = adam_fill("adam_step_multi", t, count, params, grads, exp_avgs, exp_avg_sqs, numels, lrs, beta1, beta2, epss, steps);
    if (blocks < 0) return (int)blocks;
    SYN3R_LAUNCH(k_adam_multi, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_, t);
    SYN3R_LAUNCH_CHECK("adam_step_multi launch");
    return SYN3R_OK;
}

extern "C" int syn3r_adam_step_multi_rows(int count, float* const* params, const float* const* grads, float* const* exp_avgs,
                                          float* const* exp_avg_sqs, const long long* numels, const float* lrs, const float* lrs_tail,
                                          const int* row_lens, const int* head_lens, float beta1, float beta2, const float* epss,
                                          const int* steps, void* stream_) {
    AdamRowsTable r{};
    const long long blocks = adam_fill("adam_step_multi_rows", r.t, count, params, grads, exp_avgs, exp_avg_sqs, numels, lrs, beta1, beta2, epss,
                                       steps);
    if (blocks < 0) return (int)blocks;
    SYN3R_REQUIRE(row_lens && head_lens, "adam_step_multi_rows: null table");
    for (int k = 0; k < count; ++k) {
        const int row = row_lens[k], head = head_lens[k];
        SYN3R_REQUIRE(row >= 0, "adam_step_multi_rows: tensor %d: row_len=%d is negative", k, row);
        if (row == 0) continue;
        SYN3R_REQUIRE(lrs_tail, "adam_step_multi_rows: tensor %d has a row split and lrs_tail is null", k);
        SYN3R_REQUIRE(head >= 0 && head <= row, "adam_step_multi_rows: tensor %d: head_len=%d must be 0..row_len=%d", k, head, row);
        SYN3R_REQUIRE(numels[k] % row == 0, "adam_step_multi_rows: tensor %d: n=%lld is no multiple of row_len=%d", k, numels[k], row);
        SYN3R_REQUIRE(numels[k] < (1ll << 31), "adam_step_multi_rows: tensor %d: a split tensor must have fewer than 2^31 elements", k);
        r.neg_step_tail[k] = adam_bias(beta1, beta2, steps[k], lrs_tail[k]).neg_step;
        r.row_len[k] = (unsigned)row; r.head_len[k] = (unsigned)head;
        r.tid_magic[k] = row < kThreads ? (65536u + (unsigned)row - 1u) / (unsigned)row : 0u;
        r.row_magic[k] = ~0ull / (unsigned long long)row + 1ull;
    }
    SYN3R_LAUNCH(k_adam_multi_rows, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream_, r);
    SYN3R_LAUNCH_CHECK("adam_step_multi_rows launch");
    return SYN3R_OK;
}

extern "C" int syn3r_gaussian_activate(int N, const float* log_scales, const float* rotations, const float* opacity_logits,
                                       float* scales, float* rotations_n, float* opacities, void* stream_) {
    SYN3R_REQUIRE(SYN3R_DIM_OK(N), "gaussian_activate: bad N=%d", N);
    SYN3R_REQUIRE(log_scales && rotations && opacity_logits && scales && rotations_n && opacities, "gaussian_activate: null pointer");
    SYN3R_REQUIRE((((uintptr_t)rotations | (uintptr_t)rotations_n) % 16) == 0, "gaussian_activate: quaternions must be 16-byte aligned");
    SYN3R_LAUNCH(k_activate, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream_, N, log_scales,
                 rotations, opacity_logits, scales, rotations_n, opacities);
    SYN3R_LAUNCH_CHECK("gaussian_activate launch");
    return SYN3R_OK;
}

extern "C" int syn3r_gaussian_activate_backward(int N, const float* rotations, const float* scales, const float* rotations_n,
                                                const float* opacities, const float* d_scales, const float* d_rotations_n,
                                                const float* d_opacities, float* d_log_scales, float* d_rotations,
                                                float* d_opacity_logits, void* stream_) {
    SYN3R_REQUIRE(SYN3R_DIM_OK(N), "gaussian_activate_backward: bad N=%d", N);
    SYN3R_REQUIRE(rotations && scales && rotations_n && opacities && d_scales && d_rotations_n && d_opacities && d_log_scales &&
                  d_rotations && d_opacity_logits, "gaussian_activate_backward: null pointer");
    SYN3R_REQUIRE((((uintptr_t)rotations | (uintptr_t)rotations_n | (uintptr_t)d_rotations_n | (uintptr_t)d_rotations) % 16) == 0,
                  "gaussian_activate_backward: quaternion tensors must be 16-byte aligned");
    SYN3R_LAUNCH(k_activate_bwd, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream_, N, rotations,
                 scales, rotations_n, opacities, d_scales, d_rotations_n, d_opacities, d_log_scales, d_rotations, d_opacity_logits);
    SYN3R_LAUNCH_CHECK("gaussian_activate_backward launch");
    return SYN3R_OK;
}

// both statistics entries; ABS: k_densify_stats_abs with its two extra pointers, else they are unused
static int densification_stats(const char* who, bool abs, int N, const int* radii, const float* viewspace_grad, const float* abs_grad,
                               float* grad_accum, float* grad_accum_abs, float* denom, float* max_radii, hipStream_t stream) {
    SYN3R_REQUIRE(SYN3R_DIM_OK(N), "%s: bad N=%d", who, N);
    SYN3R_REQUIRE(radii && viewspace_grad && grad_accum && denom && max_radii && (!abs || (abs_grad && grad_accum_abs)), "%s: null pointer", who);
    const dim3 grid((unsigned)((N + kThreads - 1) / kThreads)), block(kThreads);
    if (abs) SYN3R_LAUNCH(k_densify_stats_abs, grid, block, 0, stream, N, radii, viewspace_grad, abs_grad, grad_accum, grad_accum_abs, denom, max_radii);
    else SYN3R_LAUNCH(k_densify_stats, grid, block, 0, stream, N, radii, viewspace_grad, grad_accum, denom, max_radii);
    return check_launch(who);
}

extern "C" int syn3r_densification_stats(int N, const int* radii, const float* viewspace_grad, float* grad_accum, float* denom,
                                         float* max_radii, void* stream_) {
    return densification_stats("densification_stats", false, N, radii, viewspace_grad, nullptr, grad_accum, nullptr, denom, max_radii,
                               (hipStream_t)stream_);
}

extern "C" int syn3r_densification_stats_abs(int N, const int* radii, const float* viewspace_grad, const float* abs_grad,
                                             float* grad_accum, float* grad_accum_abs, float* denom, float* max_radii, void* stream_) {
    return densification_stats("densification_stats_abs", true, N, radii, viewspace_grad, abs_grad, grad_accum, grad_accum_abs, denom, max_radii,
                               (hipStream_t)stream_);
}
