// LPIPS (VGG16) perceptual term of the trainer's loss: the element-wise / per-pixel pieces around the
// 3x3 convolutions (which run on the implicit-GEMM kernel of gemm.hip, syn3r_conv2d3x3_act_f16).
//
// The reference toggles `gsTrainer.opt.use_lpips_loss` for every refine (model/diffusionGS.py:1690,1697); the loss itself
// lives in FSGS (un-vendored) and calls the `lpips` package, which is not in /root/reference either.  What is restated is
// the PUBLISHED definition (Zhang et al. 2018, `lpips.LPIPS(net='vgg')` v0.1): inputs scaled to [-1,1], the fixed
// per-channel shift / scale, VGG16 features after relu1_2, 2_2, 3_3, 4_3, 5_3, each normalised to unit length over
// channels (eps 1e-10 added to the norm), squared difference, a learned non-negative 1x1 weighting, spatial mean, summed
// over the five layers.  Weights are the caller's (no checkpoint is reachable offline): PARITY UNPINNED, oracle =
// oracle/lpips_oracle.py (torch fp32).
//
// Layout: activations are channels-last fp16 [H*W, C] (the UNet's token-matrix layout); the image enters as [3,H,W] fp32
// in [0,1] and its gradient leaves in the same form.  Gradients travel through the fp16 convolutions multiplied by a loss
// scale (they are ~1e-9 unscaled: below fp16's subnormal range) which k_lpips_image_bwd divides out.
// All kernels are HBM-bound single passes.
//
// Split activations (the "fp16x2" mode of gs/lpips.py): a forward activation v is stored as the fp16 pair hi = half(v),
// lo = half(v - float(hi)), channels-last [H*W, 2C] with the hi plane in channels [0, C) and the lo plane in [C, 2C); every kernel
// below has a variant that reads such a tensor as float(hi) + float(lo) (exact in fp32).  What rounding an activation to ONE fp16
// costs is not its 5e-4 of value but the ReLU masks it flips in the layers above, in which the gradient is discontinuous
// (profiles/README.md, "LPIPS gradient error"); the gradients themselves stay single fp16 tensors [H*W, C] in both modes.
#include "common.h"

using namespace syn3r;

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

__constant__ float kShift[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float kScale[3] = {0.458f, 0.448f, 0.450f};

// [3,H,W] fp32 in [0,1] -> [H*W, 64] fp16: channel c = ((2x - 1) - shift_c) / scale_c, channels 3..63 zero (the convolution
// kernel wants Cin % 64 == 0).  SPLIT: every channel as a pair, hi in channels 0..2, lo in 3..5 (conv1_1's weights are repeated
// there), 6..63 zero
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_lpips_image(const float* __restrict__ img, long long hw, __half* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // one thread per (pixel, 8-channel chunk)
    if (i >= hw * 8) return;
    const long long p = i >> 3;
    const int ch = (int)(i & 7);
    half8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (_Float16)0.0f;
    if (ch == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float f = ((2.0f * img[c * hw + p] - 1.0f) - kShift[c]) / kScale[c];
            v[c] = (_Float16)f;
            if constexpr (SPLIT) v[3 + c] = (_Float16)(f - (float)v[c]);
        }
    }
    *(half8*)(out + p * 64 + ch * 8) = v;
}

// gradient wrt the [H*W, 64] input of conv1_1 (scaled by loss_scale) -> d loss / d image [3,H,W] fp32
__global__ void __launch_bounds__(256) k_lpips_image_bwd(const __half* __restrict__ g, long long hw, float inv_scale, float* __restrict__ d_img) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) d_img[c * hw + p] = __half2float(g[p * 64 + c]) * (2.0f / kScale[c]) * inv_scale;
}

// The first maximum of a window in row-major order (torch's rule)
__device__ __forceinline__ int first_max4(float va, float vb, float vc, float vd) {
    int arg = 0;
    float m = va;
    if (vb > m) { m = vb; arg = 1; }
    if (vc > m) { m = vc; arg = 2; }
    if (vd > m) { m = vd; arg = 3; }
    return arg;
}

// One 2x2 window of a map at 8 channels: hi[k] (and, SPLIT, lo[k]), k = the window's cell in row-major order
template <bool SPLIT>
struct Window {
    half8 hi[4], lo[4];
    // cell k at channel e as fp32 (the pair's sum is exact)
    __device__ __forceinline__ float val(int k, int e) const {
        if constexpr (SPLIT) return (float)hi[k][e] + (float)lo[k][e];
        else return (float)hi[k][e];
    }
    __device__ __forceinline__ int first_max(int e) const { return first_max4(val(0, e), val(1, e), val(2, e), val(3, e)); }
};

// the window (yo, xo) of x [H,W,C] (SPLIT: of a split map [H,W,2C])
template <bool SPLIT>
__device__ __forceinline__ Window<SPLIT> load_window(const __half* __restrict__ x, int W, int C, int yo, int xo, int ch) {
    const long long ld = SPLIT ? 2ll * C : C;
    const __half* s = x + ((long long)(2 * yo) * W + 2 * xo) * ld + ch * 8;
    Window<SPLIT> w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const __half* c = s + ((k >> 1) ? (long long)W * ld : 0) + ((k & 1) ? ld : 0);
        w.hi[k] = *(const half8*)c;
        if constexpr (SPLIT) w.lo[k] = *(const half8*)(c + C);
    }
    return w;
}

// 2x2 / stride-2 max pooling on [H,W,C] -> [H/2,W/2,C] (floor, as nn.MaxPool2d(2,2)).  SPLIT: [H,W,2C] -> [H/2,W/2,2C], the cells
// are compared as float(hi) + float(lo) and the winning PAIR is copied (ties in the sum: the first cell, as the backward below and torch)
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_maxpool2(const __half* __restrict__ x, int H, int W, int C, __half* __restrict__ y) {
    const int Ho = H / 2, Wo = W / 2, C8 = C / 8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)Ho * Wo * C8) return;
    const int ch = (int)(i % C8);
    const long long q = i / C8;
    const Window<SPLIT> w = load_window<SPLIT>(x, W, C, (int)(q / Wo), (int)(q % Wo), ch);
    half8 oh, ol;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if constexpr (SPLIT) {
            const int arg = w.first_max(e);
            oh[e] = arg == 0 ? w.hi[0][e] : (arg == 1 ? w.hi[1][e] : (arg == 2 ? w.hi[2][e] : w.hi[3][e]));
            ol[e] = arg == 0 ? w.lo[0][e] : (arg == 1 ? w.lo[1][e] : (arg == 2 ? w.lo[2][e] : w.lo[3][e]));
        } else {
            // not a selection by first_max4: fmaxf differs from it on NaN and on signed zeros, and this entry's bits are public
            oh[e] = (_Float16)fmaxf(fmaxf(w.val(0, e), w.val(1, e)), fmaxf(w.val(2, e), w.val(3, e)));
        }
    }
    __half* d = y + q * (SPLIT ? 2 : 1) * C;
    *(half8*)(d + ch * 8) = oh;
    if constexpr (SPLIT) *(half8*)(d + C + ch * 8) = ol;
}

// its backward: the gradient of an output cell goes to the FIRST maximum of its window (row-major order, as torch); cells of
// an odd last row / column receive zero.  gx is written in full (no accumulation: a pooled activation feeds nothing else).
// gy [H/2,W/2,C] and gx [H,W,C] are plain fp16 gradients in both modes.
template <bool SPLIT>
__global__ void __launch_bounds__(256) k_maxpool2_bwd(const __half* __restrict__ x, const __half* __restrict__ gy, int H, int W, int C,
                                                     __half* __restrict__ gx) {
    const int Ho = H / 2, Wo = W / 2, C8 = C / 8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)H * W * C8) return;
    const int ch = (int)(i % C8);
    const long long q = i / C8;
    const int xi = (int)(q % W), yi = (int)(q / W);
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (_Float16)0.0f;
    const int yo = yi >> 1, xo = xi >> 1;
    if (yo < Ho && xo < Wo) {
        const Window<SPLIT> w = load_window<SPLIT>(x, W, C, yo, xo, ch);
        const half8 g = *(const half8*)(gy + ((long long)yo * Wo + xo) * C + ch * 8);
        const int me = (yi & 1) * 2 + (xi & 1);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (w.first_max(e) == me) o[e] = g[e];
    }
    *(half8*)(gx + q * C + ch * 8) = o;
}

// 8 channels of pixel p of a feature map as fp32: [P, C] fp16, or (SPLIT) the pair sum of [P, 2C]
template <bool SPLIT>
__device__ __forceinline__ void load_feat8(const __half* __restrict__ f, long long p, int C, int sub, float (&v)[8]) {
    const __half* s = f + p * (SPLIT ? 2 * C : C) + sub * 8;
    const half8 h = *(const half8*)s;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)h[e];
    if constexpr (SPLIT) {
        const half8 l = *(const half8*)(s + C);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += (float)l[e];
    }
}

// One LPIPS layer on two feature maps a, b [P, C] fp16 (SPLIT: both [P, 2C] pairs) (C = 64 .. 512, a multiple of 64; LPR = C / 8 lanes per pixel):
//   value_p = sum_c w_c (a_c / (|a| + eps) - b_c / (|b| + eps))^2 ;  the layer's term is mean_p value_p.
// Forward: per-block partial sums (fixed order) -> k_lpips_finish adds them up.
template <int LPR, bool SPLIT>
__global__ void __launch_bounds__(256) k_lpips_layer(const __half* __restrict__ a, const __half* __restrict__ b, const float* __restrict__ w,
                                                    long long P, float* __restrict__ partial) {
    constexpr int C = LPR * 8, PPB = 256 / LPR;       // pixels per block
    const int sub = threadIdx.x % LPR;
    const long long p = (long long)blockIdx.x * PPB + threadIdx.x / LPR;
    float val = 0.0f;
    if (p < P) {
        float av[8], bv[8];
        load_feat8<SPLIT>(a, p, C, sub, av);
        load_feat8<SPLIT>(b, p, C, sub, bv);
        float sa = 0.0f, sb = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { sa += av[e] * av[e]; sb += bv[e] * bv[e]; }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) { sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64); }
        const float ra = 1.0f / (sqrtf(sa) + 1e-10f), rb = 1.0f / (sqrtf(sb) + 1e-10f);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = av[e] * ra - bv[e] * rb;
            val += w[sub * 8 + e] * d * d;
        }
    }
    // block sum in a fixed order: wave shuffles, then the 4 wave sums
    for (int o = 32; o > 0; o >>= 1) val += __shfl_xor(val, o, 64);
    __shared__ float ws[4];
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = val;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// out[0] (+)= sum(partial) / P, one block, fixed order
__global__ void __launch_bounds__(1024) k_lpips_finish(const float* __restrict__ partial, int n, float inv_P, int accumulate, float* __restrict__ out) {
    __shared__ float red[1024];
    float s = 0.0f;
    for (int i = threadIdx.x; i < n; i += 1024) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (accumulate ? out[0] : 0.0f) + red[0] * inv_P;
}

// Backward of one layer wrt a: with n = a / r, r = |a| + eps, e_c = 2 w_c (n_c - b_c / (|b| + eps)) / P,
//   d value / d a_k = e_k / r - (sum_c e_c a_c) a_k / (r^2 |a|)
// written (accumulate = 0) or added (1) to ga [P, C] fp16 (a single fp16 tensor in the SPLIT variant too), multiplied by `gscale` (upstream gradient x loss scale); the sum
// is then masked by a > 0 (the feature map is the output of a ReLU: what leaves is the gradient wrt its pre-activation).
template <int LPR, bool SPLIT>
__global__ void __launch_bounds__(256) k_lpips_layer_bwd(const __half* __restrict__ a, const __half* __restrict__ b, const float* __restrict__ w,
                                                        long long P, float gscale, int accumulate, __half* __restrict__ ga) {
    constexpr int C = LPR * 8, PPB = 256 / LPR;
    const int sub = threadIdx.x % LPR;
    const long long p = (long long)blockIdx.x * PPB + threadIdx.x / LPR;
    if (p >= P) return;                                  // (whole LPR-lane groups leave together: the shuffles below stay inside a group)
    float av[8], bv[8];
    load_feat8<SPLIT>(a, p, C, sub, av);
    load_feat8<SPLIT>(b, p, C, sub, bv);
    float sa = 0.0f, sb = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { sa += av[e] * av[e]; sb += bv[e] * bv[e]; }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) { sa += __shfl_xor(sa, o, 64); sb += __shfl_xor(sb, o, 64); }
    const float na = sqrtf(sa);
    const float ra = 1.0f / (na + 1e-10f), rb = 1.0f / (sqrtf(sb) + 1e-10f);
    float ev[8], dot = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        ev[e] = 2.0f * w[sub * 8 + e] * (av[e] * ra - bv[e] * rb) * gscale;
        dot += ev[e] * av[e];
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    const float k2 = na > 0.0f ? dot * ra * ra / na : 0.0f;
    half8 o;
    if (accumulate) o = *(const half8*)(ga + p * C + sub * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float g = ev[e] * ra - k2 * av[e];
        // `a` is a post-ReLU activation: the total gradient passes its ReLU here (zero where the activation is zero).
        // The gradient carries the loss scale (1024 H W / P_k) and a factor 1 / |a|: a pixel whose feature norm is tiny would
        // overflow fp16 to inf and the backward convolutions would spread inf / NaN into the image gradient - saturate.
        const float t = fminf(fmaxf((accumulate ? (float)o[e] : 0.0f) + g, -65504.0f), 65504.0f);
        o[e] = av[e] > 0.0f ? (_Float16)t : (_Float16)0.0f;
    }
    *(half8*)(ga + p * C + sub * 8) = o;
}

template <int LPR, bool SPLIT>
int launch_layer(const __half* a, const __half* b, const float* w, long long P, float* partial, hipStream_t stream) {
    const int blocks = (int)((P + 256 / LPR - 1) / (256 / LPR));
    SYN3R_LAUNCH_NAMED(SPLIT ? "k_lpips_layer_split" : "k_lpips_layer", (k_lpips_layer<LPR, SPLIT>), dim3(blocks), dim3(256), 0, stream, a, b, w, P, partial);
    return blocks;
}
template <int LPR, bool SPLIT>
void launch_layer_bwd(const __half* a, const __half* b, const float* w, long long P, float gscale, int acc, __half* ga, hipStream_t stream) {
    const int blocks = (int)((P + 256 / LPR - 1) / (256 / LPR));
    SYN3R_LAUNCH_NAMED(SPLIT ? "k_lpips_layer_bwd_split" : "k_lpips_layer_bwd", (k_lpips_layer_bwd<LPR, SPLIT>), dim3(blocks), dim3(256), 0, stream, a, b, w, P,
                       gscale, acc, ga);
}

template <bool SPLIT>
int lpips_layer(const void* a, const void* b, const float* w, long long P, int C, int accumulate, float* value, void* ws, size_t ws_bytes,
                void* stream_) {
    SYN3R_REQUIRE(a && b && w && value && ws, "lpips_layer: null argument");
    SYN3R_REQUIRE(P > 0 && P < (1ll << 31) && (C == 64 || C == 128 || C == 256 || C == 512), "lpips_layer: P=%lld, C=%d (64 / 128 / 256 / 512)", P, C);
    SYN3R_REQUIRE(ws_bytes >= syn3r_lpips_layer_workspace_bytes(P, C), "lpips_layer: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    float* partial = (float*)ws;
    int blocks = 0;
    const __half *ah = (const __half*)a, *bh = (const __half*)b;
    if (C == 64) blocks = launch_layer<8, SPLIT>(ah, bh, w, P, partial, stream);
    else if (C == 128) blocks = launch_layer<16, SPLIT>(ah, bh, w, P, partial, stream);
    else if (C == 256) blocks = launch_layer<32, SPLIT>(ah, bh, w, P, partial, stream);
    else blocks = launch_layer<64, SPLIT>(ah, bh, w, P, partial, stream);
    SYN3R_LAUNCH(k_lpips_finish, dim3(1), dim3(1024), 0, stream, (const float*)partial, blocks, 1.0f / (float)P, accumulate, value);
    SYN3R_LAUNCH_CHECK("lpips_layer launch");
    return SYN3R_OK;
}

template <bool SPLIT>
int lpips_layer_bwd(const void* a, const void* b, const float* w, long long P, int C, float gscale, int accumulate, void* grad_a, void* stream_) {
    SYN3R_REQUIRE(a && b && w && grad_a, "lpips_layer_bwd: null argument");
    SYN3R_REQUIRE(P > 0 && P < (1ll << 31) && (C == 64 || C == 128 || C == 256 || C == 512), "lpips_layer_bwd: P=%lld, C=%d", P, C);
    hipStream_t stream = (hipStream_t)stream_;
    const __half *ah = (const __half*)a, *bh = (const __half*)b;
    __half* g = (__half*)grad_a;
    const float gs = gscale / (float)P;
    if (C == 64) launch_layer_bwd<8, SPLIT>(ah, bh, w, P, gs, accumulate, g, stream);
    else if (C == 128) launch_layer_bwd<16, SPLIT>(ah, bh, w, P, gs, accumulate, g, stream);
    else if (C == 256) launch_layer_bwd<32, SPLIT>(ah, bh, w, P, gs, accumulate, g, stream);
    else launch_layer_bwd<64, SPLIT>(ah, bh, w, P, gs, accumulate, g, stream);
    SYN3R_LAUNCH_CHECK("lpips_layer_bwd launch");
    return SYN3R_OK;
}

// The host side of the image and pooling entries (`who`: the entry's name in error messages)
template <bool SPLIT>
int lpips_image(const char* who, const float* img, int H, int W, void* out, void* stream_) {
    SYN3R_REQUIRE(img && out && SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W), "%s: bad arguments H=%d W=%d", who, H, W);
    const long long hw = (long long)H * W;
    SYN3R_LAUNCH_NAMED(SPLIT ? "k_lpips_image_split" : "k_lpips_image", k_lpips_image<SPLIT>, dim3((unsigned)((hw * 8 + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream_, img, hw, (__half*)out);
    return check_launch(who);
}

template <bool SPLIT>
int maxpool2(const char* who, const void* x, int H, int W, int C, void* y, void* stream_) {
    SYN3R_REQUIRE(x && y && SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W) && H >= 2 && W >= 2 && SYN3R_DIM_OK(C) && C % 8 == 0, "%s: bad arguments H=%d W=%d C=%d", who, H, W, C);
    const long long n = (long long)(H / 2) * (W / 2) * (C / 8);
    SYN3R_LAUNCH_NAMED(SPLIT ? "k_maxpool2_split" : "k_maxpool2", k_maxpool2<SPLIT>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_,
                       (const __half*)x, H, W, C, (__half*)y);
    return check_launch(who);
}

template <bool SPLIT>
int maxpool2_bwd(const char* who, const void* x, const void* gy, int H, int W, int C, void* gx, void* stream_) {
    SYN3R_REQUIRE(x && gy && gx && SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W) && H >= 2 && W >= 2 && SYN3R_DIM_OK(C) && C % 8 == 0, "%s: bad arguments", who);
    const long long n = (long long)H * W * (C / 8);
    SYN3R_LAUNCH_NAMED(SPLIT ? "k_maxpool2_bwd_split" : "k_maxpool2_bwd", k_maxpool2_bwd<SPLIT>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream_, (const __half*)x, (const __half*)gy, H, W, C, (__half*)gx);
    return check_launch(who);
}

}  // namespace

extern "C" int syn3r_lpips_image_f16(const float* img, int H, int W, void* out, void* stream_) {
    return lpips_image<false>("lpips_image", img, H, W, out, stream_);
}

extern "C" int syn3r_lpips_image_bwd(const void* grad64, int H, int W, float loss_scale, float* d_img, void* stream_) {
    SYN3R_REQUIRE(grad64 && d_img && SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W) && loss_scale > 0.0f, "lpips_image_bwd: bad arguments");
    const long long hw = (long long)H * W;
    SYN3R_LAUNCH(k_lpips_image_bwd, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, (const __half*)grad64, hw,
                 1.0f / loss_scale, d_img);
    SYN3R_LAUNCH_CHECK("lpips_image_bwd launch");
    return SYN3R_OK;
}

extern "C" int syn3r_maxpool2_f16(const void* x, int H, int W, int C, void* y, void* stream_) {
    return maxpool2<false>("maxpool2", x, H, W, C, y, stream_);
}

extern "C" int syn3r_maxpool2_bwd_f16(const void* x, const void* gy, int H, int W, int C, void* gx, void* stream_) {
    return maxpool2_bwd<false>("maxpool2_bwd", x, gy, H, W, C, gx, stream_);
}

extern "C" size_t syn3r_lpips_layer_workspace_bytes(long long P, int C) {
    if (P <= 0 || C < 64 || C > 512 || C % 64) return 0;
    const long long ppb = 256 / (C / 8);
    return (size_t)((P + ppb - 1) / ppb) * 4 + 256;
}

// value[0] (+)= mean_p sum_c w_c (a_c/(|a|+eps) - b_c/(|b|+eps))^2     a, b [P, C] fp16; w [C] fp32; value fp32 (device)
extern "C" int syn3r_lpips_layer_f16(const void* a, const void* b, const float* w, long long P, int C, int accumulate, float* value,
                                     void* ws, size_t ws_bytes, void* stream_) {
    return lpips_layer<false>(a, b, w, P, C, accumulate, value, ws, ws_bytes, stream_);
}

// grad_a [P, C] fp16 (=, or += with accumulate) d(layer term)/d a * gscale
extern "C" int syn3r_lpips_layer_bwd_f16(const void* a, const void* b, const float* w, long long P, int C, float gscale, int accumulate,
                                         void* grad_a, void* stream_) {
    return lpips_layer_bwd<false>(a, b, w, P, C, gscale, accumulate, grad_a, stream_);
}

// ---- the split-activation entries: feature maps / activations are [.., 2C] pairs, gradients single fp16 tensors [.., C]
extern "C" int syn3r_lpips_image_split_f16(const float* img, int H, int W, void* out, void* stream_) {
    return lpips_image<true>("lpips_image_split", img, H, W, out, stream_);
}

extern "C" int syn3r_maxpool2_split_f16(const void* x, int H, int W, int C, void* y, void* stream_) {
    return maxpool2<true>("maxpool2_split", x, H, W, C, y, stream_);
}

extern "C" int syn3r_maxpool2_bwd_split_f16(const void* x, const void* gy, int H, int W, int C, void* gx, void* stream_) {
    return maxpool2_bwd<true>("maxpool2_bwd_split", x, gy, H, W, C, gx, stream_);
}

extern "C" int syn3r_lpips_layer_split_f16(const void* a, const void* b, const float* w, long long P, int C, int accumulate, float* value,
                                           void* ws, size_t ws_bytes, void* stream_) {
    return lpips_layer<true>(a, b, w, P, C, accumulate, value, ws, ws_bytes, stream_);
}

extern "C" int syn3r_lpips_layer_bwd_split_f16(const void* a, const void* b, const float* w, long long P, int C, float gscale, int accumulate,
                                               void* grad_a, void* stream_) {
    return lpips_layer_bwd<true>(a, b, w, P, C, gscale, accumulate, grad_a, stream_);
}
