// Depth-correlation regulariser of FSGS (Zhu et al., "FSGS: Real-Time Few-shot View Synthesis using Gaussian Splatting",
// ECCV 2024, section "geometry guidance"): L = weight * (1 - Pearson(rendered depth, monocular depth prior)).  The reference
// hands HOT LOOP A to FSGS' trainer (un-vendored submodule), which adds this term on every iteration; its batch scripts
// pass FSGS' depth switches (bash_scripts/batch_{llff,dl3dv}_train.sh: --svd_depth_warmup 1).
//
// Two transforms t of the prior p are correlated with the rendered depth d (n = H*W pixels):
//   A: t = -p               (the prior is disparity-like)
//   B: t = 1 / (p + c)      (c = `offset`, 200 by default)
// r_X = S_dt / sqrt(S_dd S_tt) with CENTRED sums, clamped to [-1, 1]; L_X = 1 - r_X; mode MIN takes min(L_A, L_B) (A on a
// tie, as Python's min), modes A / B one branch.  The gradient flows through the chosen branch only:
//   dL/dd_i = -weight * g * [ (t_i - t_mean) / sqrt(S_dd S_tt) - r (d_i - d_mean) / S_dd ]      (g: device scalar, NULL = 1)
// PROVENANCE: the two-transform minimum and c = 200 are recalled from FSGS' released train.py, which is not available to this
// project: UNPINNED.  Both are arguments (offset, mode).
// DEGENERATE INPUT: a branch with S_dd == 0 or S_tt == 0 (a flat render - an empty view - or a flat prior) has r := 0, loss 1
// and a zero gradient.  torchmetrics' pearson_corrcoef returns NaN there; a NaN would poison Adam's moments.
//
// Numerics: rendered depths sit at z ~ 1 .. 100 with a small spread, where sum(x^2) - n mean^2 cancels catastrophically.
// Every element is taken to fp64; a thread keeps sums SHIFTED by its own first element, turns them into centred moments
// (count, means, co-moments) once, and the moments of threads, waves, blocks are merged with Chan et al.'s pairwise formula
//   n = na + nb,  mean = mean_a + delta nb / n,  M_xy = M_xy,a + M_xy,b + delta_x delta_y na nb / n
// in a FIXED order (no float atomics anywhere: the loss and the gradient are bitwise repeatable).
//
// Launches: the statistics pass (grid-stride, 16-byte loads where d and p are aligned, a ragged scalar tail) writes one moment
// record per block; the gradient pass merges those records itself in every block (the same order everywhere, so every block
// holds the same bits - no combine launch, no counter) and writes dL/dd; its block 0 also writes the loss.  The value-only
// entry merges the records in a one-block launch.  Nothing travels to the host.
#include "common.h"

using namespace syn3r;

namespace {

constexpr int kDcThreads = 256;
constexpr int kDcMaxBlocks = 1024;
constexpr long long kDcMaxN = 1ll << 30;                // SYN3R_SIDE_MAX^2

// centred moments of a set of (d, p, u = 1 / (p + c)) triples
struct DcMom { double n, md, mp, mu, dd, pp, uu, dp, du; };

__device__ __forceinline__ DcMom dc_merge(const DcMom& a, const DcMom& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    DcMom o;
    o.n = a.n + b.n;
    const double w = b.n / o.n, f = a.n * w;
    const double xd = b.md - a.md, xp = b.mp - a.mp, xu = b.mu - a.mu;
    o.md = a.md + xd * w; o.mp = a.mp + xp * w; o.mu = a.mu + xu * w;
    o.dd = (a.dd + b.dd) + xd * xd * f;
    o.pp = (a.pp + b.pp) + xp * xp * f;
    o.uu = (a.uu + b.uu) + xu * xu * f;
    o.dp = (a.dp + b.dp) + xd * xp * f;
    o.du = (a.du + b.du) + xd * xu * f;
    return o;
}

__device__ __forceinline__ DcMom dc_shfl(const DcMom& a, int o) {
    DcMom b;
    b.n = __shfl_xor(a.n, o, 64); b.md = __shfl_xor(a.md, o, 64); b.mp = __shfl_xor(a.mp, o, 64); b.mu = __shfl_xor(a.mu, o, 64);
    b.dd = __shfl_xor(a.dd, o, 64); b.pp = __shfl_xor(a.pp, o, 64); b.uu = __shfl_xor(a.uu, o, 64);
    b.dp = __shfl_xor(a.dp, o, 64); b.du = __shfl_xor(a.du, o, 64);
    return b;
}

// moments of the whole block, returned to EVERY thread (fixed pairing: the lower lane / wave is the left operand)
__device__ DcMom dc_block_merge(DcMom m) {
    __shared__ DcMom wm[kDcThreads / 64];
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const DcMom b = dc_shfl(m, o);
        m = (lane & o) ? dc_merge(b, m) : dc_merge(m, b);
    }
    if (lane == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    static_assert(kDcThreads == 256, "dc_block_merge: four waves");
    const DcMom r = dc_merge(dc_merge(wm[0], wm[1]), dc_merge(wm[2], wm[3]));
    __syncthreads();
    return r;
}

// sums of one thread, shifted by its first element (exact zero for a constant input)
template <bool INV>
struct DcAcc {
    double n = 0.0, kd = 0.0, kp = 0.0, ku = 0.0, sd = 0.0, sp = 0.0, su = 0.0, sdd = 0.0, spp = 0.0, suu = 0.0, sdp = 0.0, sdu = 0.0;
    __device__ __forceinline__ void add(float df, float pf, double c) {
        const double d = (double)df, p = (double)pf, u = INV ? 1.0 / (p + c) : 0.0;
        if (n == 0.0) { kd = d; kp = p; ku = u; }
        const double x = d - kd, y = p - kp, z = u - ku;
        n += 1.0;
        sd += x; sp += y; sdd += x * x; spp += y * y; sdp += x * y;
        if (INV) { su += z; suu += z * z; sdu += x * z; }
    }
    __device__ __forceinline__ DcMom moments() const {
        DcMom m{};
        if (n == 0.0) return m;
        const double ad = sd / n, ap = sp / n, au = su / n;
        m.n = n;
        m.md = kd + ad; m.mp = kp + ap; m.mu = ku + au;
        m.dd = sdd - sd * ad; m.pp = spp - sp * ap; m.uu = suu - su * au;
        m.dp = sdp - sd * ap; m.du = sdu - sd * au;
        return m;
    }
};


// Grid-stride walk over the n elements: 16-byte groups of d and p (VEC: both 16-byte aligned), two groups in flight per trip,
// then the ragged tail one element per thread.  f(e, cnt, a, b): elements e .. e + cnt - 1 (cnt 4 or 1: only .x is valid).
template <bool VEC, typename F>
__device__ __forceinline__ void dc_walk(const float* __restrict__ d, const float* __restrict__ p, long long n, F&& f) {
    const long long stride = (long long)gridDim.x * kDcThreads, t0 = (long long)blockIdx.x * kDcThreads + threadIdx.x;
    const long long n4 = VEC ? (n >> 2) : 0;
    const float4* d4 = (const float4*)d;
    const float4* p4 = (const float4*)p;
    long long i = t0;
    for (; i + stride < n4; i += 2 * stride) {
        const float4 a0 = d4[i], b0 = p4[i], a1 = d4[i + stride], b1 = p4[i + stride];
        f(4 * i, 4, a0, b0);
        f(4 * (i + stride), 4, a1, b1);
    }
    if (i < n4) f(4 * i, 4, d4[i], p4[i]);
    for (long long j = (n4 << 2) + t0; j < n; j += stride) f(j, 1, make_float4(d[j], 0.f, 0.f, 0.f), make_float4(p[j], 0.f, 0.f, 0.f));
}

template <bool VEC, bool INV>
__global__ void __launch_bounds__(kDcThreads) k_dcorr_stats(const float* __restrict__ d, const float* __restrict__ p, long long n,
                                                           float offset, DcMom* __restrict__ rec) {
    DcAcc<INV> acc;
    const double c = (double)offset;
    dc_walk<VEC>(d, p, n, [&](long long, int cnt, float4 a, float4 b) {
        acc.add(a.x, b.x, c);
        if (cnt == 4) { acc.add(a.y, b.y, c); acc.add(a.z, b.z, c); acc.add(a.w, b.w, c); }
    });
    const DcMom m = dc_block_merge(acc.moments());
    if (threadIdx.x == 0) rec[blockIdx.x] = m;
}

// What the merged moments give: the value record and the gradient's coefficients on (d - d_mean) and (x - x_mean), x = p (A)
// or 1 / (p + c) (B)
struct DcCoef { double cd, cx, md, mx; double loss, ra, rb; bool use_b, flat; };

__device__ __forceinline__ double dc_clamp1(double r) { return fmin(fmax(r, -1.0), 1.0); }

__device__ DcCoef dc_finish(const DcMom& m, int mode, double weight) {
    DcCoef k{};
    const bool ok_d = m.dd > 0.0;
    const bool ok_a = ok_d && m.pp > 0.0, ok_b = mode != SYN3R_DCORR_A && ok_d && m.uu > 0.0;
    k.ra = ok_a ? dc_clamp1(-m.dp / sqrt(m.dd * m.pp)) : 0.0;     // t = -p: S_tt = S_pp, S_dt = -S_dp
    k.rb = ok_b ? dc_clamp1(m.du / sqrt(m.dd * m.uu)) : 0.0;
    const double la = 1.0 - k.ra, lb = 1.0 - k.rb;
    k.use_b = mode == SYN3R_DCORR_B || (mode == SYN3R_DCORR_MIN && lb < la);     // a tie takes A
    const double r = k.use_b ? k.rb : k.ra;
    k.loss = weight * (k.use_b ? lb : la);
    k.flat = !(k.use_b ? ok_b : ok_a);
    if (!k.flat) {
        const double s = sqrt(m.dd * (k.use_b ? m.uu : m.pp));
        // -w [ (t - t_mean) / s - r (d - d_mean) / S_dd ]:  A: t - t_mean = -(p - p_mean);  B: t = u
        k.cx = (k.use_b ? -weight : weight) / s;
        k.cd = weight * r / m.dd;
    }
    k.md = m.md;
    k.mx = k.use_b ? m.mu : m.mp;
    return k;
}

// the block records merged in the same order by every caller: thread t takes records t, t + 256, ... then the block tree
__device__ __forceinline__ DcCoef dc_combine(const DcMom* __restrict__ rec, int nrec, int mode, double weight) {
    DcMom m{};
    for (int i = threadIdx.x; i < nrec; i += kDcThreads) m = dc_merge(m, rec[i]);
    return dc_finish(dc_block_merge(m), mode, weight);
}

// parts[0] = weight * L, parts[1] = r_A, parts[2] = r_B (0 unless mode uses B), parts[3] = chosen branch (0 = A, 1 = B)
__device__ __forceinline__ void dc_write_parts(const DcCoef& k, float* __restrict__ parts) {
    *(float4*)parts = make_float4((float)k.loss, (float)k.ra, (float)k.rb, k.use_b ? 1.0f : 0.0f);
}

__global__ void __launch_bounds__(kDcThreads) k_dcorr_final(const DcMom* __restrict__ rec, int nrec, int mode, float weight,
                                                           float* __restrict__ parts) {
    const DcCoef k = dc_combine(rec, nrec, mode, (double)weight);
    if (threadIdx.x == 0) dc_write_parts(k, parts);
}

// dL/dd_i = g * (cx (x_i - x_mean) + cd (d_i - d_mean)) in fp64, one fp32 rounding; parts (optional): written by block 0
template <bool VEC>
__global__ void __launch_bounds__(kDcThreads) k_dcorr_grad(const float* __restrict__ d, const float* __restrict__ p, long long n,
                                                          float offset, const DcMom* __restrict__ rec, int nrec, int mode,
                                                          float weight, const float* __restrict__ go, float* __restrict__ grad,
                                                          float* __restrict__ parts) {
    const DcCoef k = dc_combine(rec, nrec, mode, (double)weight);
    if (parts && blockIdx.x == 0 && threadIdx.x == 0) dc_write_parts(k, parts);
    const double g = go ? (double)*go : 1.0;
    const double cx = g * k.cx, cd = g * k.cd, c = (double)offset;
    const bool use_b = k.use_b, flat = k.flat;
    auto one = [&](float df, float pf) -> float {
        if (flat) return 0.0f;
        const double x = use_b ? 1.0 / ((double)pf + c) : (double)pf;
        return (float)(cx * (x - k.mx) + cd * ((double)df - k.md));
    };
    dc_walk<VEC>(d, p, n, [&](long long e, int cnt, float4 a, float4 b) {
        if (cnt == 4) *(float4*)(grad + e) = make_float4(one(a.x, b.x), one(a.y, b.y), one(a.z, b.z), one(a.w, b.w));
        else grad[e] = one(a.x, b.x);
    });
}

int dc_blocks(long long n) {
    long long b = (n + kDcThreads * 16 - 1) / (kDcThreads * 16);      // ~16 elements per thread
    if (b < 1) b = 1;
    if (b > kDcMaxBlocks) b = kDcMaxBlocks;
    return (int)b;
}

bool dc_aligned(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

// argument checks shared by the three entries (ws: the records of the statistics pass)
int dc_check(const char* who, const float* depth, const float* prior, long long n, float weight, float offset, int mode,
             const void* ws, size_t ws_bytes) {
    SYN3R_REQUIRE(n >= 2 && n <= kDcMaxN, "%s: n=%lld must be in [2, 2^30]", who, n);
    SYN3R_REQUIRE(depth && prior && ws, "%s: null pointer", who);
    SYN3R_REQUIRE(mode == SYN3R_DCORR_MIN || mode == SYN3R_DCORR_A || mode == SYN3R_DCORR_B, "%s: mode=%d is not MIN / A / B", who, mode);
    SYN3R_REQUIRE(weight == weight && fabsf(weight) <= 3.0e38f, "%s: weight must be finite", who);
    SYN3R_REQUIRE(mode == SYN3R_DCORR_A || (offset == offset && fabsf(offset) <= 3.0e38f), "%s: offset must be finite", who);
    SYN3R_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: workspace must be 16-byte aligned", who);
    if (ws_bytes < syn3r_depth_corr_loss_workspace_bytes(n)) {
        set_error("%s: workspace %zu < %zu bytes (syn3r_depth_corr_loss_workspace_bytes)", who, ws_bytes,
                  syn3r_depth_corr_loss_workspace_bytes(n));
        return SYN3R_E_WORKSPACE;
    }
    return SYN3R_OK;
}

void dc_stats(const float* depth, const float* prior, long long n, float offset, int mode, void* ws, hipStream_t stream) {
    const dim3 grid((unsigned)dc_blocks(n));
    const bool vec = dc_aligned(depth, prior), inv = mode != SYN3R_DCORR_A;
    DcMom* rec = (DcMom*)ws;
    auto kern = vec ? (inv ? k_dcorr_stats<true, true> : k_dcorr_stats<true, false>)
                    : (inv ? k_dcorr_stats<false, true> : k_dcorr_stats<false, false>);
    SYN3R_LAUNCH_NAMED("k_dcorr_stats", kern, grid, dim3(kDcThreads), 0, stream, depth, prior, n, offset, rec);
}

void dc_grad(const float* depth, const float* prior, long long n, float weight, float offset, int mode, const float* grad_loss,
             const void* ws, float* grad_depth, float* parts, hipStream_t stream) {
    const dim3 grid((unsigned)dc_blocks(n));
    const DcMom* rec = (const DcMom*)ws;
    const int nrec = dc_blocks(n);
    if (dc_aligned(depth, prior) && ((uintptr_t)grad_depth & 15) == 0)
        SYN3R_LAUNCH(k_dcorr_grad<true>, grid, dim3(kDcThreads), 0, stream, depth, prior, n, offset, rec, nrec, mode, weight, grad_loss,
                     grad_depth, parts);
    else
        SYN3R_LAUNCH(k_dcorr_grad<false>, grid, dim3(kDcThreads), 0, stream, depth, prior, n, offset, rec, nrec, mode, weight, grad_loss,
                     grad_depth, parts);
}

}  // namespace

extern "C" size_t syn3r_depth_corr_loss_workspace_bytes(long long n) {
    if (n < 2 || n > kDcMaxN) return 0;
    return (((size_t)dc_blocks(n) * sizeof(DcMom) + 255) / 256) * 256;
}

extern "C" int syn3r_depth_corr_loss(const float* depth, const float* prior, long long n, float weight, float offset, int mode,
                                     float* parts, void* ws, size_t ws_bytes, void* stream_) {
    const int rc = dc_check("depth_corr_loss", depth, prior, n, weight, offset, mode, ws, ws_bytes);
    if (rc) return rc;
    SYN3R_REQUIRE(parts, "depth_corr_loss: null pointer");
    SYN3R_REQUIRE(((uintptr_t)parts & 15) == 0, "depth_corr_loss: parts must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    dc_stats(depth, prior, n, offset, mode, ws, stream);
    SYN3R_LAUNCH(k_dcorr_final, dim3(1), dim3(kDcThreads), 0, stream, (const DcMom*)ws, dc_blocks(n), mode, weight, parts);
    SYN3R_LAUNCH_CHECK("depth_corr_loss launch");
    return SYN3R_OK;
}

extern "C" int syn3r_depth_corr_loss_backward(const float* depth, const float* prior, long long n, float weight, float offset, int mode,
                                              const float* grad_loss, const void* ws, size_t ws_bytes, float* grad_depth, void* stream_) {
    const int rc = dc_check("depth_corr_loss_backward", depth, prior, n, weight, offset, mode, ws, ws_bytes);
    if (rc) return rc;
    SYN3R_REQUIRE(grad_depth, "depth_corr_loss_backward: null pointer");
    dc_grad(depth, prior, n, weight, offset, mode, grad_loss, ws, grad_depth, nullptr, (hipStream_t)stream_);
    SYN3R_LAUNCH_CHECK("depth_corr_loss_backward launch");
    return SYN3R_OK;
}

extern "C" int syn3r_depth_corr_loss_step(const float* depth, const float* prior, long long n, float weight, float offset, int mode,
                                          const float* grad_loss, float* parts, float* grad_depth, void* ws, size_t ws_bytes,
                                          void* stream_) {
    const int rc = dc_check("depth_corr_loss_step", depth, prior, n, weight, offset, mode, ws, ws_bytes);
    if (rc) return rc;
    SYN3R_REQUIRE(parts && grad_depth, "depth_corr_loss_step: null pointer");
    SYN3R_REQUIRE(((uintptr_t)parts & 15) == 0, "depth_corr_loss_step: parts must be 16-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    dc_stats(depth, prior, n, offset, mode, ws, stream);
    dc_grad(depth, prior, n, weight, offset, mode, grad_loss, ws, grad_depth, parts, stream);
    SYN3R_LAUNCH_CHECK("depth_corr_loss_step launch");
    return SYN3R_OK;
}
