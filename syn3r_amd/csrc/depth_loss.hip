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
#include "plane_pass.h"

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

int dc_blocks(long long n) { return pass_blocks(n, kDcThreads * 16, kDcMaxBlocks); }      // ~16 elements per thread

// argument checks shared by the three entries (ws: the records of the statistics pass)
int dc_check(const char* who, const float* depth, const float* prior, long long n, float weight, float offset, int mode,
             const void* ws, size_t ws_bytes) {
    SYN3R_REQUIRE(n >= 2 && n <= kDcMaxN, "%s: n=%lld must be in [2, 2^30]", who, n);
    SYN3R_REQUIRE(depth && prior && ws, "%s: null pointer", who);
    SYN3R_REQUIRE(mode == SYN3R_DCORR_MIN || mode == SYN3R_DCORR_A || mode == SYN3R_DCORR_B, "%s: mode=%d is not MIN / A / B", who, mode);
    SYN3R_REQUIRE(finite_f32(weight), "%s: weight must be finite", who);
    SYN3R_REQUIRE(mode == SYN3R_DCORR_A || finite_f32(offset), "%s: offset must be finite", who);
    return check_workspace(who, ws, ws_bytes, syn3r_depth_corr_loss_workspace_bytes(n), "syn3r_depth_corr_loss_workspace_bytes");
}

void dc_stats(const float* depth, const float* prior, long long n, float offset, int mode, void* ws, hipStream_t stream) {
    const dim3 grid((unsigned)dc_blocks(n));
    DcMom* rec = (DcMom*)ws;
    with_bools([&](auto vec, auto inv) {
        SYN3R_LAUNCH_NAMED("k_dcorr_stats", (k_dcorr_stats<decltype(vec)::value, decltype(inv)::value>), grid, dim3(kDcThreads), 0, stream,
                           depth, prior, n, offset, rec);
    }, aligned16(depth, prior), mode != SYN3R_DCORR_A);
}

void dc_grad(const float* depth, const float* prior, long long n, float weight, float offset, int mode, const float* grad_loss,
             const void* ws, float* grad_depth, float* parts, hipStream_t stream) {
    const dim3 grid((unsigned)dc_blocks(n));
    const DcMom* rec = (const DcMom*)ws;
    const int nrec = dc_blocks(n);
    with_bools([&](auto vec) {      // (the trace names these two launches apart)
        SYN3R_LAUNCH_NAMED(decltype(vec)::value ? "k_dcorr_grad<true>" : "k_dcorr_grad<false>", k_dcorr_grad<decltype(vec)::value>, grid,
                           dim3(kDcThreads), 0, stream, depth, prior, n, offset, rec, nrec, mode, weight, grad_loss, grad_depth, parts);
    }, aligned16(depth, prior, grad_depth));
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
    if (const int rp = check_parts("depth_corr_loss", parts)) return rp;
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
    SYN3R_REQUIRE(grad_depth, "depth_corr_loss_step: null pointer");
    if (const int rp = check_parts("depth_corr_loss_step", parts)) return rp;
    hipStream_t stream = (hipStream_t)stream_;
    dc_stats(depth, prior, n, offset, mode, ws, stream);
    dc_grad(depth, prior, n, weight, offset, mode, grad_loss, ws, grad_depth, parts, stream);
    SYN3R_LAUNCH_CHECK("depth_corr_loss_step launch");
    return SYN3R_OK;
}


// ================================================================================================ the patch-wise term
// The same term per P x P patch (SparseGS' patch-based Pearson, DNGaussian's local depth normalisation: a monocular prior is
// consistent only locally).  Origin (oy, ox), 0 <= oy, ox < P; patch (i, j) covers rows oy + iP .. oy + (i+1)P - 1 and columns
// ox + jP .. ox + (j+1)P - 1; only the K = floor((H - oy) / P) * floor((W - ox) / P) patches that lie inside the image count.
//   L = weight / K * sum_k L_k,   L_k = min(1 - r_A, 1 - r_B) of patch k (the branch chosen PER PATCH, the flat rule per patch)
//   dL/dd_i = weight * g / K * (the formula above with patch k's sums and means) for i in patch k, 0 in no full patch
// Flat patches stay in K: K depends on the geometry alone, so no device reduction stands between the statistics and the gradient.
//
// Mapping of the statistics pass.  A STRIP is 64 lanes wide: floor(64 / P) patches side by side for P <= 64 (lane = column, the
// last lanes idle when P does not divide 64), one patch for P > 64 (a lane then takes columns lane, lane + 64, ...).  A wave always
// reads 64 contiguous columns of one row (4-byte loads: a patch row starts at any column).  P <= 16: one wave per strip, four
// strips per block, so a small patch costs P / 64 of a wave.  P > 16: one block per strip - four waves for P <= 64, sixteen above
// (a 256 x 256 patch is 1024 row chunks, and only enough loads in flight hide their latency) - whose waves take the strip's
// (row, 64-column chunk) pairs round-robin; their per-lane moments meet through LDS and wave 0 merges them in wave order.  The
// lanes of
// one patch are then merged by a segmented shuffle tree (lane l takes lane l + o while that lane is in the same patch, o = 1, 2,
// 4 ...: lane 0 of the segment ends with the patch in column order), and that lane writes the patch's finished record.  Every
// order is fixed.  Each block also leaves the sum of its patches' (L_k, r, branch, flat) so that nobody has to walk K records.
// The gradient pass is a plain 256-column x kDlRows-row tile of the image per block: a thread keeps its column, hence its patch
// column, and fetches the 64-byte record (one line, shared by the P lanes beside it) when the patch row changes.

namespace {

constexpr int kDlPMin = 2, kDlPMax = 256;
constexpr int kDlWaveP = 16;                             // P <= kDlWaveP: one wave per strip; above: one block per strip,
constexpr int kDlWideP = 64;                             // of 4 waves up to kDlWideP and of 16 above
constexpr int dl_threads(int wps) { return wps == 16 ? 1024 : kDcThreads; }
constexpr int kDlRows = 4;                               // image rows per block of the gradient pass

struct DlRec { double md, mx, cd, cx, lk, r, use_b, flat; };      // cd, cx for weight 1: 64 bytes, one per patch
struct DlSum { double l, r, b, f; };                              // sums over the patches of one statistics block
static_assert(sizeof(DlRec) == 64 && sizeof(DlSum) == 32, "record layout");

struct DlGeom {
    int PY, PX;              // full patches down and across
    int npw, spr, wps;       // patches per strip, strips per patch row, waves per strip
    int strips, blocks;      // of the statistics pass
    long long K;
};

// false for arguments the entries reject (sizes alone)
bool dl_geom(int H, int W, int P, int oy, int ox, DlGeom* g) {
    if (!SYN3R_SIDE_OK(H) || !SYN3R_SIDE_OK(W) || P < kDlPMin || P > kDlPMax || oy < 0 || oy >= P || ox < 0 || ox >= P) return false;
    g->PY = (H - oy) / P;
    g->PX = (W - ox) / P;
    g->K = (long long)g->PY * g->PX;
    if (g->K < 1) return false;
    g->npw = P <= 64 ? 64 / P : 1;
    g->spr = (g->PX + g->npw - 1) / g->npw;
    g->wps = P <= kDlWaveP ? 1 : (P <= kDlWideP ? 4 : 16);
    g->strips = g->PY * g->spr;                          // <= 2^14 * 2^9
    g->blocks = g->wps == 1 ? (g->strips + 3) / 4 : g->strips;
    return true;
}

size_t dl_rec_bytes(const DlGeom& g) { return (size_t)g.K * sizeof(DlRec); }

__device__ __forceinline__ DcMom dc_shfl_down(const DcMom& a, int o) {
    DcMom b;
    b.n = __shfl_down(a.n, o, 64); b.md = __shfl_down(a.md, o, 64); b.mp = __shfl_down(a.mp, o, 64); b.mu = __shfl_down(a.mu, o, 64);
    b.dd = __shfl_down(a.dd, o, 64); b.pp = __shfl_down(a.pp, o, 64); b.uu = __shfl_down(a.uu, o, 64);
    b.dp = __shfl_down(a.dp, o, 64); b.du = __shfl_down(a.du, o, 64);
    return b;
}

// the sum of s over the block's NW waves in a fixed order (plain additions commute: the xor tree needs no sides)
template <int NW>
__device__ DlSum dl_block_sum(DlSum s) {
    __shared__ DlSum ws[NW];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        s.l += __shfl_xor(s.l, o, 64); s.r += __shfl_xor(s.r, o, 64); s.b += __shfl_xor(s.b, o, 64); s.f += __shfl_xor(s.f, o, 64);
    }
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    DlSum t = ws[0];
#pragma unroll 1
    for (int w = 1; w < NW; ++w) { t.l += ws[w].l; t.r += ws[w].r; t.b += ws[w].b; t.f += ws[w].f; }
    __syncthreads();
    return t;
}

template <int WPS, bool INV>
__global__ void __launch_bounds__(dl_threads(WPS)) k_dlocal_stats(const float* __restrict__ d, const float* __restrict__ p, int W, int P,
                                                            int oy, int ox, int PX, int npw, int spr, int strips, int mode,
                                                            float offset, DlRec* __restrict__ rec, DlSum* __restrict__ part) {
    static_assert(WPS == 1 || WPS == 4 || WPS == 16, "k_dlocal_stats: waves per strip");
    constexpr int U = WPS == 1 ? 4 : 8;                              // (row, chunk) pairs in flight per wave
    __shared__ DcMom xm[WPS == 1 ? 1 : (WPS - 1) * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int strip = WPS == 1 ? (int)blockIdx.x * 4 + wave : (int)blockIdx.x, sub = WPS == 1 ? 0 : wave;
    const bool live = strip < strips;                                // (wave-uniform)
    const int i = live ? strip / spr : 0, j0 = live ? (strip - i * spr) * npw : 0;
    const int seg = P < 64 ? P : 64;                                 // lanes of one patch
    // columns of the strip that belong to a full patch, and the 64-column chunks of one of its rows
    const int cols = !live ? 0 : (P > 64 ? P : (PX - j0 < npw ? PX - j0 : npw) * P);
    const int nch = (cols + 63) >> 6;
    const int E = P * nch;                                           // (row, chunk) pairs of the strip
    const size_t base = (size_t)(oy + i * P) * (size_t)W + (size_t)(ox + j0 * P);
    const double c = (double)offset;
    DcAcc<INV> acc;
    for (int e0 = sub; e0 < E; e0 += U * WPS) {
        float a[U], b[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int e = e0 + u * WPS, r = e / nch, cc = ((e - r * nch) << 6) + lane;
            ok[u] = e < E && cc < cols;
            a[u] = 0.f; b[u] = 0.f;
            if (ok[u]) {
                const size_t at = base + (size_t)r * (size_t)W + (size_t)cc;
                a[u] = d[at]; b[u] = p[at];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (ok[u]) acc.add(a[u], b[u], c);
    }
    DcMom m = acc.moments();
    if (WPS > 1) {                                                   // the waves of the strip, lane by lane
        if (wave) xm[(wave - 1) * 64 + lane] = m;
        __syncthreads();
        if (wave == 0) {
#pragma unroll 1
            for (int w = 1; w < WPS; ++w) m = dc_merge(m, xm[(w - 1) * 64 + lane]);
        }
    }
    DlSum s{0.0, 0.0, 0.0, 0.0};
    if (sub == 0) {                                                  // (wave-uniform)
        const int ls = lane % seg;
        for (int o = 1; o < seg; o <<= 1) {
            const DcMom t = dc_shfl_down(m, o);
            if (ls + o < seg) m = dc_merge(m, t);
        }
        if (ls == 0 && lane < cols) {                                // P > 64: lane 0 alone
            const DcCoef k = dc_finish(m, mode, 1.0);
            DlRec o;
            o.md = k.md; o.mx = k.mx; o.cd = k.cd; o.cx = k.cx;
            o.lk = k.loss; o.r = k.use_b ? k.rb : k.ra; o.use_b = k.use_b ? 1.0 : 0.0; o.flat = k.flat ? 1.0 : 0.0;
            rec[(size_t)i * PX + j0 + lane / seg] = o;
            s.l = o.lk; s.r = o.r; s.b = o.use_b; s.f = o.flat;
        }
    }
    s = dl_block_sum<dl_threads(WPS) / 64>(s);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// parts = [L, mean chosen r, share of patches on branch B, share of flat patches] from the block sums, by one whole block:
// thread t adds sums t, t + 256, ... in that order, then the block tree
__device__ void dl_write_parts(const DlSum* __restrict__ part, int nparts, long long K, float weight, float* __restrict__ parts) {
    DlSum s{0.0, 0.0, 0.0, 0.0};
    for (int q = threadIdx.x; q < nparts; q += kDcThreads) {
        const DlSum t = part[q];
        s.l += t.l; s.r += t.r; s.b += t.b; s.f += t.f;
    }
    s = dl_block_sum<kDcThreads / 64>(s);
    const double k = (double)K;
    if (threadIdx.x == 0)
        *(float4*)parts = make_float4((float)((double)weight * s.l / k), (float)(s.r / k), (float)(s.b / k), (float)(s.f / k));
}

__global__ void __launch_bounds__(kDcThreads) k_dlocal_final(const DlSum* __restrict__ part, int nparts, long long K, float weight,
                                                            float* __restrict__ parts) {
    dl_write_parts(part, nparts, K, weight, parts);
}

// ACC 0: every pixel of grad is written (0 outside the full patches); ACC 1: the pixels inside them are added to
template <bool ACC>
__global__ void __launch_bounds__(kDcThreads) k_dlocal_grad(const float* __restrict__ d, const float* __restrict__ p, int H, int W, int P,
                                                           int oy, int ox, int PY, int PX, float offset,
                                                           const DlRec* __restrict__ rec, const DlSum* __restrict__ part, int nparts,
                                                           long long K, float weight, const float* __restrict__ go,
                                                           float* __restrict__ grad, float* __restrict__ parts) {
    if (parts && blockIdx.x == 0 && blockIdx.y == 0) dl_write_parts(part, nparts, K, weight, parts);     // (block-uniform)
    const int x = (int)blockIdx.x * kDcThreads + (int)threadIdx.x;
    if (x >= W) return;
    const int y0 = (int)blockIdx.y * kDlRows;
    const int jx = x >= ox ? (x - ox) / P : PX;
    const bool in_x = jx < PX;
    const double wg = (double)weight * (go ? (double)*go : 1.0) / (double)K, c = (double)offset;
    float a[kDlRows], b[kDlRows];
    int iy[kDlRows];
#pragma unroll
    for (int u = 0; u < kDlRows; ++u) {
        const int y = y0 + u;
        iy[u] = (in_x && y >= oy && y < H) ? (y - oy) / P : PY;
        if (iy[u] >= PY) iy[u] = -1;                                 // -1: in no full patch
        a[u] = 0.f; b[u] = 0.f;
        if (iy[u] >= 0) {
            const size_t at = (size_t)y * (size_t)W + (size_t)x;
            a[u] = d[at]; b[u] = p[at];
        }
    }
    DlRec k{};
    int have = -1;
#pragma unroll
    for (int u = 0; u < kDlRows; ++u) {
        const int y = y0 + u;
        if (y >= H) break;
        const size_t at = (size_t)y * (size_t)W + (size_t)x;
        if (iy[u] < 0) {
            if (!ACC) grad[at] = 0.0f;
            continue;
        }
        if (iy[u] != have) { k = rec[(size_t)iy[u] * PX + jx]; have = iy[u]; }
        float v = 0.0f;
        if (k.flat == 0.0) {
            const double t = k.use_b != 0.0 ? 1.0 / ((double)b[u] + c) : (double)b[u];
            v = (float)(wg * (k.cx * (t - k.mx) + k.cd * ((double)a[u] - k.md)));
        }
        if (ACC) { if (k.flat == 0.0) grad[at] += v; }
        else grad[at] = v;
    }
}

// argument checks shared by the three entries, all before any HIP call
int dl_check(const char* who, const float* depth, const float* prior, int H, int W, int P, int oy, int ox, float weight, float offset,
             int mode, const void* ws, size_t ws_bytes, DlGeom* g) {
    SYN3R_REQUIRE(SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W), "%s: H=%d, W=%d must be in [1, %d]", who, H, W, SYN3R_SIDE_MAX);
    SYN3R_REQUIRE(P >= kDlPMin && P <= kDlPMax, "%s: patch P=%d must be in [%d, %d]", who, P, kDlPMin, kDlPMax);
    SYN3R_REQUIRE(oy >= 0 && oy < P && ox >= 0 && ox < P, "%s: origin (%d, %d) must be in [0, P=%d)", who, oy, ox, P);
    SYN3R_REQUIRE(dl_geom(H, W, P, oy, ox, g), "%s: K=0: no full %dx%d patch in %dx%d from origin (%d, %d)", who, P, P, H, W, oy, ox);
    SYN3R_REQUIRE(depth && prior && ws, "%s: null pointer", who);
    SYN3R_REQUIRE(mode == SYN3R_DCORR_MIN || mode == SYN3R_DCORR_A || mode == SYN3R_DCORR_B, "%s: mode=%d is not MIN / A / B", who, mode);
    SYN3R_REQUIRE(finite_f32(weight), "%s: weight must be finite", who);
    SYN3R_REQUIRE(mode == SYN3R_DCORR_A || finite_f32(offset), "%s: offset must be finite", who);
    return check_workspace(who, ws, ws_bytes, syn3r_depth_corr_local_workspace_bytes(H, W, P, oy, ox),
                           "syn3r_depth_corr_local_workspace_bytes");
}

void dl_stats(const float* depth, const float* prior, int W, int P, int oy, int ox, const DlGeom& g, float offset, int mode, void* ws,
              hipStream_t stream) {
    DlRec* rec = (DlRec*)ws;
    DlSum* part = (DlSum*)((char*)ws + dl_rec_bytes(g));
    const bool inv = mode != SYN3R_DCORR_A;
    auto kern = g.wps == 16 ? (inv ? k_dlocal_stats<16, true> : k_dlocal_stats<16, false>)
              : g.wps == 4  ? (inv ? k_dlocal_stats<4, true> : k_dlocal_stats<4, false>)
                            : (inv ? k_dlocal_stats<1, true> : k_dlocal_stats<1, false>);
    SYN3R_LAUNCH_NAMED("k_dlocal_stats", kern, dim3((unsigned)g.blocks), dim3((unsigned)dl_threads(g.wps)), 0, stream, depth, prior, W, P, oy, ox, g.PX,
                       g.npw, g.spr, g.strips, mode, offset, rec, part);
}

void dl_grad(const float* depth, const float* prior, int H, int W, int P, int oy, int ox, const DlGeom& g, float weight, float offset,
             const float* grad_loss, const void* ws, float* grad_depth, int accumulate, float* parts, hipStream_t stream) {
    const DlRec* rec = (const DlRec*)ws;
    const DlSum* part = (const DlSum*)((const char*)ws + dl_rec_bytes(g));
    const dim3 grid((unsigned)((W + kDcThreads - 1) / kDcThreads), (unsigned)((H + kDlRows - 1) / kDlRows));
    auto kern = accumulate ? k_dlocal_grad<true> : k_dlocal_grad<false>;
    SYN3R_LAUNCH_NAMED("k_dlocal_grad", kern, grid, dim3(kDcThreads), 0, stream, depth, prior, H, W, P, oy, ox, g.PY, g.PX, offset, rec,
                       part, g.blocks, g.K, weight, grad_loss, grad_depth, parts);
}

}  // namespace

extern "C" size_t syn3r_depth_corr_local_workspace_bytes(int H, int W, int P, int oy, int ox) {
    DlGeom g;
    if (!dl_geom(H, W, P, oy, ox, &g)) return 0;
    return ((dl_rec_bytes(g) + (size_t)g.blocks * sizeof(DlSum) + 255) / 256) * 256;
}

extern "C" int syn3r_depth_corr_local_loss(const float* depth, const float* prior, int H, int W, int P, int oy, int ox, float weight,
                                           float offset, int mode, float* parts, void* ws, size_t ws_bytes, void* stream_) {
    DlGeom g;
    const int rc = dl_check("depth_corr_local_loss", depth, prior, H, W, P, oy, ox, weight, offset, mode, ws, ws_bytes, &g);
    if (rc) return rc;
    if (const int rp = check_parts("depth_corr_local_loss", parts)) return rp;
    hipStream_t stream = (hipStream_t)stream_;
    dl_stats(depth, prior, W, P, oy, ox, g, offset, mode, ws, stream);
    SYN3R_LAUNCH(k_dlocal_final, dim3(1), dim3(kDcThreads), 0, stream, (const DlSum*)((const char*)ws + dl_rec_bytes(g)), g.blocks, g.K,
                 weight, parts);
    SYN3R_LAUNCH_CHECK("depth_corr_local_loss launch");
    return SYN3R_OK;
}

extern "C" int syn3r_depth_corr_local_loss_backward(const float* depth, const float* prior, int H, int W, int P, int oy, int ox,
                                                    float weight, float offset, int mode, const float* grad_loss, const void* ws,
                                                    size_t ws_bytes, float* grad_depth, int accumulate, void* stream_) {
    DlGeom g;
    const int rc = dl_check("depth_corr_local_loss_backward", depth, prior, H, W, P, oy, ox, weight, offset, mode, ws, ws_bytes, &g);
    if (rc) return rc;
    SYN3R_REQUIRE(grad_depth, "depth_corr_local_loss_backward: null pointer");
    SYN3R_REQUIRE(accumulate == 0 || accumulate == 1, "depth_corr_local_loss_backward: accumulate=%d must be 0 or 1", accumulate);
    dl_grad(depth, prior, H, W, P, oy, ox, g, weight, offset, grad_loss, ws, grad_depth, accumulate, nullptr, (hipStream_t)stream_);
    SYN3R_LAUNCH_CHECK("depth_corr_local_loss_backward launch");
    return SYN3R_OK;
}

extern "C" int syn3r_depth_corr_local_loss_step(const float* depth, const float* prior, int H, int W, int P, int oy, int ox, float weight,
                                                float offset, int mode, const float* grad_loss, float* parts, float* grad_depth,
                                                int accumulate, void* ws, size_t ws_bytes, void* stream_) {
    DlGeom g;
    const int rc = dl_check("depth_corr_local_loss_step", depth, prior, H, W, P, oy, ox, weight, offset, mode, ws, ws_bytes, &g);
    if (rc) return rc;
    SYN3R_REQUIRE(parts && grad_depth, "depth_corr_local_loss_step: null pointer");
    SYN3R_REQUIRE(accumulate == 0 || accumulate == 1, "depth_corr_local_loss_step: accumulate=%d must be 0 or 1", accumulate);
    if (const int rp = check_parts("depth_corr_local_loss_step", parts)) return rp;      // after `accumulate`, as ever
    hipStream_t stream = (hipStream_t)stream_;
    dl_stats(depth, prior, W, P, oy, ox, g, offset, mode, ws, stream);
    dl_grad(depth, prior, H, W, P, oy, ox, g, weight, offset, grad_loss, ws, grad_depth, accumulate, parts, stream);
    SYN3R_LAUNCH_CHECK("depth_corr_local_loss_step launch");
    return SYN3R_OK;
}
