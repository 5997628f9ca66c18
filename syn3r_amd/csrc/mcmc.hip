// 3DGS-MCMC density control (EXTENSION, include/syn3r_hip.h; Kheradmand et al., NeurIPS 2024 - every constant recalled, UNPINNED):
//   syn3r_mcmc_noise      xyz_i += scale * gate(o_i) * Sigma_i eps_i            every training step, one launch
//   syn3r_mcmc_reg_step   the L1 regularisers on opacity and scale, their values and their gradients: two launches, no atomics
//   syn3r_mcmc_weights    integer sampling weights, 0 = dead
//   syn3r_mcmc_sample     for every dead row (and every appended row) a live source, drawn with probability ~ weight: integers only
//   syn3r_mcmc_relocate   the sources' new opacity / scale, the destinations as copies, Adam moments of touched rows zeroed
//
// Random numbers: Philox4x32-10 (Salmon et al., SC 2011; the standard multipliers and key increments), counter = (index, 0, stream
// tag, step), key = (low, high) half of the 64-bit seed.  No generator state: the draw of an index is a function of (seed, step, tag,
// index) alone, whatever n or the grid is.
//
// Precision.  The noise is eps in fp32 (Box-Muller on exact fp32 uniforms, logf / sqrtf / cospif / sinpif) and everything after it -
// the activations, R, Sigma eps, the gate, the product with `scale` and the add - in fp64, rounded to fp32 once: off-diagonal entries
// of Sigma = R diag(s^2) R^T cancel (a needle across an axis), and fp32 rotation arithmetic leaves an error there that is relative
// to the LARGEST scale, not to the entry.  The kernel is one trip of ~11 loads per thread and stays short of its bytes' time anyway
// (profiles/r16/mcmc.txt).  The relocation sums 51 alternating binomial terms (sum |term| / |sum| up to 8.9e3): fp64 as well.
// Built without fma contraction (build.py STRICT_FP).  No floating-point atomics; the integer atomics of the sampler count draws and
// do not depend on order.  Every result is the same bits from call to call.
#include "plane_pass.h"

using namespace syn3r;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;          // the cap of train.hip's grids (kMaxBlocks)
constexpr int kChunk = 4096;              // elements of one scan chunk: 32-bit sums inside (<= 2^12 * 2^16), 64-bit bases across
constexpr int kPerThread = kChunk / kThreads;
constexpr int kMaxChunks = SYN3R_DIM_MAX / kChunk;       // 4096
constexpr int kBaseThreads = 1024;
constexpr int kRatioMax = 51;             // the released code's binomial table: recalled, UNPINNED
constexpr unsigned kTagNoise = 0, kTagSample = 1;

struct U4 { unsigned x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}

int blocks_for(long long items) { return pass_blocks(items, kThreads, kMaxBlocks); }

size_t round256(size_t b) { return ((b + 255) / 256) * 256; }

// ------------------------------------------------------------------------------------------------------------------ noise
// u in (0, 1] and v in [0, 1) from the top 24 bits of a word: exact in fp32
__device__ __forceinline__ float u01_open0(unsigned x) { return (float)((x >> 8) + 1u) * 0x1p-24f; }
__device__ __forceinline__ float u01_open1(unsigned x) { return (float)(x >> 8) * 0x1p-24f; }

__global__ void __launch_bounds__(kThreads) k_mcmc_noise(float* __restrict__ xyz, const float* __restrict__ log_scales,
                                                        const float4* __restrict__ rotations, const float* __restrict__ logits, int n,
                                                        double scale, unsigned k0, unsigned k1, unsigned step) {
    for (long long base = (long long)blockIdx.x * kThreads; base < n; base += (long long)gridDim.x * kThreads) {
        const long long i = base + threadIdx.x;
        const long long j = i < n ? i : n - 1;        // a thread past the end loads the last Gaussian: all loads unconditional, together
        const float p0 = xyz[3 * j], p1 = xyz[3 * j + 1], p2 = xyz[3 * j + 2];
        const float l0 = log_scales[3 * j], l1 = log_scales[3 * j + 1], l2 = log_scales[3 * j + 2];
        const float4 q = rotations[j];
        const float lg = logits[j];
        // eps: three of the four Box-Muller normals of the index' four words
        const U4 w = philox4x32_10((unsigned)j, 0u, kTagNoise, step, k0, k1);
        const float r01 = sqrtf(-2.0f * logf(u01_open0(w.x))), r2 = sqrtf(-2.0f * logf(u01_open0(w.z)));
        const float a01 = 2.0f * u01_open1(w.y), a2 = 2.0f * u01_open1(w.w);
        const double e0 = (double)(r01 * cospif(a01)), e1 = (double)(r01 * sinpif(a01)), e2 = (double)(r2 * cospif(a2));
        // R of the normalised (w, x, y, z) quaternion (torch's normalize: / max(|q|, 1e-12))
        const double nq = sqrt((double)q.x * q.x + (double)q.y * q.y + (double)q.z * q.z + (double)q.w * q.w);
        const double inv = 1.0 / fmax(nq, 1e-12);
        const double r = q.x * inv, x = q.y * inv, y = q.z * inv, z = q.w * inv;
        const double R00 = 1.0 - 2.0 * (y * y + z * z), R01 = 2.0 * (x * y - r * z), R02 = 2.0 * (x * z + r * y);
        const double R10 = 2.0 * (x * y + r * z), R11 = 1.0 - 2.0 * (x * x + z * z), R12 = 2.0 * (y * z - r * x);
        const double R20 = 2.0 * (x * z - r * y), R21 = 2.0 * (y * z + r * x), R22 = 1.0 - 2.0 * (x * x + y * y);
        const double s0 = exp((double)l0), s1 = exp((double)l1), s2 = exp((double)l2);
        // Sigma eps = R (s^2 . (R^T eps))
        const double t0 = s0 * s0 * (R00 * e0 + R10 * e1 + R20 * e2);
        const double t1 = s1 * s1 * (R01 * e0 + R11 * e1 + R21 * e2);
        const double t2 = s2 * s2 * (R02 * e0 + R12 * e1 + R22 * e2);
        const double o = 1.0 / (1.0 + exp(-(double)lg));
        const double g = scale / (1.0 + exp(-100.0 * (0.005 - o)));       // k = 100, x0 = 0.995 on 1 - o: recalled, UNPINNED
        if (i < n) {
            xyz[3 * i] = (float)((double)p0 + g * (R00 * t0 + R01 * t1 + R02 * t2));
            xyz[3 * i + 1] = (float)((double)p1 + g * (R10 * t0 + R11 * t1 + R12 * t2));
            xyz[3 * i + 2] = (float)((double)p2 + g * (R20 * t0 + R21 * t1 + R22 * t2));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ regularisers
__global__ void __launch_bounds__(kThreads) k_mcmc_reg_pass(const float* __restrict__ logits, const float* __restrict__ log_scales, int n,
                                                           float go /*opacity_reg / n*/, float gs /*scale_reg / 3n*/,
                                                           float* __restrict__ grad_opacity, float* __restrict__ grad_log_scales,
                                                           float* __restrict__ rows) {
    float so = 0.0f, ss = 0.0f;
    for (long long base = (long long)blockIdx.x * kThreads; base < n; base += (long long)gridDim.x * kThreads) {
        const long long i = base + threadIdx.x;
        const long long j = i < n ? i : n - 1;
        const float lg = logits[j], l0 = log_scales[3 * j], l1 = log_scales[3 * j + 1], l2 = log_scales[3 * j + 2];
        const float d = grad_opacity[j], d0 = grad_log_scales[3 * j], d1 = grad_log_scales[3 * j + 1], d2 = grad_log_scales[3 * j + 2];
        if (i < n) {
            const float o = act_sigmoid(lg), e0 = act_exp(l0), e1 = act_exp(l1), e2 = act_exp(l2);
            grad_opacity[i] = d + go * (o * (1.0f - o));
            grad_log_scales[3 * i] = d0 + gs * e0;
            grad_log_scales[3 * i + 1] = d1 + gs * e1;
            grad_log_scales[3 * i + 2] = d2 + gs * e2;
            so += o;
            ss += (e0 + e1) + e2;
        }
    }
    // (not plane_pass.h's block_rows: thread k stores column k here, and on the shared staging the kernel compiled to other code)
    __shared__ float part[kThreads / 64][2];
    const float wo = wave_sum(so), ws = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = wo; part[threadIdx.x >> 6][1] = ws; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        rows[(size_t)blockIdx.x * 2 + k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
    }
}

// one block: the block rows in a fixed order in fp64 (thread t takes rows t, t + 1024, ...; the threads are added in ascending order
// of wave, then lane pairs by the butterfly of wave_sum_d - fixed for a given row count)
__global__ void __launch_bounds__(kBaseThreads) k_mcmc_reg_finish(int nrows, const float* __restrict__ rows, double wo /*opacity_reg / n*/,
                                                                 double ws /*scale_reg / 3n*/, float* __restrict__ loss_out) {
    __shared__ double part[kBaseThreads / 64][2];
    double a = 0.0, b = 0.0;
    for (int r = threadIdx.x; r < nrows; r += kBaseThreads) { a += (double)rows[2 * (size_t)r]; b += (double)rows[2 * (size_t)r + 1]; }
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = a; part[threadIdx.x >> 6][1] = b; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < kBaseThreads / 64; ++q) t += part[q][threadIdx.x];
        loss_out[threadIdx.x] = (float)(t * (threadIdx.x == 0 ? wo : ws));
    }
}

// ------------------------------------------------------------------------------------------------------------------ weights
__global__ void __launch_bounds__(kThreads) k_mcmc_weights(const float* __restrict__ logits, int n, float dead_logit,
                                                          unsigned* __restrict__ weights) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const float lg = logits[i];
        weights[i] = lg <= dead_logit ? 0u : (unsigned)rintf(act_sigmoid(lg) * 65536.0f);
    }
}

// ------------------------------------------------------------------------------------------------------------------ sampling
// one block per chunk of kChunk weights: the exclusive prefix sums INSIDE the chunk (32 bits), the chunk's sum, and counts = 0
__global__ void __launch_bounds__(kThreads) k_mcmc_scan_chunks(const unsigned* __restrict__ weights, int n, unsigned* __restrict__ excl,
                                                              unsigned* __restrict__ chunk_sum, unsigned* __restrict__ counts) {
    __shared__ unsigned smem[kThreads / 64 + 1];
    const long long first = (long long)blockIdx.x * kChunk + (long long)threadIdx.x * kPerThread;
    unsigned w[kPerThread], mine = 0u;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        w[k] = first + k < n ? weights[first + k] : 0u;
        mine += w[k];
    }
    unsigned total;
    unsigned run = block_exclusive_scan<kThreads / 64>(mine, smem, total);
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (first + k < n) { excl[first + k] = run; counts[first + k] = 0u; }
        run += w[k];
    }
    if (threadIdx.x == 0) chunk_sum[blockIdx.x] = total;
}

// one block: base[c] = sum of the chunk sums before c, base[nchunks] = the total (64 bits; nchunks <= kMaxChunks = 4 per thread)
__global__ void __launch_bounds__(kBaseThreads) k_mcmc_scan_bases(const unsigned* __restrict__ chunk_sum, int nchunks,
                                                                 unsigned long long* __restrict__ base) {
    __shared__ unsigned long long buf[2][kBaseThreads];
    constexpr int kPer = kMaxChunks / kBaseThreads;
    unsigned v[kPer];
    unsigned long long mine = 0ull;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int c = threadIdx.x * kPer + k;
        v[k] = c < nchunks ? chunk_sum[c] : 0u;
        mine += v[k];
    }
    int cur = 0;
    buf[0][threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < kBaseThreads; o <<= 1) {         // inclusive Hillis-Steele scan, double-buffered
        buf[cur ^ 1][threadIdx.x] = buf[cur][threadIdx.x] + (threadIdx.x >= o ? buf[cur][threadIdx.x - o] : 0ull);
        cur ^= 1;
        __syncthreads();
    }
    unsigned long long run = buf[cur][threadIdx.x] - mine;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int c = threadIdx.x * kPer + k;
        if (c < nchunks) base[c] = run;
        run += v[k];
    }
    if (threadIdx.x == kBaseThreads - 1) base[nchunks] = buf[cur][threadIdx.x];
}

__global__ void __launch_bounds__(kThreads) k_mcmc_draw(const unsigned* __restrict__ weights, const unsigned* __restrict__ excl,
                                                       const unsigned long long* __restrict__ base, int n, int nchunks, int m_extra,
                                                       unsigned k0, unsigned k1, unsigned step, int* __restrict__ src,
                                                       unsigned* __restrict__ counts) {
    const unsigned long long total = base[nchunks];
    const long long dests = (long long)n + m_extra;
    for (long long d = (long long)blockIdx.x * kThreads + threadIdx.x; d < dests; d += (long long)gridDim.x * kThreads) {
        int s = -1;
        if (total != 0ull && (d >= n || weights[d] == 0u)) {
            const U4 w = philox4x32_10((unsigned)d, 0u, kTagSample, step, k0, k1);
            const unsigned long long r = __umul64hi(((unsigned long long)w.x << 32) | w.y, total);       // in [0, total)
            int lo = 0, hi = nchunks - 1;                 // the LAST chunk whose base is <= r (a chunk of sum 0 shares its base with
            while (lo < hi) {                             // the next and is passed over)
                const int mid = (lo + hi + 1) >> 1;
                if (base[mid] <= r) lo = mid; else hi = mid - 1;
            }
            const unsigned r32 = (unsigned)(r - base[lo]);
            int a = lo * kChunk, b = a + kChunk - 1 < n - 1 ? a + kChunk - 1 : n - 1;
            while (a < b) {                               // the LAST element of the chunk whose prefix is <= r32 (zeros are passed over)
                const int mid = (int)(((long long)a + b + 1) >> 1);
                if (excl[mid] <= r32) a = mid; else b = mid - 1;
            }
            s = a;
            atomicAdd(&counts[s], 1u);
        }
        src[d] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------------ relocation
struct Moments { float* p[10]; };         // exp_avg, exp_avg_sq of xyz, features, opacity, log-scales, rotations; any may be null

struct NewValues { float logit, dls; };   // the new opacity logit, and what is added to every log-scale

// a source of opacity sigmoid(lg) that was drawn `count` times (ratio = min(count + 1, 51) Gaussians share its place):
//   o' = clamp(1 - (1 - o)^(1 / ratio), min_opacity, 1 - 2^-23)
//   scale' = scale * o / D,  D = sum_{j=1..ratio} sum_{k<j} C(j-1, k) (-1)^k o'^(k+1) / sqrt(k+1) = sum_{m=1..ratio} C(ratio, m) (-1)^(m-1) o'^m / sqrt(m)
// (the inner sum over j of C(j-1, m-1) is C(ratio, m)).  fp64: the terms cancel
__device__ __forceinline__ NewValues mcmc_new_values(float lg, unsigned count, double min_opacity) {
    const int ratio = count + 1u < (unsigned)kRatioMax ? (int)(count + 1u) : kRatioMax;
    const double o = 1.0 / (1.0 + exp(-(double)lg));
    double on = -expm1(log1p(-o) / (double)ratio);
    on = fmin(fmax(on, min_opacity), 1.0 - 0x1p-23);
    double D = 0.0, binom = 1.0, pw = 1.0;
    for (int m = 1; m <= ratio; ++m) {
        binom = binom * (double)(ratio - m + 1) / (double)m;
        pw *= on;
        const double term = binom * pw / sqrt((double)m);
        D += (m & 1) ? term : -term;
    }
    NewValues v;
    v.logit = (float)log(on / (1.0 - on));
    v.dls = (float)log(o / D);
    return v;
}

__device__ __forceinline__ void zero_row(float* m, long long row, int len) {
    if (m)
        for (int k = 0; k < len; ++k) m[row * len + k] = 0.0f;
}
__device__ __forceinline__ void zero_moments(const Moments& mo, long long row, int feature_row_len) {
    zero_row(mo.p[0], row, 3); zero_row(mo.p[1], row, 3);
    zero_row(mo.p[2], row, feature_row_len); zero_row(mo.p[3], row, feature_row_len);
    zero_row(mo.p[4], row, 1); zero_row(mo.p[5], row, 1);
    zero_row(mo.p[6], row, 3); zero_row(mo.p[7], row, 3);
    zero_row(mo.p[8], row, 4); zero_row(mo.p[9], row, 4);
}

// first launch: every destination d < n becomes a copy of its source with the source's NEW opacity and scale, computed from the
// source's OLD values (the sources are rewritten by the second launch, after this one)
__global__ void __launch_bounds__(kThreads) k_mcmc_relocate_dst(int n, const int* __restrict__ src, const unsigned* __restrict__ counts,
                                                               float* xyz, float* features, int feature_row_len, float* logits,
                                                               float* log_scales, float* rotations, Moments mo, double min_opacity) {
    for (long long d = (long long)blockIdx.x * kThreads + threadIdx.x; d < n; d += (long long)gridDim.x * kThreads) {
        const int s = src[d];
        if (s < 0 || s >= n || s == d) continue;
        const NewValues v = mcmc_new_values(logits[s], counts[s], min_opacity);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            xyz[3 * d + k] = xyz[3 * (long long)s + k];
            log_scales[3 * d + k] = log_scales[3 * (long long)s + k] + v.dls;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) rotations[4 * d + k] = rotations[4 * (long long)s + k];
        for (int k = 0; k < feature_row_len; ++k) features[d * feature_row_len + k] = features[(long long)s * feature_row_len + k];
        logits[d] = v.logit;
        zero_moments(mo, d, feature_row_len);
    }
}

// second launch: every source takes its own new values
__global__ void __launch_bounds__(kThreads) k_mcmc_relocate_src(int n, const unsigned* __restrict__ counts, float* logits,
                                                               float* log_scales, int feature_row_len, Moments mo, double min_opacity) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const unsigned c = counts[i];
        if (c == 0u) continue;
        const NewValues v = mcmc_new_values(logits[i], c, min_opacity);
#pragma unroll
        for (int k = 0; k < 3; ++k) log_scales[3 * i + k] = log_scales[3 * i + k] + v.dls;
        logits[i] = v.logit;
        zero_moments(mo, i, feature_row_len);
    }
}

}  // namespace

extern "C" int syn3r_mcmc_noise(float* xyz, const float* log_scales, const float* rotations, const float* opacity_logits, int n,
                                float scale, unsigned long long seed, int step, void* stream_) {
    SYN3R_REQUIRE(SYN3R_DIM_OK(n), "mcmc_noise: n=%d must be in [1, 2^24]", n);
    SYN3R_REQUIRE(xyz && log_scales && rotations && opacity_logits, "mcmc_noise: null pointer");
    SYN3R_REQUIRE((((uintptr_t)xyz | (uintptr_t)log_scales | (uintptr_t)opacity_logits) & 3) == 0 && ((uintptr_t)rotations & 15) == 0,
                  "mcmc_noise: pointers must be 4-byte aligned, rotations 16-byte aligned");
    SYN3R_REQUIRE(scale == scale, "mcmc_noise: scale is NaN");
    const size_t b3 = (size_t)n * 3 * sizeof(float);
    SYN3R_REQUIRE(!ranges_overlap(xyz, b3, log_scales, b3) && !ranges_overlap(xyz, b3, rotations, (size_t)n * 16) &&
                  !ranges_overlap(xyz, b3, opacity_logits, (size_t)n * 4), "mcmc_noise: xyz aliases an input");
    SYN3R_LAUNCH(k_mcmc_noise, dim3((unsigned)blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream_, xyz, log_scales,
                 (const float4*)rotations, opacity_logits, n, (double)scale, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32),
                 (unsigned)step);
    SYN3R_LAUNCH_CHECK("mcmc_noise launch");
    return SYN3R_OK;
}

extern "C" size_t syn3r_mcmc_reg_step_workspace_bytes(int n) {
    return SYN3R_DIM_OK(n) ? round256((size_t)blocks_for(n) * 2 * sizeof(float)) : 0;
}

extern "C" int syn3r_mcmc_reg_step(const float* opacity_logits, const float* log_scales, int n, float opacity_reg, float scale_reg,
                                   float* grad_opacity, float* grad_log_scales, float* loss_out, void* ws, size_t ws_bytes,
                                   void* stream_) {
    SYN3R_REQUIRE(SYN3R_DIM_OK(n), "mcmc_reg_step: n=%d must be in [1, 2^24]", n);
    SYN3R_REQUIRE(opacity_logits && log_scales && grad_opacity && grad_log_scales && loss_out && ws, "mcmc_reg_step: null pointer");
    SYN3R_REQUIRE((((uintptr_t)opacity_logits | (uintptr_t)log_scales | (uintptr_t)grad_opacity | (uintptr_t)grad_log_scales |
                    (uintptr_t)loss_out) & 3) == 0, "mcmc_reg_step: pointers must be 4-byte aligned");
    if (const int rc = check_workspace("mcmc_reg_step", ws, ws_bytes, syn3r_mcmc_reg_step_workspace_bytes(n),
                                       "syn3r_mcmc_reg_step_workspace_bytes")) return rc;
    const size_t b1 = (size_t)n * sizeof(float), b3 = 3 * b1;
    SYN3R_REQUIRE(!ranges_overlap(grad_opacity, b1, opacity_logits, b1) && !ranges_overlap(grad_opacity, b1, log_scales, b3) &&
                  !ranges_overlap(grad_log_scales, b3, opacity_logits, b1) && !ranges_overlap(grad_log_scales, b3, log_scales, b3) &&
                  !ranges_overlap(grad_opacity, b1, grad_log_scales, b3) && !ranges_overlap(loss_out, 8, grad_opacity, b1) &&
                  !ranges_overlap(loss_out, 8, grad_log_scales, b3), "mcmc_reg_step: an output aliases an input or another output");
    hipStream_t stream = (hipStream_t)stream_;
    const int nb = blocks_for(n);
    const double wo = (double)opacity_reg / (double)n, wsc = (double)scale_reg / (3.0 * (double)n);
    SYN3R_LAUNCH(k_mcmc_reg_pass, dim3((unsigned)nb), dim3(kThreads), 0, stream, opacity_logits, log_scales, n, (float)wo, (float)wsc,
                 grad_opacity, grad_log_scales, (float*)ws);
    SYN3R_LAUNCH(k_mcmc_reg_finish, dim3(1), dim3(kBaseThreads), 0, stream, nb, (const float*)ws, wo, wsc, loss_out);
    SYN3R_LAUNCH_CHECK("mcmc_reg_step launch");
    return SYN3R_OK;
}

extern "C" int syn3r_mcmc_weights(const float* opacity_logits, int n, float dead_logit, unsigned* weights, void* stream_) {
    SYN3R_REQUIRE(SYN3R_DIM_OK(n), "mcmc_weights: n=%d must be in [1, 2^24]", n);
    SYN3R_REQUIRE(opacity_logits && weights, "mcmc_weights: null pointer");
    SYN3R_REQUIRE((((uintptr_t)opacity_logits | (uintptr_t)weights) & 3) == 0, "mcmc_weights: pointers must be 4-byte aligned");
    SYN3R_REQUIRE(dead_logit == dead_logit, "mcmc_weights: dead_logit is NaN");
    SYN3R_REQUIRE(!ranges_overlap(weights, (size_t)n * 4, opacity_logits, (size_t)n * 4), "mcmc_weights: weights aliases the logits");
    SYN3R_LAUNCH(k_mcmc_weights, dim3((unsigned)blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream_, opacity_logits, n, dead_logit,
                 weights);
    SYN3R_LAUNCH_CHECK("mcmc_weights launch");
    return SYN3R_OK;
}

// ws: excl[n] (32 bits), chunk sums [nchunks] (32 bits), bases [nchunks + 1] (64 bits), each part rounded up to 256 bytes
extern "C" size_t syn3r_mcmc_sample_workspace_bytes(int n) {
    if (!SYN3R_DIM_OK(n)) return 0;
    const size_t nchunks = ((size_t)n + kChunk - 1) / kChunk;
    return round256((size_t)n * 4) + round256(nchunks * 4) + round256((nchunks + 1) * 8);
}

extern "C" int syn3r_mcmc_sample(const unsigned* weights, int n, int m_extra, unsigned long long seed, int step, int* src,
                                 unsigned* counts, void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(SYN3R_DIM_OK(n), "mcmc_sample: n=%d must be in [1, 2^24]", n);
    SYN3R_REQUIRE(m_extra >= 0 && m_extra <= SYN3R_DIM_MAX, "mcmc_sample: m_extra=%d must be in [0, 2^24]", m_extra);
    SYN3R_REQUIRE(weights && src && counts && ws, "mcmc_sample: null pointer");
    SYN3R_REQUIRE((((uintptr_t)weights | (uintptr_t)src | (uintptr_t)counts) & 3) == 0, "mcmc_sample: pointers must be 4-byte aligned");
    if (const int rc = check_workspace("mcmc_sample", ws, ws_bytes, syn3r_mcmc_sample_workspace_bytes(n),
                                       "syn3r_mcmc_sample_workspace_bytes")) return rc;
    const size_t bn = (size_t)n * 4, bs = ((size_t)n + (size_t)m_extra) * 4;
    SYN3R_REQUIRE(!ranges_overlap(src, bs, weights, bn) && !ranges_overlap(counts, bn, weights, bn) && !ranges_overlap(src, bs, counts, bn),
                  "mcmc_sample: src / counts alias each other or the weights");
    hipStream_t stream = (hipStream_t)stream_;
    const int nchunks = (n + kChunk - 1) / kChunk;
    unsigned* excl = (unsigned*)ws;
    unsigned* chunk_sum = (unsigned*)((char*)ws + round256(bn));
    unsigned long long* base = (unsigned long long*)((char*)chunk_sum + round256((size_t)nchunks * 4));
    SYN3R_LAUNCH(k_mcmc_scan_chunks, dim3((unsigned)nchunks), dim3(kThreads), 0, stream, weights, n, excl, chunk_sum, counts);
    SYN3R_LAUNCH(k_mcmc_scan_bases, dim3(1), dim3(kBaseThreads), 0, stream, (const unsigned*)chunk_sum, nchunks, base);
    SYN3R_LAUNCH(k_mcmc_draw, dim3((unsigned)blocks_for((long long)n + m_extra)), dim3(kThreads), 0, stream, weights,
                 (const unsigned*)excl, (const unsigned long long*)base, n, nchunks, m_extra, (unsigned)(seed & 0xffffffffull),
                 (unsigned)(seed >> 32), (unsigned)step, src, counts);
    SYN3R_LAUNCH_CHECK("mcmc_sample launch");
    return SYN3R_OK;
}

extern "C" int syn3r_mcmc_relocate(int n, const int* src, const unsigned* counts, float* xyz, float* features, int feature_row_len,
                                   float* opacity_logits, float* log_scales, float* rotations, void* const* moments, float min_opacity,
                                   void* stream_) {
    SYN3R_REQUIRE(SYN3R_DIM_OK(n), "mcmc_relocate: n=%d must be in [1, 2^24]", n);
    SYN3R_REQUIRE(feature_row_len >= 1 && feature_row_len <= 4096, "mcmc_relocate: feature_row_len=%d must be in [1, 4096]", feature_row_len);
    SYN3R_REQUIRE(src && counts && xyz && features && opacity_logits && log_scales && rotations && moments, "mcmc_relocate: null pointer");
    SYN3R_REQUIRE(min_opacity > 0.0f && min_opacity < 1.0f, "mcmc_relocate: min_opacity=%g must be in (0, 1)", (double)min_opacity);
    uintptr_t bits = (uintptr_t)src | (uintptr_t)counts | (uintptr_t)xyz | (uintptr_t)features | (uintptr_t)opacity_logits |
                     (uintptr_t)log_scales | (uintptr_t)rotations;
    Moments mo;
    for (int k = 0; k < 10; ++k) { mo.p[k] = (float*)moments[k]; bits |= (uintptr_t)moments[k]; }
    SYN3R_REQUIRE((bits & 3) == 0, "mcmc_relocate: pointers must be 4-byte aligned");
    const size_t b1 = (size_t)n * 4;
    const void* arr[7] = {src, counts, xyz, features, opacity_logits, log_scales, rotations};
    const size_t len[7] = {b1, b1, 3 * b1, (size_t)feature_row_len * b1, b1, 3 * b1, 4 * b1};
    for (int a = 0; a < 7; ++a)
        for (int b = a + 1; b < 7; ++b)
            SYN3R_REQUIRE(!ranges_overlap(arr[a], len[a], arr[b], len[b]), "mcmc_relocate: two arrays alias each other");
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)blocks_for(n));
    SYN3R_LAUNCH(k_mcmc_relocate_dst, grid, dim3(kThreads), 0, stream, n, src, counts, xyz, features, feature_row_len, opacity_logits,
                 log_scales, rotations, mo, (double)min_opacity);
    SYN3R_LAUNCH(k_mcmc_relocate_src, grid, dim3(kThreads), 0, stream, n, counts, opacity_logits, log_scales, feature_row_len, mo,
                 (double)min_opacity);
    SYN3R_LAUNCH_CHECK("mcmc_relocate launch");
    return SYN3R_OK;
}
