// Gaussian rasteriser, backward: per-tile back-to-front traversal of the blend, then the
// per-Gaussian chain rule through EWA projection, SH colour and covariance construction.
//
// Replaces the rasteriser backward inside gsTrainer.training()/finetune() (call sites
// model/diffusionGS.py:139,1640); restates the published 3DGS backward (see raster_common.h;
// reference CUDA source absent).  Gradients are validated against autograd
// through oracle/raster_oracle.py.
//
// MI355X mapping: each wavefront owns a 16 x 8 pixel half of the tile, two pixels per lane on packed fp32
// arithmetic, and walks only the splats that can reach alpha >= 1/255 on that half (splat_reaches_rect,
// raster_common.h).  The kernel is bound by vector-instruction issue, so the visit body is written for its instruction count,
// not after the published per-channel form: ONE running scalar per pixel stands for the colours / depth of everything behind
// the current splat, the visit sums only RAW moments of G * dL/dalpha (the opacity, conic and pixel -> NDC factors, uniform
// per splat, are applied once per Gaussian in k_preprocess_bwd), and a loss without a depth gradient runs an instance without
// the depth terms (k_render_bwd's comment has the formulas; 125 -> 94 / 91 vector instructions per 128-pixel visit in round 7,
// 80 / 74 now).  Per visited splat the up to 128 pixel contributions to 10 quantities (9 without a depth gradient) are summed by
// reduce_lanes (two half/row swap levels + transposing DPP row rotates, 21 / 19 VALU instructions; the x moments are formed
// after the lane's two pixels, which share dx, are added), accumulated per (tile, splat) in LDS across the two wavefronts, and flushed with
// ONE atomic per record slot onto a contiguous 64-byte gradient record (MI355X float atomics want
// contiguous segments, MI355X_MICROARCH.md "Global float atomics").
#include "common.h"
#include "raster_common.h"

using namespace syn3r;

namespace {

// 64-byte per-Gaussian gradient record written by the blend backward
constexpr int kGradSlots = 16;
// slots 4-8 hold RAW moments of h = G * dL/dalpha over the splat's pixels (Sx = sum h dx, Sy, Sxx, Sxy, Syy with (dx, dy) = mean -
// pixel); k_preprocess_bwd turns them into the gradients of the pixel mean and the conic.  Slot 9 (sum h) is dL/d(opacity x confidence).
enum { G_R = 0, G_G, G_B, G_DEPTH, G_MX, G_MY, G_CXX, G_CXY, G_CYY, G_OP, G_USED = 10 };
// slots 10 and 11, written by the ABS instances of k_render_bwd alone (else they keep the memset's zero): the ABSOLUTE first moments
//     sum over the splat's pixels of |h| |cxx dx + cxy dy|   and of   |h| |cyy dy + cxy dx|
// (AbsGS, Ye et al. 2024, section 3.2: per pixel the mean's gradient is -opacity h conic (dx, dy); its components are summed by
// magnitude, so the pulls of the pixels on either side of a large Gaussian do not cancel).  The conic is inside the absolute value, so
// unlike G_MX / G_MY these are formed WITH it in the visit; the opacity and the pixel -> NDC factors still wait for k_abs_means2D.
enum { G_AMX = 10, G_AMY = 11, G_USED_ABS = 12 };

// Sum the per-lane gradient terms over the 64 lanes: NV = 10 values, or 9 without a depth gradient (value 9 is the depth term).
// Returns, on the lanes reduce_value names, a (partial) total of one value; every other lane holds a by-product.
// Two transposing levels use gfx950's half / row swaps (v_permlane32_swap, v_permlane16_swap): one VALU instruction moves BOTH
// directions of the exchange, so a level costs a swap and an add per PAIR of values and halves the number of live registers
// (10 -> 5 -> 3).  A value without a partner is not swapped at all: its register stays with both halves (rows), each of which
// sums its own lanes and hands in a partial total - the LDS atomic that follows adds the two.  That is value 4 at the first
// level when value 9 is dead (NV = 9) and a[2] at the second level, always.  Who owns what after the two levels (row q = lane >> 4):
//     b[0]: rows 0-3 own values 0, 3, 5, 8     b[1]: 1, 4, 6, 9 (NV = 9: 1, 4, 6, 4)     b[2]: 2, 2, 7, 7
// The last four levels stay inside a 16-lane row and transpose as well: v_add_f32 with a DPP row rotate (lane c reads lane
// c - n of its row) whose bank_mask keeps the banks of four lanes that a step must not write.
//     row_ror:8   b[0] + its rotation into lanes 0-7, b[1] + its rotation into lanes 8-15 of ONE register t; b[2] whole (period 8)
//     row_ror:4   t + its rotation is a complete sum over the lanes = c (mod 4) where lane c - 4 held the same value: banks 1 (b[0])
//                 and 3 (b[1]); b[2] + its rotation goes into the free banks 0 and 2
//     row_ror:2, row_ror:1 on t alone: lane 3 of a bank has read lanes 2, 1, 0 of the SAME bank only
// so lane 3 of a row ends with the row's sum of b[2], lane 7 of b[0], lane 15 of b[1] (lane 11: b[2] again, not used): 7
// instructions where three separate row sums and two selects took 14; 21 / 19 in all (rounds 6-7: 30, rounds 2-5: 38).
// The DPP steps are ONE inline-asm block with their wait states written in it: a VALU write of a register needs two wait states
// before a DPP read of it, and hipcc's hazard recogniser does not look into asm (the per-instruction asm of round 6 was safe only
// where the scheduler happened to interleave three chains).  __builtin_amdgcn_update_dpp cannot say these steps: it is a MOVE whose
// masked-off lanes take `old`, and hipcc folds move + add into v_add_f32_dpp only with the add's other operand in those lanes; a
// step that puts one value's sum into some banks and KEEPS another value in the rest is an add with a tied destination - through
// the builtin it would cost a select per merge (and round 6 saw the row_ror:1 step split even with full masks).  s_nop is not a
// vector instruction: the SIMD issues another wavefront's meanwhile.  No LDS-pipe ds_bpermute anywhere.
template <int NV>
__device__ __forceinline__ float reduce_lanes(float (&v)[10]) {
    static_assert(NV == 9 || NV == 10, "value 9 is the only optional one");
    float a[5];
#pragma unroll
    for (int k = 0; k < NV - 5; ++k) {   // lanes 32-63 of v[k] <-> lanes 0-31 of v[k+5]: the lower half owns k, the upper k + 5
        auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(v[k]), __float_as_int(v[k + 5]), false, false);
        a[k] = __int_as_float(r[0]) + __int_as_float(r[1]);
    }
    if (NV == 9) a[4] = v[4];            // both halves keep their own lanes' share of value 4
    float b[3];
#pragma unroll
    for (int k = 0; k < 2; ++k) {        // odd 16-lane rows of a[k] <-> even rows of a[k+3]: even rows own k, odd rows k + 3
        auto r = __builtin_amdgcn_permlane16_swap(__float_as_int(a[k]), __float_as_int(a[k + 3]), false, false);
        b[k] = __int_as_float(r[0]) + __int_as_float(r[1]);
    }
    b[2] = a[2];                         // both rows of a pair keep their own lanes' share
    asm("s_nop 1\n\t"                                                                    // b[] are fresh VALU results
        "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"             // lanes 0-7:  b0[c] + b0[c + 8]
        "v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"             // lanes 8-15: b1[c] + b1[c - 8]
        "v_add_f32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 0\n\t"                                                                    // (one instruction + one state since %0 was written)
        "v_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"             // banks 1, 3
        "v_add_f32_dpp %0, %2, %2 row_ror:4 row_mask:0xf bank_mask:0x5\n\t"             // banks 0, 2
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf"
        : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]));
    return b[0];
}
// the VALUE (index into reduce_lanes' argument) whose partial total this lane holds afterwards, or -1
template <int NV>
__device__ __forceinline__ int reduce_value(int lane) {
    const int c = lane & 15, q = lane >> 4;
    if (c == 7) return ((5 * q + 1) >> 1);                       // b[0]: 0, 3, 5, 8
    if (c == 15) return (NV == 9 && q == 3) ? 4 : ((5 * q + 1) >> 1) + 1;   // b[1]: 1, 4, 6, 9
    if (c == 3) return q < 2 ? 2 : 7;                            // b[2]
    return -1;
}

// ---------------------------------------------------------------------------------------------
// Blend backward, two pixels per lane.
//
// A 16 x 16 tile is a block of TWO wavefronts; wavefront w owns the 16 x 8 half (rows 8w .. 8w+7) and lane l the
// pixels (l & 15, 8w + (l >> 4)) and (l & 15, 8w + (l >> 4) + 4).  Every per-pixel quantity is a float2 and the
// arithmetic is written on float2 so that it compiles to gfx950's packed fp32 instructions (v_pk_fma_f32 /
// v_pk_mul_f32 / v_pk_add_f32: two pixels per VALU issue); only exp, rcp, min and the compares stay one per pixel.
// The kernel is VALU-bound (rocprofv3 round 1: 78 % VALU issue): against one pixel per lane this halves the issue
// slots of the chain-rule arithmetic and halves the number of cross-lane reductions per pixel (the two pixels of a
// lane are added before reduce_lanes).  The visit list is per wavefront, i.e. per 16 x 8 half: coarser than the former
// 8 x 8 quadrant (more visits pass the reach test), but a visit now carries 128 pixels for ~0.6 of the issue cost
// of two 64-pixel visits.  Splats are staged 128 at a time (one per thread).
constexpr int kBwdThreads = kBlendThreads;
#ifdef SYN3R_RASTER_STATS
__device__ unsigned long long g_bwd_stats[4];
#endif

// Per visit (splat i, T_i the transmittance in front of it, a_i its alpha, w_i = a_i T_i its blend weight, g the pixel's
// output gradients):
//     d_i      = g_r r_i + g_g g_i + g_b b_i (+ g_D depth_i)       the splat's colours are wave-uniform
//     dL/da_i  = T_i d_i + R / (1 - a_i)                           R = tail - sum over the splats j BEHIND i of w_j d_j
//     R       -= w_i d_i
// The published backward keeps the normalised colour behind i per channel (acc_c = a_last c_last + (1 - a_last) acc_c) and
// forms sum_c (c_i - acc_c) g_c; T_i (1 - a_i) acc_c = sum_{j behind i} c_j w_j (induction on that recursion), so the four
// recursions collapse into the one running scalar R, carried across visits and staging rounds as T is.  A pixel that does not
// take the splat has a_i = 0: w_i = 0 leaves R alone, and G = 0 zeroes every geometric term.
// The geometric terms are all h = G dL/da_i times powers of (dx, dy) times values uniform for the splat: the visit sums the raw
// moments  h, h dx, h dy, h dx dx, h dx dy, h dy dy  and k_preprocess_bwd applies opacity, conic, W/2, H/2 once per Gaussian.
// HAS_DEPTH_GRAD = false (no dL_ddepth: a colour-only loss): the depth term of d_i and the depth slot are compiled out.
// ABS (a caller that asked for dL_dmeans2D_abs): two more per-lane values, ax = |h0 ux0| + |h1 ux1| with ux = cxx dx + cxy dy and ay
// likewise with uy = cyy dy + cxy dx (|h| |u| = |h u| exactly in floating point), summed over the wavefront on their own - the ten
// values above go through reduce_lanes as in the plain instances: one half swap of the PAIR (lanes 0-31 then own ax, lanes 32-63 ay)
// and four full-mask row rotates, after which every lane of a row holds the row's total; lane 11 of each row, the one lane with a
// reduce_lanes by-product nobody reads, hands it to the SAME LDS atomic instruction (rows 0-1: G_AMX, rows 2-3: G_AMY; the atomic
// adds the two rows' partials as it does for reduce_lanes' unpaired values).  A pixel that does not take the splat has h = 0 and
// adds an exact zero; a clamped alpha keeps its gradient as the signed moments do.  ABS = false compiles to the code without it.
template <bool HAS_DEPTH_GRAD, bool ABS>
__global__ void __launch_bounds__(kBwdThreads) k_render_bwd(
    int H, int W, int gx, int gy, const uint2* __restrict__ ranges, const unsigned* __restrict__ point_list,
    const Splat* __restrict__ splats, float bg0, float bg1, float bg2, const unsigned* __restrict__ n_contrib,
    const float* __restrict__ final_T, const float* __restrict__ dL_dcolor, const float* __restrict__ dL_ddepth,
    const float* __restrict__ dL_dalpha_out, float* __restrict__ grad_rec, const unsigned* __restrict__ tile_order) {
    __shared__ float4 sm[kBwdThreads * 3];
    __shared__ unsigned sid[kBwdThreads];
    __shared__ float sacc[kBwdThreads * kGradSlots];   // per-round gradient records: the 2 wavefronts meet here first
    const unsigned tile = tile_order ? tile_order[blockIdx.x] : xcd_remap(blockIdx.x, (unsigned)(gx * gy));
    const int wq = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const BlendFrame f = blend_frame(tile, wq, lane, H, W, gx);
    const bool in0 = f.in0, in1 = f.in1;
    const uint2 range = ranges[tile];
    const size_t hw = (size_t)H * W, pix0 = (size_t)f.py0 * W + f.px, pix1 = (size_t)f.py1 * W + f.px;

    const f2 T_final = (f2){in0 ? final_T[pix0] : 0.0f, in1 ? final_T[pix1] : 0.0f};
    f2 T = T_final;
    const int lc0 = in0 ? (int)n_contrib[pix0] : 0, lc1 = in1 ? (int)n_contrib[pix1] : 0;
    // The forward pass stops a tile once every pixel is saturated; the backward walks back from the LAST splat
    // any pixel of the tile took (max of n_contrib), not from the end of the tile's list.
    __shared__ int s_live;
    int wave_live;                        // the same bound for this wavefront's half alone
    if (threadIdx.x == 0) s_live = 0;
    __syncthreads();
    {
        int mc = max(lc0, lc1);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mc = max(mc, __shfl_xor(mc, o, 64));
        if (lane == 0) atomicMax(&s_live, mc);
        wave_live = mc;
    }
    __syncthreads();
    const int total = min(s_live, (int)(range.y - range.x));
    const int rounds = (total + kBwdThreads - 1) / kBwdThreads;
    const BlendHalf hf = blend_half(tile, wq, gx);
    f2 gr = splat2(0.f), gg = splat2(0.f), gb = splat2(0.f), gD = splat2(0.f), gA = splat2(0.f);
    if (in0) {
        gr.x = dL_dcolor[pix0]; gg.x = dL_dcolor[hw + pix0]; gb.x = dL_dcolor[2 * hw + pix0];
        if constexpr (HAS_DEPTH_GRAD) gD.x = dL_ddepth[pix0];
        gA.x = dL_dalpha_out ? dL_dalpha_out[pix0] : 0.0f;
    }
    if (in1) {
        gr.y = dL_dcolor[pix1]; gg.y = dL_dcolor[hw + pix1]; gb.y = dL_dcolor[2 * hw + pix1];
        if constexpr (HAS_DEPTH_GRAD) gD.y = dL_ddepth[pix1];
        gA.y = dL_dalpha_out ? dL_dalpha_out[pix1] : 0.0f;
    }
    // output terms that do not depend on the splat: background of the colour output and A = 1 - T_final
    const f2 tail = T_final * (gA - (bg0 * gr + bg1 * gg + bg2 * gb));
    f2 R = tail;                          // tail minus the weighted gradient-colour products of everything behind the current splat

    // reduce_lanes' argument order: the depth term last, so that it is the value the colour-only instance leaves out
    constexpr int NV = HAS_DEPTH_GRAD ? 10 : 9;
    const int rval = reduce_value<NV>(lane);
    int rslot = -1;                       // the gradient slot this lane's total belongs to
    {
        const int order[10] = {G_R, G_G, G_B, G_MX, G_MY, G_CXX, G_CXY, G_CYY, G_OP, G_DEPTH};
#pragma unroll
        for (int k = 0; k < 10; ++k) rslot = rval == k ? order[k] : rslot;
    }
    const bool abs_lane = ABS && (lane & 15) == 11;
    if constexpr (ABS) rslot = abs_lane ? (lane < 32 ? G_AMX : G_AMY) : rslot;
    int todo = total;
    // The records of round rd + 1 are requested (list entry, then the 48-byte record: two dependent global loads)
    // BEFORE round rd is processed and land in registers meanwhile: the gather latency is off the critical path.
    float4 n0, n1, n2;
    unsigned ngid = 0;
    bool have = false;
    auto fetch = [&](int rd) {
        const int progress = rd * kBwdThreads + threadIdx.x;
        have = progress < total;
        if (have) {
            ngid = point_list[range.x + total - 1 - progress];   // back to front
            const float4* src = (const float4*)(splats + ngid);
            n0 = src[0]; n1 = src[1]; n2 = src[2];
        }
    };
    fetch(0);
    for (int rd = 0; rd < rounds; ++rd, todo -= kBwdThreads) {
        __syncthreads();
        if (have) {
            stage_splat(sm, threadIdx.x, n0, n1, n2);
            sid[threadIdx.x] = ngid;
        }
        fetch(rd + 1);
#pragma unroll
        for (int k = 0; k < kGradSlots / 4; ++k)
            ((float4*)sacc)[threadIdx.x * (kGradSlots / 4) + k] = make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        const int cnt = min(kBwdThreads, todo);
        // visit list of this wavefront's half (see k_render): one lane-test per staged splat, then a scalar walk
        // over the ballot; splats that cannot reach alpha >= 1/255 on the half are never evaluated
        for (int c0 = 0; c0 < cnt; c0 += 64) {
          bool hit = false;
          if (c0 + lane < cnt) {
              const float4 ta = sm[(c0 + lane) * 3], tb = sm[(c0 + lane) * 3 + 1];
              hit = splat_reaches_rect(ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, hf.sx0, hf.sx1, hf.sy0, hf.sy1) &&
                    (total - 1 - (rd * kBwdThreads + c0 + lane)) < wave_live;
          }
          unsigned long long vm = __ballot(hit);
          RASTER_STAT(g_bwd_stats, 0, min(64, cnt - c0));
          RASTER_STAT(g_bwd_stats, 1, __popcll(vm));
          while (vm) {
            const int j = c0 + (int)__builtin_ctzll(vm);
            vm &= vm - 1;
            const int contributor = total - 1 - (rd * kBwdThreads + j);
            const float4 a = sm[j * 3], b = sm[j * 3 + 1], c = sm[j * 3 + 2];
            const BlendEval e = blend_eval(a, b, f);
            const float dx = e.dx;
            const f2 dy = e.dy, power = e.power, araw = b.y * e.G;
            f2 G = e.G;
            const bool act0 = (contributor < lc0) && (power.x <= 0.0f) && (fminf(kAlphaMax, araw.x) >= kAlphaMin);
            const bool act1 = (contributor < lc1) && (power.y <= 0.0f) && (fminf(kAlphaMax, araw.y) >= kAlphaMin);
            if (__ballot(act0 || act1) == 0ull) continue;   // wave-uniform
            RASTER_STAT(g_bwd_stats, 2, 1); RASTER_STAT(g_bwd_stats, 3, __popcll(__ballot(act0)) + __popcll(__ballot(act1)));
            // Branch-free: a pixel that does not take this splat blends it with alpha = 0 and G = 0, which is an exact
            // no-op on its running state (T * rcp(1) = T, R - 0 * d = R) and makes every gradient term an exact
            // zero - no EXEC-masked region.
            const f2 a_eff = (f2){act0 ? fminf(kAlphaMax, araw.x) : 0.0f, act1 ? fminf(kAlphaMax, araw.y) : 0.0f};
            G = (f2){act0 ? G.x : 0.0f, act1 ? G.y : 0.0f};
            const f2 one_m = 1.0f - a_eff;
            const f2 inv1ma = (f2){__builtin_amdgcn_rcpf(one_m.x), __builtin_amdgcn_rcpf(one_m.y)};   // 1 ulp reciprocal
            T = T * inv1ma;
            const f2 wgt = a_eff * T;
            // one running scalar for everything behind this splat (see the kernel's header)
            f2 d = b.z * gr;
            d = b.w * gg + d;
            d = c.x * gb + d;
            if constexpr (HAS_DEPTH_GRAD) d = c.y * gD + d;
            const f2 dL_da = T * d + inv1ma * R;
            R = R - wgt * d;
            // raw moments of h = G dL/dalpha; opacity, conic and the pixel -> NDC factors wait for k_preprocess_bwd
            const f2 h = G * dL_da;
            // the two pixels of a lane share dx: the x moments are formed from the pair's sums
            const f2 hy = h * dy, hyy = hy * dy;
            const f2 wr = wgt * gr, wg = wgt * gg, wb = wgt * gb;
            const float Sh = h.x + h.y, Sy = hy.x + hy.y, Sx = Sh * dx;
            float v[10];
            v[0] = wr.x + wr.y; v[1] = wg.x + wg.y; v[2] = wb.x + wb.y;
            v[3] = Sx;
            v[4] = Sy;
            v[5] = Sx * dx;
            v[6] = Sy * dx;
            v[7] = hyy.x + hyy.y;
            v[8] = Sh;
            v[9] = 0.0f;
            if constexpr (HAS_DEPTH_GRAD) { const f2 wd = wgt * gD; v[9] = wd.x + wd.y; }
            float s = reduce_lanes<NV>(v);
            if constexpr (ABS) {
                const f2 ux = a.w * dy + splat2(a.z * dx), uy = b.x * dy + splat2(a.w * dx);
                const f2 hux = h * ux, huy = h * uy;
                const float ax = fabsf(hux.x) + fabsf(hux.y), ay = fabsf(huy.x) + fabsf(huy.y);
                auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(ax), __float_as_int(ay), false, false);
                float t = __int_as_float(r[0]) + __int_as_float(r[1]);
                // one block with its wait states, as in reduce_lanes: two between a VALU write of t and the DPP read of it
                asm("s_nop 1\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
                    "s_nop 1\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
                    "s_nop 1\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
                    "s_nop 1\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf"
                    : "+v"(t));
                s = abs_lane ? t : s;
            }
            if (rslot >= 0) atomicAdd(&sacc[j * kGradSlots + rslot], s);   // LDS, 10 banks (12 with ABS)
          }
        }
        // one global atomic per (tile, splat) instead of one per (wavefront, splat): 16 lanes per record, so a
        // wave-instruction covers four contiguous 64-byte records
        __syncthreads();
        {
            const int slot = threadIdx.x & 15;
            for (int q = threadIdx.x >> 4; q < cnt; q += kBwdThreads / 16) {
                float val = sacc[q * kGradSlots + slot];
                if (slot < (ABS ? G_USED_ABS : G_USED) && val != 0.0f) unsafeAtomicAdd(grad_rec + (size_t)sid[q] * kGradSlots + slot, val);
            }
        }
    }
}

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 f3(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ F3 operator*(float s, F3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ F3 operator+(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ float dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// SH colour backward: writes dL_dsh (M x 3) and returns dL_dmean through the view direction
// PRELOAD (M == 16): every coefficient is read into registers before the first output is written, so `dL_dsh` may be the row
// `sh` itself (k_preprocess_bwd's LDS-staged rows)
// WRITE = false: dL_dsh is not written (the camera pass of k_preprocess_bwd wants the returned direction gradient alone)
template <bool PRELOAD, bool WRITE = true>
__device__ __forceinline__ F3 sh_backward(int D, int M, F3 pos, const float* campos, const float* sh, unsigned clamped,
                                          F3 dL_dRGB, float* dL_dsh) {
    F3 dir_o = f3(pos.x - campos[0], pos.y - campos[1], pos.z - campos[2]);
    float len2 = dot(dir_o, dir_o);
    float inv = 1.0f / sqrtf(len2);
    float x = dir_o.x * inv, y = dir_o.y * inv, z = dir_o.z * inv;
    if (clamped & 1u) dL_dRGB.x = 0.0f;
    if (clamped & 2u) dL_dRGB.y = 0.0f;
    if (clamped & 4u) dL_dRGB.z = 0.0f;
    float pre[PRELOAD ? 48 : 1];
    if constexpr (PRELOAD) {
#pragma unroll
        for (int k = 0; k < 48; ++k) pre[k] = sh[k];
    }
    auto c = [&](int k) { return PRELOAD ? f3(pre[3 * k], pre[3 * k + 1], pre[3 * k + 2]) : f3(sh[3 * k], sh[3 * k + 1], sh[3 * k + 2]); };
    auto put = [&](int k, float s) {
        if constexpr (!WRITE) return;
        dL_dsh[3 * k] = s * dL_dRGB.x; dL_dsh[3 * k + 1] = s * dL_dRGB.y; dL_dsh[3 * k + 2] = s * dL_dRGB.z;
    };
    F3 dx = f3(0, 0, 0), dy = f3(0, 0, 0), dz = f3(0, 0, 0);
    put(0, SH_C0);
    if (D > 0) {
        put(1, -SH_C1 * y); put(2, SH_C1 * z); put(3, -SH_C1 * x);
        dx = -SH_C1 * c(3); dy = -SH_C1 * c(1); dz = SH_C1 * c(2);
        if (D > 1) {
            float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            put(4, SH_C2[0] * xy); put(5, SH_C2[1] * yz); put(6, SH_C2[2] * (2.f * zz - xx - yy));
            put(7, SH_C2[3] * xz); put(8, SH_C2[4] * (xx - yy));
            dx = dx + (SH_C2[0] * y) * c(4) + (SH_C2[2] * 2.f * -x) * c(6) + (SH_C2[3] * z) * c(7) + (SH_C2[4] * 2.f * x) * c(8);
            dy = dy + (SH_C2[0] * x) * c(4) + (SH_C2[1] * z) * c(5) + (SH_C2[2] * 2.f * -y) * c(6) + (SH_C2[4] * 2.f * -y) * c(8);
            dz = dz + (SH_C2[1] * y) * c(5) + (SH_C2[2] * 2.f * 2.f * z) * c(6) + (SH_C2[3] * x) * c(7);
            if (D > 2) {
                put(9, SH_C3[0] * y * (3.f * xx - yy)); put(10, SH_C3[1] * xy * z);
                put(11, SH_C3[2] * y * (4.f * zz - xx - yy)); put(12, SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy));
                put(13, SH_C3[4] * x * (4.f * zz - xx - yy)); put(14, SH_C3[5] * z * (xx - yy));
                put(15, SH_C3[6] * x * (xx - 3.f * yy));
                dx = dx + (SH_C3[0] * 3.f * 2.f * xy) * c(9) + (SH_C3[1] * yz) * c(10) + (SH_C3[2] * -2.f * xy) * c(11) +
                     (SH_C3[3] * -3.f * 2.f * xz) * c(12) + (SH_C3[4] * (-3.f * xx + 4.f * zz - yy)) * c(13) +
                     (SH_C3[5] * 2.f * xz) * c(14) + (SH_C3[6] * 3.f * (xx - yy)) * c(15);
                dy = dy + (SH_C3[0] * 3.f * (xx - yy)) * c(9) + (SH_C3[1] * xz) * c(10) +
                     (SH_C3[2] * (-3.f * yy + 4.f * zz - xx)) * c(11) + (SH_C3[3] * -3.f * 2.f * yz) * c(12) +
                     (SH_C3[4] * -2.f * xy) * c(13) + (SH_C3[5] * -2.f * yz) * c(14) + (SH_C3[6] * -3.f * 2.f * xy) * c(15);
                dz = dz + (SH_C3[1] * xy) * c(10) + (SH_C3[2] * 4.f * 2.f * yz) * c(11) +
                     (SH_C3[3] * 3.f * (2.f * zz - xx - yy)) * c(12) + (SH_C3[4] * 4.f * 2.f * xz) * c(13) +
                     (SH_C3[5] * (xx - yy)) * c(14);
            }
        }
    }
    for (int k = (D + 1) * (D + 1); k < M; ++k) put(k, 0.0f);
    F3 dL_ddir = f3(dot(dx, dL_dRGB), dot(dy, dL_dRGB), dot(dz, dL_dRGB));
    // d(v/|v|): (g - vhat (vhat . g)) / |v|
    F3 vh = f3(x, y, z);
    float vg = dot(vh, dL_ddir);
    return f3((dL_ddir.x - x * vg) * inv, (dL_ddir.y - y * vg) * inv, (dL_ddir.z - z * vg) * inv);
}

// STAGED (sh_coeffs == 16, 16-byte aligned tensors): a block's spherical-harmonics rows (256 x 192 B, contiguous in memory) come in
// and its gradient rows go out through LDS with coalesced 16-byte accesses; a thread reading and writing its own 192-byte row in
// global memory touches 64 different cache lines per wave instruction (32 of the kernel's 42 us at 200 000 Gaussians).
// AA and F3D are explained where the forward's values are formed (mip_rho, f3d_scales, mode_factors in raster_common.h: this kernel
// calls the same functions, so rho and coef are the forward's bits); here, the derivatives.  G = gr[G_OP] is dL/d(the blend opacity)
// = dL/d(op [coef] [rho] cf).
// AA: rho = mip_rho(r), r = d0 / d1 with d0 = a c - b^2 the determinant before the dilation and d1 = A C - b^2 (= `den`) after it
// (A = a + h, C = c + h, h = kLowPass).  dL/dop = G cf rho, dL/dcf = G op rho, dL/drho = G op cf, and above the floor
// dL/dr = dL/drho / (2 rho) (on the floor rho is a constant) enters the covariance gradients through
//     dr/da = (c d1 - C d0) / d1^2 = h (c C + b^2) / d1^2      dr/dc = (a d1 - A d0) / d1^2 = h (a A + b^2) / d1^2
//     dr/db = -2 b (d1 - d0) / d1^2 = -2 b h (a + C) / d1^2
// (the right-hand forms are the same polynomials with A - a = C - c = h taken out: no difference of two large products in fp32).
// F3D: q_i = sqrt(s_i^2 + f^2), coef = prod r_i, r_i = s_i / q_i.  dL/dop = G coef [rho] cf, dL/dcf = G op coef [rho], the rho terms
// above carry coef, and the scales receive
//     dL/ds_i = dL/dq_i r_i + G op cf [rho] coef f^2 / (s_i q_i^2)         (dq_i/ds_i = r_i, dcoef/ds_i = coef f^2 / (s_i q_i^2))
// evaluated WITHOUT the division by s_i: coef / s_i = prod_{j != i} r_j / q_i on the activated route, and on the raw route the
// chain rule's factor s_i cancels it (dL/dlog s_i = dL/dq_i r_i s_i + G op cf [rho] coef f^2 / q_i^2).  The filter gets no gradient.
// The scales are loaded BEFORE the opacity gradient is written on the F3D path only (coef is needed there).
// POSE (a caller that asked for dL_dcamera, syn3r_raster_backward_cam; launched AFTER the POSE = false instance of the same mode): every
// thread forms the 27 terms its Gaussian adds to the gradients of the camera - the three inputs taken as INDEPENDENT, as the ABI takes them:
//     view (12):  t = view [p,1], so dL/dview[c*4+r] += [p,1]_c (dtx, dty, dtz)_r; W = view[:3,:3] also enters T = J W, so dL/dW = J^T dT
//                 with J = (J00 0 J02; 0 J11 J12) the VALUES ewa_rows used (J02 / J12 from the clamped tx / ty: inside dT they are
//                 factors; the guard band's x_mul / y_mul are in dtx / dty already)
//     proj (12):  ph = proj [p,1] (x, y, w read): dL/dph = (mw g2x, mw g2y, -(mul1 g2x + mul2 g2y)), outer product with [p,1]
//     campos (3): the SH direction is p - campos: -dm_sh
// AA and F3D add nothing: their rho / coef terms are in dL_dA/B/C and hence in dT.  A culled Gaussian and a thread past N add zeros.
// The block's sums leave as ONE row of kPoseRow floats (pose_row_sum), without atomics; k_camera_grad_finish adds the rows.  POSE = false
// compiles to the code without any of it.  The POSE instance is the SAME chain rule with the stores of the per-Gaussian outputs compiled
// out (and with them whatever only they need: the scale / rotation part, the SH products): the per-Gaussian gradients of a call with
// dL_dcamera are written by the POSE = false instance and are the bits of a call without it.  One kernel that did both was tried first:
// the 27 extra products change which multiplications hipcc pairs into packed instructions and hence which of them it contracts with
// an addition, and dL_dshs / dL_dmeans3D came out an ulp away from the plain instance's.
constexpr int kPoseTerms = 27, kPoseRow = 32;
// Sum kPoseRow per-thread values (27 terms, 5 zeros) over the block of four wavefronts and write them to `row`.  Two transposing
// levels (reduce_lanes' half and row swaps: 32 -> 16 -> 8 live values), then four xor steps inside a 16-lane row; all through
// compiler-visible builtins, so hipcc places the wait states.  Lane 16 q of a wavefront ends with the wavefront's totals of the
// values k + 8 (q & 1) + 16 (q >> 1), k = 0 .. 7.  The four wavefronts meet in `lds` (an array of its own: the STAGED instances still
// hold `shl`) and are added in a fixed order: the row is the same bits in every launch.  Every thread of the block must call this.
__device__ __forceinline__ void pose_row_sum(float (&v)[kPoseRow], float (&lds)[4][kPoseRow], float* __restrict__ row) {
    float a[16], b[8];
#pragma unroll
    for (int k = 0; k < 16; ++k) {   // the lower half owns value k, the upper k + 16
        auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(v[k]), __float_as_int(v[k + 16]), false, false);
        a[k] = __int_as_float(r[0]) + __int_as_float(r[1]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {    // even rows own k, odd rows k + 8
        auto r = __builtin_amdgcn_permlane16_swap(__float_as_int(a[k]), __float_as_int(a[k + 8]), false, false);
        b[k] = __int_as_float(r[0]) + __int_as_float(r[1]);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < 8; ++k) b[k] += __shfl_xor(b[k], o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
    if ((lane & 15) == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) lds[wave][k + 8 * (q & 1) + 16 * (q >> 1)] = b[k];
    }
    __syncthreads();
    if (threadIdx.x < kPoseRow) row[threadIdx.x] = ((lds[0][threadIdx.x] + lds[1][threadIdx.x]) + lds[2][threadIdx.x]) + lds[3][threadIdx.x];
}

constexpr int kShLd = 49;      // LDS row stride (floats): odd, so the 64 rows of a wavefront fall into 64 banks
template <bool STAGED, bool AA, bool F3D, bool POSE>
__global__ void __launch_bounds__(256) k_preprocess_bwd(
    int N, int D, int M, const float* __restrict__ means3D, const float* __restrict__ scales,
    const float* __restrict__ rots, const float* __restrict__ opacities, const float* __restrict__ shs,
    const float* __restrict__ conf, float scale_mod, Camera cam, const int* __restrict__ radii, GeomState g,
    const float* __restrict__ grad_rec, float* __restrict__ dL_dmeans3D, float* __restrict__ dL_dscales,
    float* __restrict__ dL_drots, float* __restrict__ dL_dopacity, float* __restrict__ dL_dshs,
    float* __restrict__ dL_dmeans2D, float* __restrict__ dL_dconf, int raw, const float* __restrict__ filter3d,
    float* __restrict__ pose_rows) {
    __shared__ float shl[STAGED ? 256 * kShLd : 1];
    float pz[POSE ? kPoseRow : 1];        // this thread's camera terms: view 0-11 (c * 3 + r), proj 12-23 (c * 3 + x/y/w), campos 24-26
    if constexpr (POSE) {
#pragma unroll
        for (int k = 0; k < kPoseRow; ++k) pz[k] = 0.0f;
    }
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t blk0 = (size_t)blockIdx.x * 256 * 48;                // first float of the block's rows
    const int rows = min(256, N - (int)blockIdx.x * 256);
    if constexpr (STAGED) {
        // the twelve loads of a thread are issued TOGETHER (a full block: every block but the last); behind a per-load `row < rows`
        // branch each would wait for the one before it (hipcc keeps a load inside its exec-mask region)
        if (rows == 256) {
            float4 v4[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) v4[k] = *(const float4*)(shs + blk0 + (threadIdx.x + 256 * k) * 4);
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                const int e = (threadIdx.x + 256 * k) * 4, row = e / 48, col = e - row * 48;
                float* d = &shl[row * kShLd + col];
                d[0] = v4[k].x; d[1] = v4[k].y; d[2] = v4[k].z; d[3] = v4[k].w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                const int e = (threadIdx.x + 256 * k) * 4, row = e / 48, col = e - row * 48;
                if (row < rows) {
                    const float4 v4 = *(const float4*)(shs + blk0 + e);
                    float* d = &shl[row * kShLd + col];
                    d[0] = v4.x; d[1] = v4.y; d[2] = v4.z; d[3] = v4.w;
                }
            }
        }
        __syncthreads();
    }
    if (i < N) do {
    float* osh = STAGED ? &shl[threadIdx.x * kShLd] : dL_dshs + (size_t)i * M * 3;
    if (radii[i] <= 0) {
        if constexpr (POSE) break;
        for (int k = 0; k < 3; ++k) { dL_dmeans3D[3 * i + k] = 0.f; dL_dscales[3 * i + k] = 0.f; dL_dmeans2D[3 * i + k] = 0.f; }
        for (int k = 0; k < 4; ++k) dL_drots[4 * i + k] = 0.f;
        dL_dopacity[i] = 0.f;
        if (dL_dconf) dL_dconf[i] = 0.f;
        for (int k = 0; k < 3 * M; ++k) osh[k] = 0.f;
        break;
    }
    const float* gr = grad_rec + (size_t)i * kGradSlots;
    const float3 p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
    const float* v = cam.view;
    const float3 t = xf43(v, p);

    // ---- conic -> 2D covariance
    const float* cv = g.cov3D + 6 * (size_t)i;
    float c0 = cv[0], c1 = cv[1], c2 = cv[2], c3 = cv[3], c4 = cv[4], c5 = cv[5];
    float limx = kFovGuard * cam.tanfovx, limy = kFovGuard * cam.tanfovy;
    float txtz = t.x / t.z, tytz = t.y / t.z;
    float x_mul = (txtz < -limx || txtz > limx) ? 0.0f : 1.0f;
    float y_mul = (tytz < -limy || tytz > limy) ? 0.0f : 1.0f;
    const EwaRows w = ewa_rows(cam, t.x, t.y, t.z);
    const float tx = w.tx, ty = w.ty, T00 = w.T00, T01 = w.T01, T02 = w.T02, T10 = w.T10, T11 = w.T11, T12 = w.T12;
    float W00 = v[0], W01 = v[4], W02 = v[8], W10 = v[1], W11 = v[5], W12 = v[9], W20 = v[2], W21 = v[6], W22 = v[10];
    const auto [a0, a1, a2, b0, b1, b2, pA, pC, B] = ewa_cov(w, c0, c1, c2, c3, c4, c5);   // (pA, B; B, pC): before the dilation
    float A = pA + kLowPass;
    float C = pC + kLowPass;
    float den = A * C - B * B;
    float den2inv = 1.0f / (den * den + 0.0000001f);
    // the blend summed raw moments (k_render_bwd); the factors are the float values IT multiplied: the splat record's conic and its
    // opacity x confidence (GeomState::conic_opacity holds the opacity without the confidence)
    const Splat* sp = g.splats + i;
    const float s_cxx = sp->cxx, s_cxy = sp->cxy, s_cyy = sp->cyy, s_op = sp->opacity;
    float gxx = -0.5f * s_op * gr[G_CXX], gxy = -s_op * gr[G_CXY], gyy = -0.5f * s_op * gr[G_CYY];
    float dL_dA = 0.f, dL_dB = 0.f, dL_dC = 0.f;
    if (den2inv != 0.0f) {
        dL_dA = den2inv * (-C * C * gxx + B * C * gxy + (den - A * C) * gyy);
        dL_dC = den2inv * ((den - A * C) * gxx + A * B * gxy - A * A * gyy);
        dL_dB = den2inv * (2.f * B * C * gxx - (den + 2.f * B * B) * gxy + 2.f * A * B * gyy);
    }
    // raw (syn3r_raster_backward_raw): `scales` / `rots` / `opacities` are the trainer's PARAMETERS; the activations are formed
    // again (k_activate's arithmetic, common.h) and the gradients leave through their chain rule (k_activate_bwd's): the same bits
    // as the two-launch route
    const float cf = conf ? conf[i] : 1.0f;
    const float op_a = raw ? act_sigmoid(opacities[i]) : opacities[i];
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    F3dScales fs;
    if constexpr (F3D) {
        s0 = scales[3 * i]; s1 = scales[3 * i + 1]; s2 = scales[3 * i + 2];
        if (raw) { s0 = act_exp(s0); s1 = act_exp(s1); s2 = act_exp(s2); }
        fs = f3d_scales(s0, s1, s2, filter3d[i]);
    }
    float rho = 1.0f;
    if constexpr (AA) {
        const float r = mip_ratio(pA, B, pC), den_inv = 1.0f / den;     // r: the forward's bits (one function, explicit roundings)
        rho = mip_rho(r);
        if (r > kMipFloor) {
            float k = gr[G_OP] * op_a * cf / (2.0f * rho) * kLowPass * den_inv * den_inv;   // dL/dr h / d1^2
            if constexpr (F3D) k *= fs.coef;
            dL_dA += k * (pC * C + B * B);
            dL_dC += k * (pA * A + B * B);
            dL_dB -= k * 2.0f * B * (pA + C);
        }
    }
    // dL/dSigma (stored upper triangle; off-diagonals count both symmetric entries)
    float dS0 = T00 * T00 * dL_dA + T00 * T10 * dL_dB + T10 * T10 * dL_dC;
    float dS3 = T01 * T01 * dL_dA + T01 * T11 * dL_dB + T11 * T11 * dL_dC;
    float dS5 = T02 * T02 * dL_dA + T02 * T12 * dL_dB + T12 * T12 * dL_dC;
    float dS1 = 2.f * T00 * T01 * dL_dA + (T00 * T11 + T01 * T10) * dL_dB + 2.f * T10 * T11 * dL_dC;
    float dS2 = 2.f * T00 * T02 * dL_dA + (T00 * T12 + T02 * T10) * dL_dB + 2.f * T10 * T12 * dL_dC;
    float dS4 = 2.f * T02 * T01 * dL_dA + (T01 * T12 + T02 * T11) * dL_dB + 2.f * T11 * T12 * dL_dC;
    // dL/dT, T = J W (2x3)
    float dT00 = 2.f * a0 * dL_dA + b0 * dL_dB, dT01 = 2.f * a1 * dL_dA + b1 * dL_dB, dT02 = 2.f * a2 * dL_dA + b2 * dL_dB;
    float dT10 = 2.f * b0 * dL_dC + a0 * dL_dB, dT11 = 2.f * b1 * dL_dC + a1 * dL_dB, dT12 = 2.f * b2 * dL_dC + a2 * dL_dB;
    float dJ00 = W00 * dT00 + W01 * dT01 + W02 * dT02;
    float dJ02 = W20 * dT00 + W21 * dT01 + W22 * dT02;
    float dJ11 = W10 * dT10 + W11 * dT11 + W12 * dT12;
    float dJ12 = W20 * dT10 + W21 * dT11 + W22 * dT12;
    float tz = 1.f / t.z, tz2 = tz * tz, tz3 = tz2 * tz;
    float dtx = x_mul * -cam.focal_x * tz2 * dJ02;
    float dty = y_mul * -cam.focal_y * tz2 * dJ12;
    float dtz = -cam.focal_x * tz2 * dJ00 - cam.focal_y * tz2 * dJ11 + (2.f * cam.focal_x * tx) * tz3 * dJ02 +
                (2.f * cam.focal_y * ty) * tz3 * dJ12;
    // depth output: d(view z)/d(mean)
    dtz += gr[G_DEPTH];
    F3 dmean = f3(W00 * dtx + W10 * dty + W20 * dtz, W01 * dtx + W11 * dty + W21 * dtz, W02 * dtx + W12 * dty + W22 * dtz);

    // ---- screen-space mean (NDC) -> mean
    const float* pj = cam.proj;
    const float4 ph = xf44(pj, p);
    float mw = 1.0f / (ph.w + 0.0000001f);
    float mul1 = ph.x * mw * mw, mul2 = ph.y * mw * mw;
    float g2x = -0.5f * (float)cam.W * s_op * (s_cxx * gr[G_MX] + s_cxy * gr[G_MY]);
    float g2y = -0.5f * (float)cam.H * s_op * (s_cyy * gr[G_MY] + s_cxy * gr[G_MX]);
    dmean.x += (pj[0] * mw - pj[3] * mul1) * g2x + (pj[1] * mw - pj[3] * mul2) * g2y;
    dmean.y += (pj[4] * mw - pj[7] * mul1) * g2x + (pj[5] * mw - pj[7] * mul2) * g2y;
    dmean.z += (pj[8] * mw - pj[11] * mul1) * g2x + (pj[9] * mw - pj[11] * mul2) * g2y;
    if constexpr (!POSE) { dL_dmeans2D[3 * i] = g2x; dL_dmeans2D[3 * i + 1] = g2y; dL_dmeans2D[3 * i + 2] = 0.f; }

    // ---- colour -> SH and mean
    F3 dm_sh = sh_backward<STAGED, !POSE>(D, M, f3(p.x, p.y, p.z), cam.campos, STAGED ? (const float*)osh : shs + (size_t)i * M * 3, g.clamped[i],
                                   f3(gr[G_R], gr[G_G], gr[G_B]), osh);
    dmean = dmean + dm_sh;
    if constexpr (POSE) {
        const float J00 = cam.focal_x * tz, J02 = -(cam.focal_x * tx) * tz2, J11 = cam.focal_y * tz, J12 = -(cam.focal_y * ty) * tz2;
        const float pc[4] = {p.x, p.y, p.z, 1.0f};
        const float dT0[3] = {dT00, dT01, dT02}, dT1[3] = {dT10, dT11, dT12};
        const float dph_x = mw * g2x, dph_y = mw * g2y, dph_w = -(mul1 * g2x + mul2 * g2y);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            pz[3 * c] = pc[c] * dtx; pz[3 * c + 1] = pc[c] * dty; pz[3 * c + 2] = pc[c] * dtz;
            pz[12 + 3 * c] = pc[c] * dph_x; pz[13 + 3 * c] = pc[c] * dph_y; pz[14 + 3 * c] = pc[c] * dph_w;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {     // dL/dW[r][c], W[r][c] = view[c * 4 + r]
            pz[3 * c] += J00 * dT0[c]; pz[3 * c + 1] += J11 * dT1[c]; pz[3 * c + 2] += J02 * dT0[c] + J12 * dT1[c];
        }
        pz[24] = -dm_sh.x; pz[25] = -dm_sh.y; pz[26] = -dm_sh.z;
        break;                            // the per-Gaussian outputs are the POSE = false instance's
    }
    dL_dmeans3D[3 * i] = dmean.x; dL_dmeans3D[3 * i + 1] = dmean.y; dL_dmeans3D[3 * i + 2] = dmean.z;

    // ---- opacity / confidence (blend used opacity * confidence; cf and op_a: above the AA block)
    // rho goes on G first and coef second, as this kernel has always multiplied them: g_rho = G [rho] = dL/d(op coef cf) / (op cf)
    const float g_rho = mode_factors(gr[G_OP], 1.0f, rho);
    const float g_op = mode_factors(g_rho, F3D ? fs.coef : 1.0f, 1.0f);   // dL/d(op x cf)
    dL_dopacity[i] = raw ? act_sigmoid_bwd(op_a, g_op * cf) : g_op * cf;
    if (dL_dconf) dL_dconf[i] = g_op * op_a;

    // ---- Sigma = M M^T, M = R S  -> scale, rotation
    if constexpr (!F3D) { s0 = scales[3 * i]; s1 = scales[3 * i + 1]; s2 = scales[3 * i + 2]; }
    float4 q4 = make_float4(rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3]);
    float q_inv = 1.0f;
    if (raw) {
        if constexpr (!F3D) { s0 = act_exp(s0); s1 = act_exp(s1); s2 = act_exp(s2); }
        q_inv = act_quat_inv_norm(q4);
        q4 = act_quat(q4, q_inv);
    }
    float sx = scale_mod * s0, sy = scale_mod * s1, sz = scale_mod * s2;
    if constexpr (F3D) { sx = scale_mod * fs.q0; sy = scale_mod * fs.q1; sz = scale_mod * fs.q2; }   // the covariance's scales
    float qr = q4.x, qx = q4.y, qy = q4.z, qz = q4.w;
    const auto [R00, R01, R02, R10, R11, R12, R20, R21, R22] = quat_rotation(q4);
    float m00 = R00 * sx, m01 = R01 * sy, m02 = R02 * sz;
    float m10 = R10 * sx, m11 = R11 * sy, m12 = R12 * sz;
    float m20 = R20 * sx, m21 = R21 * sy, m22 = R22 * sz;
    // full symmetric gradient G (off-diagonals halved); dL/dM = 2 G M
    float G00 = dS0, G11 = dS3, G22 = dS5, G01 = 0.5f * dS1, G02 = 0.5f * dS2, G12 = 0.5f * dS4;
    float dM00 = 2.f * (G00 * m00 + G01 * m10 + G02 * m20), dM01 = 2.f * (G00 * m01 + G01 * m11 + G02 * m21),
          dM02 = 2.f * (G00 * m02 + G01 * m12 + G02 * m22);
    float dM10 = 2.f * (G01 * m00 + G11 * m10 + G12 * m20), dM11 = 2.f * (G01 * m01 + G11 * m11 + G12 * m21),
          dM12 = 2.f * (G01 * m02 + G11 * m12 + G12 * m22);
    float dM20 = 2.f * (G02 * m00 + G12 * m10 + G22 * m20), dM21 = 2.f * (G02 * m01 + G12 * m11 + G22 * m21),
          dM22 = 2.f * (G02 * m02 + G12 * m12 + G22 * m22);
    float ds0 = scale_mod * (dM00 * R00 + dM10 * R10 + dM20 * R20);
    float ds1 = scale_mod * (dM01 * R01 + dM11 * R11 + dM21 * R21);
    float ds2 = scale_mod * (dM02 * R02 + dM12 * R12 + dM22 * R22);
    float dR00 = dM00 * sx, dR01 = dM01 * sy, dR02 = dM02 * sz;
    float dR10 = dM10 * sx, dR11 = dM11 * sy, dR12 = dM12 * sz;
    float dR20 = dM20 * sx, dR21 = dM21 * sy, dR22 = dM22 * sz;
    float4 dq;
    dq.x = 2.f * (-qz * dR01 + qy * dR02 + qz * dR10 - qx * dR12 - qy * dR20 + qx * dR21);
    dq.y = 2.f * (qy * dR01 + qz * dR02 + qy * dR10 - 2.f * qx * dR11 - qr * dR12 + qz * dR20 + qr * dR21 -
                  2.f * qx * dR22);
    dq.z = 2.f * (-2.f * qy * dR00 + qx * dR01 + qr * dR02 + qx * dR10 + qz * dR12 - qr * dR20 + qz * dR21 -
                  2.f * qy * dR22);
    dq.w = 2.f * (-2.f * qz * dR00 - qr * dR01 + qx * dR02 + qr * dR10 - 2.f * qz * dR11 + qy * dR12 +
                  qx * dR20 + qy * dR21);
    if constexpr (F3D) {
        // ds_i is dL/dq_i so far; kc = G op cf [rho] = dL/dcoef.  fs.ff == 0: coef is the constant 1 (and q_i may be 0)
        const float kc = g_rho * op_a * cf;
        if (raw) {
            ds0 *= fs.r0 * s0; ds1 *= fs.r1 * s1; ds2 *= fs.r2 * s2;
            if (fs.ff > 0.0f) {
                const float kf = kc * fs.coef * fs.ff;
                ds0 += kf / (fs.q0 * fs.q0); ds1 += kf / (fs.q1 * fs.q1); ds2 += kf / (fs.q2 * fs.q2);
            }
        } else {
            ds0 *= fs.r0; ds1 *= fs.r1; ds2 *= fs.r2;
            if (fs.ff > 0.0f) {
                const float kf = kc * fs.ff;
                ds0 += kf * (fs.r1 * fs.r2) / (fs.q0 * fs.q0 * fs.q0);
                ds1 += kf * (fs.r0 * fs.r2) / (fs.q1 * fs.q1 * fs.q1);
                ds2 += kf * (fs.r0 * fs.r1) / (fs.q2 * fs.q2 * fs.q2);
            }
        }
        if (raw) dq = act_quat_bwd(q4, dq, q_inv);
    } else if (raw) {
        ds0 *= s0; ds1 *= s1; ds2 *= s2;
        dq = act_quat_bwd(q4, dq, q_inv);
    }
    dL_dscales[3 * i] = ds0; dL_dscales[3 * i + 1] = ds1; dL_dscales[3 * i + 2] = ds2;
    dL_drots[4 * i] = dq.x; dL_drots[4 * i + 1] = dq.y; dL_drots[4 * i + 2] = dq.z; dL_drots[4 * i + 3] = dq.w;
    } while (0);
    if constexpr (POSE) {                 // uniform control flow: culled Gaussians, threads past N and the last block arrive with zeros
        __shared__ float pose_lds[4][kPoseRow];
        pose_row_sum(pz, pose_lds, pose_rows + (size_t)blockIdx.x * kPoseRow);
    }
    if constexpr (STAGED && !POSE) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const int e = (threadIdx.x + 256 * k) * 4, row = e / 48, col = e - row * 48;
            if (row < rows) {
                const float* d = &shl[row * kShLd + col];
                *(float4*)(dL_dshs + blk0 + e) = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
    }
}

// dL_dmeans2D_abs of the `_abs` entry: the element-wise absolute counterpart of (g2x, g2y) above, from the two slots the ABS instances
// of k_render_bwd summed.  s_op is the splat record's blend opacity, the value the blend multiplied (opacity x confidence, x rho and
// x coef in the anti-aliased and filtered modes: non-negative); culled Gaussians write zeros.  A kernel of its own, launched only for
// a caller that asked: k_preprocess_bwd is the same code with and without it.
__global__ void __launch_bounds__(256) k_abs_means2D(int N, float half_w, float half_h, const int* __restrict__ radii,
                                                     const Splat* __restrict__ splats, const float* __restrict__ grad_rec,
                                                     float* __restrict__ abs2D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float2 o = make_float2(0.0f, 0.0f);
    if (radii[i] > 0) {
        const float s_op = splats[i].opacity;
        const float2 m = *(const float2*)(grad_rec + (size_t)i * kGradSlots + G_AMX);
        o = make_float2(half_w * s_op * m.x, half_h * s_op * m.y);
    }
    *(float2*)(abs2D + 2 * (size_t)i) = o;
}

// dL_dcamera of the `_cam` entry: the block rows of the POSE instances of k_preprocess_bwd, added in a fixed order (thread (g, col)
// takes rows g, g + 32, ... of column col, then the 32 groups in order) with fp64 accumulators, rounded once to fp32 and written in
// the storage order of the three inputs: view[16], proj[16], campos[3].  The third clip row (proj 2, 6, 10, 14) and the fourth view
// row (view 3, 7, 11, 15) are not read by the render: exact zeros.  accumulate != 0: one fp32 add per slot onto what `out` holds.
// One block of 1024 threads (782 rows at 200 000 Gaussians: 25 per thread, the loads of eight rows in flight at a time - with 256
// threads and one load per dependent add the kernel took 24 us); the same bits in every launch.
constexpr int kCameraGrad = 35, kFinishGroups = 32;
__global__ void __launch_bounds__(kFinishGroups * kPoseRow) k_camera_grad_finish(int nrows, const float* __restrict__ rows,
                                                                                 float* __restrict__ out, int accumulate) {
    __shared__ double part[kFinishGroups][kPoseRow];
    const int col = threadIdx.x & (kPoseRow - 1), grp = threadIdx.x / kPoseRow;
    double acc = 0.0;
    int r = grp;
    for (; r + 7 * kFinishGroups < nrows; r += 8 * kFinishGroups) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = rows[(size_t)(r + k * kFinishGroups) * kPoseRow + col];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += (double)v[k];
    }
    for (; r < nrows; r += kFinishGroups) acc += (double)rows[(size_t)r * kPoseRow + col];
    part[grp][col] = acc;
    __syncthreads();
    const int j = threadIdx.x;
    if (j >= kCameraGrad) return;
    int term = -1;                        // the index into a block row, or -1: a slot the render does not read
    if (j < 16) { const int c = j >> 2, r = j & 3; term = r < 3 ? 3 * c + r : -1; }
    else if (j < 32) { const int c = (j - 16) >> 2, r = j & 3; term = r == 2 ? -1 : 12 + 3 * c + (r == 3 ? 2 : r); }
    else term = 24 + (j - 32);
    float val = 0.0f;
    if (term >= 0) {
        double t = 0.0;
#pragma unroll
        for (int g = 0; g < kFinishGroups; ++g) t += part[g][term];
        val = (float)t;
    }
    out[j] = accumulate ? out[j] + val : val;
}

}  // namespace

extern "C" size_t syn3r_raster_backward_workspace_bytes(int N) {
    return N > 0 ? align256((size_t)N * kGradSlots * sizeof(float)) : 0;
}

// ... plus one row of kPoseRow floats per block of k_preprocess_bwd, behind the gradient records
extern "C" size_t syn3r_raster_backward_cam_workspace_bytes(int N) {
    return N > 0 ? syn3r_raster_backward_workspace_bytes(N) + align256((size_t)ceil_div(N, 256) * kPoseRow * sizeof(float)) : 0;
}

// the three upstream gradients (depth, alpha: may be null) and the seven gradient outputs (confidence: may be null)
struct RasterGrads {
    const float *dL_dcolor, *dL_ddepth, *dL_dalpha;
    float *dL_dmeans3D, *dL_dscales, *dL_drotations, *dL_dopacities, *dL_dshs, *dL_dmeans2D, *dL_dconfidence;
    float* dL_dmeans2D_abs = nullptr;   // [N,2], syn3r_raster_backward_abs alone; null: the backward of the other entries
    float* dL_dcamera = nullptr;        // [35], syn3r_raster_backward_cam alone; null: no POSE instance, no finishing launch
    int accumulate = 0;                 // dL_dcamera: add to what the buffer holds
};

static int raster_backward(const RasterScene& s, long long P, const float* bg, const int* radii, void* geom, size_t geom_bytes_,
                           const unsigned* point_list, void* image, size_t image_bytes_, const RasterGrads& d, void* workspace,
                           size_t workspace_bytes, void* stream_) {
    if (int rc = raster_check_scene("raster_backward", s)) return rc;
    const int N = s.N, H = s.H, W = s.W;
    SYN3R_REQUIRE(P >= 0, "raster_backward: bad sizes P=%lld", P);
    SYN3R_REQUIRE(bg && radii, "raster_backward: null input");
    SYN3R_REQUIRE(d.dL_dcolor && d.dL_dmeans3D && d.dL_dscales && d.dL_drotations && d.dL_dopacities && d.dL_dshs && d.dL_dmeans2D,
                  "raster_backward: null gradient buffer");
    SYN3R_REQUIRE(P == 0 || point_list, "raster_backward: point list required");
    const size_t need = syn3r_raster_backward_workspace_bytes(N);          // the gradient records (the memset below)
    const size_t need_all = d.dL_dcamera ? syn3r_raster_backward_cam_workspace_bytes(N) : need;
    if (!geom || geom_bytes_ < geom_bytes(N) || !image || image_bytes_ < image_bytes(H, W) || !workspace ||
        workspace_bytes < need_all) {
        set_error("raster_backward: state/workspace buffer too small");
        return SYN3R_E_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    GeomState g = carve_geom(geom, N);
    ImageState im = carve_image(image, H, W);
    Camera cam;
    raster_fill_camera(cam, s.viewmatrix, s.projmatrix, s.campos, s.tanfovx, s.tanfovy, H, W);
    float* grad_rec = (float*)workspace;
    float* pose_rows = d.dL_dcamera ? (float*)((char*)workspace + need) : nullptr;   // every block writes its whole row: no memset
    int rc = check_hip(hipMemsetAsync(grad_rec, 0, need, stream), "memset grads");
    if (rc) return rc;
    const unsigned tiles = (unsigned)(cam.grid_x * cam.grid_y);
    const unsigned* tile_order = raster_tiles_ordered(N, cam.grid_x, cam.grid_y) ? im.tile_order : nullptr;
    // all four instances keep the one trace name: the benchmark's per-kernel tables are keyed by it.  Without a depth gradient (a
    // colour-only loss) slot G_DEPTH keeps the memset's zero, without dL_dmeans2D_abs slots G_AMX and G_AMY do.
    if (P > 0)
        with_bools([&](auto depth, auto abs) {
            SYN3R_LAUNCH_NAMED("k_render_bwd", (k_render_bwd<decltype(depth)::value, decltype(abs)::value>), dim3(tiles),
                               dim3(kBwdThreads), 0, stream, H, W, cam.grid_x, cam.grid_y, im.ranges, point_list, g.splats, bg[0], bg[1],
                               bg[2], im.n_contrib, im.final_T, d.dL_dcolor, d.dL_ddepth, d.dL_dalpha, grad_rec, tile_order);
        }, d.dL_ddepth != nullptr, d.dL_dmeans2D_abs != nullptr);
    // the trace name says `staged` alone, as before the anti-aliased and filtered instances existed (the benchmark's tables again)
    const bool staged = s.sh_coeffs == 16 && ((((uintptr_t)s.shs) | ((uintptr_t)d.dL_dshs)) & 15) == 0;
    with_bools([&](auto st, auto aa, auto f3d) {
        SYN3R_LAUNCH_NAMED(staged ? "k_preprocess_bwd<true>" : "k_preprocess_bwd<false>",
                           (k_preprocess_bwd<decltype(st)::value, decltype(aa)::value, decltype(f3d)::value, false>), dim3(ceil_div(N, 256)),
                           dim3(256), 0, stream, N, s.sh_degree, s.sh_coeffs, s.means3D, s.scales, s.rotations, s.opacities, s.shs,
                           s.confidence, s.scale_modifier, cam, radii, g, grad_rec, d.dL_dmeans3D, d.dL_dscales, d.dL_drotations,
                           d.dL_dopacities, d.dL_dshs, d.dL_dmeans2D, d.dL_dconfidence, s.raw, s.filter3d, nullptr);
    }, staged, (s.flags & SYN3R_RASTER_ANTIALIAS) != 0, s.filter3d != nullptr);
    if (d.dL_dcamera) {
        // the camera pass: the same kernel without its stores (see POSE), then the sum over its block rows
        with_bools([&](auto st, auto aa, auto f3d) {
            SYN3R_LAUNCH_NAMED("k_preprocess_bwd_pose",
                               (k_preprocess_bwd<decltype(st)::value, decltype(aa)::value, decltype(f3d)::value, true>), dim3(ceil_div(N, 256)),
                               dim3(256), 0, stream, N, s.sh_degree, s.sh_coeffs, s.means3D, s.scales, s.rotations, s.opacities, s.shs,
                               s.confidence, s.scale_modifier, cam, radii, g, grad_rec, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr, nullptr, s.raw, s.filter3d, pose_rows);
        }, s.sh_coeffs == 16 && (((uintptr_t)s.shs) & 15) == 0, (s.flags & SYN3R_RASTER_ANTIALIAS) != 0, s.filter3d != nullptr);
        SYN3R_LAUNCH(k_camera_grad_finish, dim3(1), dim3(kFinishGroups * kPoseRow), 0, stream, ceil_div(N, 256), pose_rows, d.dL_dcamera, d.accumulate);
    }
    if (d.dL_dmeans2D_abs)
        SYN3R_LAUNCH(k_abs_means2D, dim3(ceil_div(N, 256)), dim3(256), 0, stream, N, 0.5f * (float)W, 0.5f * (float)H, radii, g.splats,
                     grad_rec, d.dL_dmeans2D_abs);
    SYN3R_LAUNCH_CHECK("raster_backward launch");
    return SYN3R_OK;
}

extern "C" int syn3r_raster_backward(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                                     const float* scales, const float* rotations, const float* opacities,
                                     const float* shs, const float* confidence, float scale_modifier,
                                     const float* viewmatrix, const float* projmatrix, const float* campos,
                                     float tanfovx, float tanfovy, int H, int W, const float* bg, const int* radii,
                                     void* geom, size_t geom_bytes_, const unsigned* point_list, void* image,
                                     size_t image_bytes_, const float* dL_dcolor, const float* dL_ddepth,
                                     const float* dL_dalpha, float* dL_dmeans3D, float* dL_dscales,
                                     float* dL_drotations, float* dL_dopacities, float* dL_dshs, float* dL_dmeans2D,
                                     float* dL_dconfidence, void* workspace, size_t workspace_bytes, void* stream_) {
    return raster_backward(raster_scene(N, sh_degree, sh_coeffs, means3D, scales, rotations, opacities, shs, confidence,
                                        scale_modifier, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, 0, 0, nullptr),
                           P, bg, radii, geom, geom_bytes_, point_list, image, image_bytes_,
                           RasterGrads{dL_dcolor, dL_ddepth, dL_dalpha, dL_dmeans3D, dL_dscales, dL_drotations, dL_dopacities,
                                       dL_dshs, dL_dmeans2D, dL_dconfidence},
                           workspace, workspace_bytes, stream_);
}

extern "C" int syn3r_raster_backward_raw(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                                         const float* log_scales, const float* raw_rotations, const float* opacity_logits,
                                         const float* shs, const float* confidence, float scale_modifier,
                                         const float* viewmatrix, const float* projmatrix, const float* campos,
                                         float tanfovx, float tanfovy, int H, int W, const float* bg, const int* radii,
                                         void* geom, size_t geom_bytes_, const unsigned* point_list, void* image,
                                         size_t image_bytes_, const float* dL_dcolor, const float* dL_ddepth,
                                         const float* dL_dalpha, float* dL_dmeans3D, float* dL_dlog_scales,
                                         float* dL_draw_rotations, float* dL_dopacity_logits, float* dL_dshs, float* dL_dmeans2D,
                                         float* dL_dconfidence, void* workspace, size_t workspace_bytes, void* stream_) {
    return raster_backward(raster_scene(N, sh_degree, sh_coeffs, means3D, log_scales, raw_rotations, opacity_logits, shs, confidence,
                                        scale_modifier, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, 1, 0, nullptr),
                           P, bg, radii, geom, geom_bytes_, point_list, image, image_bytes_,
                           RasterGrads{dL_dcolor, dL_ddepth, dL_dalpha, dL_dmeans3D, dL_dlog_scales, dL_draw_rotations,
                                       dL_dopacity_logits, dL_dshs, dL_dmeans2D, dL_dconfidence},
                           workspace, workspace_bytes, stream_);
}

extern "C" int syn3r_raster_backward_ex(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                                        const float* scales, const float* rotations, const float* opacities,
                                        const float* shs, const float* confidence, float scale_modifier,
                                        const float* viewmatrix, const float* projmatrix, const float* campos,
                                        float tanfovx, float tanfovy, int H, int W, const float* bg, const int* radii,
                                        void* geom, size_t geom_bytes_, const unsigned* point_list, void* image,
                                        size_t image_bytes_, const float* dL_dcolor, const float* dL_ddepth,
                                        const float* dL_dalpha, float* dL_dmeans3D, float* dL_dscales,
                                        float* dL_drotations, float* dL_dopacities, float* dL_dshs, float* dL_dmeans2D,
                                        float* dL_dconfidence, void* workspace, size_t workspace_bytes, int raw, int flags,
                                        void* stream_) {
    return raster_backward(raster_scene(N, sh_degree, sh_coeffs, means3D, scales, rotations, opacities, shs, confidence,
                                        scale_modifier, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, raw, flags, nullptr),
                           P, bg, radii, geom, geom_bytes_, point_list, image, image_bytes_,
                           RasterGrads{dL_dcolor, dL_ddepth, dL_dalpha, dL_dmeans3D, dL_dscales, dL_drotations, dL_dopacities,
                                       dL_dshs, dL_dmeans2D, dL_dconfidence},
                           workspace, workspace_bytes, stream_);
}

extern "C" int syn3r_raster_backward_f3d(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                                         const float* scales, const float* rotations, const float* opacities,
                                         const float* shs, const float* confidence, float scale_modifier,
                                         const float* viewmatrix, const float* projmatrix, const float* campos,
                                         float tanfovx, float tanfovy, int H, int W, const float* bg, const int* radii,
                                         void* geom, size_t geom_bytes_, const unsigned* point_list, void* image,
                                         size_t image_bytes_, const float* dL_dcolor, const float* dL_ddepth,
                                         const float* dL_dalpha, float* dL_dmeans3D, float* dL_dscales,
                                         float* dL_drotations, float* dL_dopacities, float* dL_dshs, float* dL_dmeans2D,
                                         float* dL_dconfidence, void* workspace, size_t workspace_bytes, int raw, int flags,
                                         const float* filter3d, void* stream_) {
    return raster_backward(raster_scene(N, sh_degree, sh_coeffs, means3D, scales, rotations, opacities, shs, confidence,
                                        scale_modifier, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, raw, flags, filter3d),
                           P, bg, radii, geom, geom_bytes_, point_list, image, image_bytes_,
                           RasterGrads{dL_dcolor, dL_ddepth, dL_dalpha, dL_dmeans3D, dL_dscales, dL_drotations, dL_dopacities,
                                       dL_dshs, dL_dmeans2D, dL_dconfidence},
                           workspace, workspace_bytes, stream_);
}

extern "C" int syn3r_raster_backward_abs(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                                         const float* scales, const float* rotations, const float* opacities,
                                         const float* shs, const float* confidence, float scale_modifier,
                                         const float* viewmatrix, const float* projmatrix, const float* campos,
                                         float tanfovx, float tanfovy, int H, int W, const float* bg, const int* radii,
                                         void* geom, size_t geom_bytes_, const unsigned* point_list, void* image,
                                         size_t image_bytes_, const float* dL_dcolor, const float* dL_ddepth,
                                         const float* dL_dalpha, float* dL_dmeans3D, float* dL_dscales,
                                         float* dL_drotations, float* dL_dopacities, float* dL_dshs, float* dL_dmeans2D,
                                         float* dL_dconfidence, void* workspace, size_t workspace_bytes, int raw, int flags,
                                         const float* filter3d, float* dL_dmeans2D_abs, void* stream_) {
    SYN3R_REQUIRE(!dL_dmeans2D_abs || ((uintptr_t)dL_dmeans2D_abs & 7) == 0, "raster_backward: dL_dmeans2D_abs must be 8-byte aligned");
    return raster_backward(raster_scene(N, sh_degree, sh_coeffs, means3D, scales, rotations, opacities, shs, confidence,
                                        scale_modifier, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, raw, flags, filter3d),
                           P, bg, radii, geom, geom_bytes_, point_list, image, image_bytes_,
                           RasterGrads{dL_dcolor, dL_ddepth, dL_dalpha, dL_dmeans3D, dL_dscales, dL_drotations, dL_dopacities,
                                       dL_dshs, dL_dmeans2D, dL_dconfidence, dL_dmeans2D_abs},
                           workspace, workspace_bytes, stream_);
}

extern "C" int syn3r_raster_backward_cam(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                                         const float* scales, const float* rotations, const float* opacities,
                                         const float* shs, const float* confidence, float scale_modifier,
                                         const float* viewmatrix, const float* projmatrix, const float* campos,
                                         float tanfovx, float tanfovy, int H, int W, const float* bg, const int* radii,
                                         void* geom, size_t geom_bytes_, const unsigned* point_list, void* image,
                                         size_t image_bytes_, const float* dL_dcolor, const float* dL_ddepth,
                                         const float* dL_dalpha, float* dL_dmeans3D, float* dL_dscales,
                                         float* dL_drotations, float* dL_dopacities, float* dL_dshs, float* dL_dmeans2D,
                                         float* dL_dconfidence, void* workspace, size_t workspace_bytes, int raw, int flags,
                                         const float* filter3d, float* dL_dmeans2D_abs, float* dL_dcamera, int accumulate,
                                         void* stream_) {
    SYN3R_REQUIRE(!dL_dmeans2D_abs || ((uintptr_t)dL_dmeans2D_abs & 7) == 0, "raster_backward: dL_dmeans2D_abs must be 8-byte aligned");
    SYN3R_REQUIRE(!dL_dcamera || ((uintptr_t)dL_dcamera & 3) == 0, "raster_backward: dL_dcamera must be 4-byte aligned");
    return raster_backward(raster_scene(N, sh_degree, sh_coeffs, means3D, scales, rotations, opacities, shs, confidence,
                                        scale_modifier, viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, raw, flags, filter3d),
                           P, bg, radii, geom, geom_bytes_, point_list, image, image_bytes_,
                           RasterGrads{dL_dcolor, dL_ddepth, dL_dalpha, dL_dmeans3D, dL_dscales, dL_drotations, dL_dopacities,
                                       dL_dshs, dL_dmeans2D, dL_dconfidence, dL_dmeans2D_abs, dL_dcamera, accumulate},
                           workspace, workspace_bytes, stream_);
}

#ifdef SYN3R_RASTER_STATS
extern "C" __attribute__((visibility("default"))) int syn3r_debug_bwd_stats(unsigned long long* out4, int reset) {
    int rc = (int)hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_bwd_stats), sizeof(unsigned long long) * 4);
    if (reset) { unsigned long long z[4] = {0, 0, 0, 0}; rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_bwd_stats), z, sizeof(z)); }
    return rc;
}
#endif
