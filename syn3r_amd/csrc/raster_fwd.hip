// Gaussian rasteriser, forward: projection (EWA) and the front-to-back alpha blend with colour / depth /
// alpha outputs and a per-Gaussian confidence factor; the tile binning between the two is raster_bin.hip.
//
// Replaces the reference's `gsTrainer.render_view(cam)` hot kernels (call sites
// model/diffusionGS.py:154,166); the CUDA source is an un-vendored submodule
// (SURVEY.md §8c), so this follows the published 3DGS algorithm — see
// raster_common.h.  PARITY UNPINNED against the CUDA build; pinned against
// oracle/raster_oracle.py.
//
// MI355X mapping: one 16x16 tile = one 128-thread workgroup = 2 wavefronts, a wavefront covers a 16 x 8 half with two
// pixels per lane on packed fp32 arithmetic (k_render below).  Sorted splats are staged through LDS in batches as 48-byte
// records (3 x 16-byte loads per lane, broadcast reads in the blend loop).  The per-tile lists come from a hierarchical
// filter of the Gaussians, not from a pair sort, and the blend kernels take the tiles longest list first
// ("Hierarchical binning" in raster_bin.hip).
#include "common.h"
#include "raster_common.h"

using namespace syn3r;

namespace syn3r {

size_t geom_bytes(int N) {
    size_t n = (size_t)N;
    size_t b = 256;                         // header
    b += align256(n * 4);                   // depths
    b += align256(n * 8);                   // means2D
    b += align256(n * 24);                  // cov3D
    b += align256(n * 16);                  // conic_opacity
    b += align256(n * 12);                  // rgb
    b += align256(n * 4);                   // clamped
    b += align256(n * 4);                   // tiles_touched
    b += align256(n * 4);                   // point_offsets
    b += align256(n * sizeof(Splat));       // splats
    b += 4 * align256(n * 4);               // depth keys / order, ping + pong
    b += align256(sort_scratch_bytes(n));   // argsort histograms
    b += scan_scratch_bytes(n);
    return b;
}

GeomState carve_geom(void* buf, int N) {
    size_t n = (size_t)N;
    char* p = (char*)buf;
    GeomState g;
    g.header = (unsigned*)p; p += 256;
    g.depths = (float*)p; p += align256(n * 4);
    g.means2D = (float*)p; p += align256(n * 8);
    g.cov3D = (float*)p; p += align256(n * 24);
    g.conic_opacity = (float*)p; p += align256(n * 16);
    g.rgb = (float*)p; p += align256(n * 12);
    g.clamped = (unsigned*)p; p += align256(n * 4);
    g.tiles_touched = (unsigned*)p; p += align256(n * 4);
    g.point_offsets = (unsigned*)p; p += align256(n * 4);
    g.splats = (Splat*)p; p += align256(n * sizeof(Splat));
    g.dkeys_a = (unsigned*)p; p += align256(n * 4);
    g.dkeys_b = (unsigned*)p; p += align256(n * 4);
    g.order_a = (unsigned*)p; p += align256(n * 4);
    g.order_b = (unsigned*)p; p += align256(n * 4);
    g.order = g.order_a;                    // 32 bits in 8-bit digits = 4 passes: the result is back in the ping buffer
    g.sort_scratch = p; p += align256(sort_scratch_bytes(n));
    g.scan_scratch = p;
    return g;
}

size_t image_bytes(int H, int W) {
    size_t tiles = (size_t)((W + kTileX - 1) / kTileX) * ((H + kTileY - 1) / kTileY);
    size_t px = (size_t)H * W;
    return align256(tiles * 8) + align256(px * 4) + align256(px * 4) + align256(tiles * 16) + align256((kBinCounters + kMaxSuperSlots) * 4) + align256(tiles * 4);
}

ImageState carve_image(void* buf, int H, int W) {
    size_t tiles = (size_t)((W + kTileX - 1) / kTileX) * ((H + kTileY - 1) / kTileY);
    size_t px = (size_t)H * W;
    char* p = (char*)buf;
    ImageState s;
    s.ranges = (uint2*)p; p += align256(tiles * 8);
    s.n_contrib = (unsigned*)p; p += align256(px * 4);
    s.final_T = (float*)p; p += align256(px * 4);
    s.tile_counts = (unsigned*)p; p += align256(tiles * 16);
    s.bin_counters = (unsigned*)p; p += align256((kBinCounters + kMaxSuperSlots) * 4);
    s.tile_order = (unsigned*)p;
    return s;
}


}  // namespace syn3r

namespace {

__device__ __forceinline__ float ndc2pix(float v, int S) { return ((v + 1.0f) * (float)S - 1.0f) * 0.5f; }

// view-dependent colour from spherical harmonics (degree D <= 3), +0.5, clamped at 0
__device__ float3 sh_to_rgb(int D, int M, float3 pos, const float* campos, const float* __restrict__ sh,
                            unsigned& clamped) {
    float3 dir = make_float3(pos.x - campos[0], pos.y - campos[1], pos.z - campos[2]);
    float inv = 1.0f / sqrtf(dir.x * dir.x + dir.y * dir.y + dir.z * dir.z);
    dir.x *= inv; dir.y *= inv; dir.z *= inv;
    auto c = [&](int k) { return make_float3(sh[3 * k], sh[3 * k + 1], sh[3 * k + 2]); };
    auto mad = [](float3& a, float s, float3 b) { a.x += s * b.x; a.y += s * b.y; a.z += s * b.z; };
    float3 res = make_float3(0, 0, 0);
    mad(res, SH_C0, c(0));
    if (D > 0) {
        float x = dir.x, y = dir.y, z = dir.z;
        mad(res, -SH_C1 * y, c(1));
        mad(res, SH_C1 * z, c(2));
        mad(res, -SH_C1 * x, c(3));
        if (D > 1) {
            float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            mad(res, SH_C2[0] * xy, c(4));
            mad(res, SH_C2[1] * yz, c(5));
            mad(res, SH_C2[2] * (2.0f * zz - xx - yy), c(6));
            mad(res, SH_C2[3] * xz, c(7));
            mad(res, SH_C2[4] * (xx - yy), c(8));
            if (D > 2) {
                mad(res, SH_C3[0] * y * (3.0f * xx - yy), c(9));
                mad(res, SH_C3[1] * xy * z, c(10));
                mad(res, SH_C3[2] * y * (4.0f * zz - xx - yy), c(11));
                mad(res, SH_C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy), c(12));
                mad(res, SH_C3[4] * x * (4.0f * zz - xx - yy), c(13));
                mad(res, SH_C3[5] * z * (xx - yy), c(14));
                mad(res, SH_C3[6] * x * (xx - 3.0f * yy), c(15));
            }
        }
    }
    res.x += 0.5f; res.y += 0.5f; res.z += 0.5f;
    clamped = (res.x < 0.0f ? 1u : 0u) | (res.y < 0.0f ? 2u : 0u) | (res.z < 0.0f ? 4u : 0u);
    return make_float3(fmaxf(res.x, 0.0f), fmaxf(res.y, 0.0f), fmaxf(res.z, 0.0f));
}

// Projection.  AA and F3D are explained at mip_rho, f3d_scales and mode_factors in raster_common.h.  What stays for the later stages:
// GeomState (cov3D of the possibly FILTERED Gaussian; conic_opacity[3] = the plain op, without confidence, rho or coef: the
// backward forms those again) and the blend's Splat record, whose opacity is the whole product.  F3D = false never reads `filter3d`.
template <bool AA, bool F3D>
__global__ void __launch_bounds__(256) k_preprocess(int N, int D, int M, const float* __restrict__ means3D,
                                                    const float* __restrict__ scales,
                                                    const float* __restrict__ rots,
                                                    const float* __restrict__ opacities,
                                                    const float* __restrict__ shs, const float* __restrict__ conf,
                                                    float scale_mod, Camera cam, int* __restrict__ radii,
                                                    GeomState g, int raw, const float* __restrict__ filter3d) {
    int i = blockIdx.x * 256 + threadIdx.x;
    // pair count (written by the scan that follows), overflow flag, clipped and exact totals: cleared whatever N is (N < 4 too)
    if (i < 4) g.header[i] = 0u;
    if (i >= N) return;
    radii[i] = 0;
    g.tiles_touched[i] = 0;
    g.dkeys_a[i] = 0xFFFFFFFFu;             // culled Gaussians sort behind every visible one
    float3 p = make_float3(means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]);
    float3 t = xf43(cam.view, p);
    if (t.z <= kNearClip) return;
    float4 ph = xf44(cam.proj, p);
    float pw = 1.0f / (ph.w + 0.0000001f);
    float ndcx = ph.x * pw, ndcy = ph.y * pw;

    // 3D covariance  Sigma = R S^2 R^T  (q = (r, x, y, z), not renormalised here)
    // raw (syn3r_raster_preprocess_raw): the tensors are the trainer's PARAMETERS (log-scales, unnormalised quaternions, opacity
    // logits) and the published activations are applied here, in k_activate's arithmetic (common.h: the same bits)
    float s0 = scales[3 * i], s1 = scales[3 * i + 1], s2 = scales[3 * i + 2];
    float4 q4 = make_float4(rots[4 * i], rots[4 * i + 1], rots[4 * i + 2], rots[4 * i + 3]);
    if (raw) {
        s0 = act_exp(s0); s1 = act_exp(s1); s2 = act_exp(s2);
        q4 = act_quat(q4, act_quat_inv_norm(q4));
    }
    float coef = 1.0f;
    if constexpr (F3D) {
        const F3dScales fs = f3d_scales(s0, s1, s2, filter3d[i]);
        s0 = fs.q0; s1 = fs.q1; s2 = fs.q2; coef = fs.coef;
    }
    float sx = scale_mod * s0, sy = scale_mod * s1, sz = scale_mod * s2;
    const Rot3 k = quat_rotation(q4);
    float m00 = k.R00 * sx, m01 = k.R01 * sy, m02 = k.R02 * sz;   // M = R S
    float m10 = k.R10 * sx, m11 = k.R11 * sy, m12 = k.R12 * sz;
    float m20 = k.R20 * sx, m21 = k.R21 * sy, m22 = k.R22 * sz;
    float c0 = m00 * m00 + m01 * m01 + m02 * m02;   // Sigma = M M^T
    float c1 = m00 * m10 + m01 * m11 + m02 * m12;
    float c2 = m00 * m20 + m01 * m21 + m02 * m22;
    float c3 = m10 * m10 + m11 * m11 + m12 * m12;
    float c4 = m10 * m20 + m11 * m21 + m12 * m22;
    float c5 = m20 * m20 + m21 * m21 + m22 * m22;
    float* cv = g.cov3D + 6 * (size_t)i;
    cv[0] = c0; cv[1] = c1; cv[2] = c2; cv[3] = c3; cv[4] = c4; cv[5] = c5;

    // EWA: cov2D = (J W) Sigma (J W)^T, W = rotation part of the view matrix
    const EwaRows w = ewa_rows(cam, t.x, t.y, t.z);
    const EwaCov e = ewa_cov(w, c0, c1, c2, c3, c4, c5);
    const float pxx = e.xx, pyy = e.yy;                                                       // before the dilation
    float cxx = pxx + kLowPass;
    float cxy = e.xy;
    float cyy = pyy + kLowPass;

    float det = cxx * cyy - cxy * cxy;
    if (det == 0.0f) return;
    float det_inv = 1.0f / det;
    float conx = cyy * det_inv, cony = -cxy * det_inv, conz = cxx * det_inv;
    float mid = 0.5f * (cxx + cyy);
    float sq = sqrtf(fmaxf(0.1f, mid * mid - det));
    float lambda1 = mid + sq, lambda2 = mid - sq;
    int radius = (int)ceilf(3.0f * sqrtf(fmaxf(lambda1, lambda2)));
    float px = ndc2pix(ndcx, cam.W), py = ndc2pix(ndcy, cam.H);
    int x0, y0, x1, y1;
    tile_rect(px, py, radius, cam.grid_x, cam.grid_y, x0, y0, x1, y1);
    int area = (x1 - x0) * (y1 - y0);
    if (area == 0) return;

    unsigned cl;
    float3 rgb = sh_to_rgb(D, M, p, cam.campos, shs + (size_t)i * M * 3, cl);
    float op = raw ? act_sigmoid(opacities[i]) : opacities[i];
    float cf = conf ? conf[i] : 1.0f;
    const float rho = AA ? mip_rho(mip_ratio(pxx, cxy, pyy)) : 1.0f;
    const float blend_op = mode_factors(op, coef, rho) * cf;
    g.depths[i] = t.z;
    g.dkeys_a[i] = __float_as_uint(t.z);    // t.z > kNearClip > 0: the bit pattern orders like the float
    radii[i] = radius;
    g.means2D[2 * (size_t)i] = px;
    g.means2D[2 * (size_t)i + 1] = py;
    float* co = g.conic_opacity + 4 * (size_t)i;
    co[0] = conx; co[1] = cony; co[2] = conz; co[3] = op;
    g.rgb[3 * (size_t)i] = rgb.x; g.rgb[3 * (size_t)i + 1] = rgb.y; g.rgb[3 * (size_t)i + 2] = rgb.z;
    g.clamped[i] = cl;
    g.tiles_touched[i] = (unsigned)area;
    Splat s;
    s.x = px; s.y = py; s.cxx = conx; s.cxy = cony; s.cyy = conz; s.opacity = blend_op;
    s.r = rgb.x; s.g = rgb.y; s.b = rgb.z; s.depth = t.z; s.pad0 = 0.f; s.pad1 = 0.f;
    g.splats[i] = s;
}

// Two pixels per lane (see k_render_bwd in raster_bwd.hip): a 16 x 16 tile is a block of TWO wavefronts, wavefront w
// owns the 16 x 8 half (rows 8w .. 8w+7) and lane l the pixels (l & 15, 8w + (l >> 4)) and (.., + 4).  The
// quadratic form, the exponent argument, the weights and the colour / depth accumulation are float2 arithmetic
// (v_pk_fma_f32 / v_pk_mul_f32: two pixels per VALU issue); exp, min and the compares stay one per pixel.
// Bound by vector issue like the backward: a visit is 37 vector instructions (40 until round 8: the exponentials' log2(e) multiply
// is one packed instruction, and the transmittance goes down by the blend weight, T -= alpha T, instead of T (1 - alpha) behind
// two selects: the same value up to its last bit).
constexpr int kFwdThreads = kBlendThreads;
#ifdef SYN3R_RASTER_STATS
__device__ unsigned long long g_fwd_stats[4];
#endif

__global__ void __launch_bounds__(kFwdThreads) k_render(int H, int W, int gx, int gy, const uint2* __restrict__ ranges,
                                                        const unsigned* __restrict__ point_list,
                                                        const Splat* __restrict__ splats, float bg0, float bg1,
                                                        float bg2, unsigned* __restrict__ n_contrib,
                                                        float* __restrict__ final_T, float* __restrict__ out_color,
                                                        float* __restrict__ out_depth, float* __restrict__ out_alpha,
                                                        const unsigned* __restrict__ tile_order) {
    __shared__ float4 sm[kFwdThreads * 3];
    const unsigned tile = tile_order ? tile_order[blockIdx.x] : xcd_remap(blockIdx.x, (unsigned)(gx * gy));
    const int wq = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const BlendFrame f = blend_frame(tile, wq, lane, H, W, gx);
    const uint2 range = ranges[tile];
    const int total = (int)(range.y - range.x);
    const int rounds = (total + kFwdThreads - 1) / kFwdThreads;

    bool done0 = !f.in0, done1 = !f.in1;
    f2 T = (f2){1.0f, 1.0f}, Cr = (f2){0.f, 0.f}, Cg = Cr, Cb = Cr, Dp = Cr;
    unsigned last0 = 0, last1 = 0;
    int todo = total;
    const BlendHalf hf = blend_half(tile, wq, gx);
    // The records of round rd + 1 are requested (list entry, then the 48-byte record: two dependent global loads)
    // BEFORE round rd is blended and land in registers meanwhile: the gather latency is off the critical path.
    float4 n0, n1, n2;
    bool have = false;
    auto fetch = [&](int rd) {
        const int idx = rd * kFwdThreads + threadIdx.x;
        have = idx < total;
        if (have) {
            const float4* src = (const float4*)(splats + point_list[range.x + idx]);
            n0 = src[0]; n1 = src[1]; n2 = src[2];
        }
    };
    fetch(0);
    for (int rd = 0; rd < rounds; ++rd, todo -= kFwdThreads) {
        if (__syncthreads_count(done0 && done1) == kFwdThreads) break;
        if (have) stage_splat(sm, threadIdx.x, n0, n1, n2);
        fetch(rd + 1);
        __syncthreads();
        const int cnt = min(kFwdThreads, todo);
        // Visit list: each lane tests ONE staged splat against the wavefront's 16 x 8 half (splat_reaches_rect); the
        // ballot is the list, walked in order with scalar bit operations.  Most (wavefront, splat) visits of the
        // 3-sigma tile lists never reach alpha >= 1/255 on the half and are skipped for the price of one lane-test
        // instead of a 128-pixel evaluation.
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            if (__ballot(!(done0 && done1)) == 0ull) break;
            bool hit = false;
            if (c0 + lane < cnt) {
                const float4 a = sm[(c0 + lane) * 3], b = sm[(c0 + lane) * 3 + 1];
                hit = splat_reaches_rect(a.x, a.y, a.z, a.w, b.x, b.y, hf.sx0, hf.sx1, hf.sy0, hf.sy1);
            }
            unsigned long long m = __ballot(hit);
            RASTER_STAT(g_fwd_stats, 0, min(64, cnt - c0));
            RASTER_STAT(g_fwd_stats, 1, __popcll(m));
            while (m) {
                const int j = c0 + (int)__builtin_ctzll(m);
                m &= m - 1;
                const float4 a = sm[j * 3], b = sm[j * 3 + 1], c = sm[j * 3 + 2];
                const BlendEval e = blend_eval(a, b, f);
                const f2 power = e.power, araw = b.y * e.G;
                const float al0 = fminf(kAlphaMax, araw.x), al1 = fminf(kAlphaMax, araw.y);
                const f2 w_raw = (f2){al0, al1} * T;      // the weight if the pixel takes the splat; T - w is T (1 - alpha)
                const f2 test_T = T - w_raw;
                const bool c0_ = !done0 && power.x <= 0.0f && al0 >= kAlphaMin;
                const bool c1_ = !done1 && power.y <= 0.0f && al1 >= kAlphaMin;
                if (c0_ && test_T.x < kTransmittanceMin) done0 = true;
                if (c1_ && test_T.y < kTransmittanceMin) done1 = true;
                const bool t0 = c0_ && !done0, t1 = c1_ && !done1;
#ifdef SYN3R_RASTER_STATS
                { unsigned long long b0 = __ballot(t0), b1 = __ballot(t1); RASTER_STAT(g_fwd_stats, 2, (b0 | b1) != 0ull); RASTER_STAT(g_fwd_stats, 3, __popcll(b0) + __popcll(b1)); }
#endif
                // a pixel that does not take the splat adds a zero weight and keeps its transmittance: branch-free
                const f2 w = (f2){t0 ? w_raw.x : 0.0f, t1 ? w_raw.y : 0.0f};
                Cr += b.z * w; Cg += b.w * w; Cb += c.x * w; Dp += c.y * w;
                T -= w;
                const unsigned here = (unsigned)(rd * kFwdThreads + j + 1);
                last0 = t0 ? here : last0;
                last1 = t1 ? here : last1;
            }
        }
    }
    const size_t hw = (size_t)H * W;
    if (f.in0) {
        const size_t pix = (size_t)f.py0 * W + f.px;
        final_T[pix] = T.x;
        n_contrib[pix] = last0;
        out_color[pix] = Cr.x + T.x * bg0;
        out_color[hw + pix] = Cg.x + T.x * bg1;
        out_color[2 * hw + pix] = Cb.x + T.x * bg2;
        out_depth[pix] = Dp.x;
        out_alpha[pix] = 1.0f - T.x;
    }
    if (f.in1) {
        const size_t pix = (size_t)f.py1 * W + f.px;
        final_T[pix] = T.y;
        n_contrib[pix] = last1;
        out_color[pix] = Cr.y + T.y * bg0;
        out_color[hw + pix] = Cg.y + T.y * bg1;
        out_color[2 * hw + pix] = Cb.y + T.y * bg2;
        out_depth[pix] = Dp.y;
        out_alpha[pix] = 1.0f - T.y;
    }
}

}  // namespace

namespace syn3r {
void raster_fill_camera(Camera& cam, const float* view, const float* proj, const float* campos, float tanfovx,
                        float tanfovy, int H, int W) {
    for (int i = 0; i < 16; ++i) { cam.view[i] = view[i]; cam.proj[i] = proj[i]; }
    for (int i = 0; i < 3; ++i) cam.campos[i] = campos[i];
    cam.tanfovx = tanfovx; cam.tanfovy = tanfovy;
    cam.focal_x = W / (2.0f * tanfovx);
    cam.focal_y = H / (2.0f * tanfovy);
    cam.H = H; cam.W = W;
    cam.grid_x = (W + kTileX - 1) / kTileX;
    cam.grid_y = (H + kTileY - 1) / kTileY;
}
}  // namespace syn3r

extern "C" size_t syn3r_raster_geom_bytes(int N) { return SYN3R_DIM_OK(N) ? geom_bytes(N) : 0; }
extern "C" size_t syn3r_raster_image_bytes(int H, int W) { return (SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W)) ? image_bytes(H, W) : 0; }
extern "C" size_t syn3r_raster_binning_bytes(long long P) { return P >= 0 ? binning_bytes(P) : 0; }

namespace syn3r {
int raster_check_scene(const char* who, const RasterScene& s) {
    SYN3R_REQUIRE(s.raw == 0 || s.raw == 1, "%s: raw must be 0 or 1, got %d", who, s.raw);
    SYN3R_REQUIRE((s.flags & ~SYN3R_RASTER_ANTIALIAS) == 0, "%s: unknown flag bits 0x%x", who,
                  (unsigned)s.flags & ~(unsigned)SYN3R_RASTER_ANTIALIAS);
    SYN3R_REQUIRE(SYN3R_DIM_OK(s.N) && SYN3R_SIDE_OK(s.H) && SYN3R_SIDE_OK(s.W), "%s: bad sizes N=%d H=%d W=%d", who, s.N, s.H, s.W);
    SYN3R_REQUIRE(s.sh_degree >= 0 && s.sh_degree <= 3, "%s: sh_degree %d not in 0..3", who, s.sh_degree);
    SYN3R_REQUIRE(s.sh_coeffs >= (s.sh_degree + 1) * (s.sh_degree + 1) && s.sh_coeffs <= 1024,
                  "%s: sh_degree %d needs >= %d coefficients (<= 1024), got %d", who, s.sh_degree, (s.sh_degree + 1) * (s.sh_degree + 1),
                  s.sh_coeffs);
    SYN3R_REQUIRE(s.means3D && s.scales && s.rotations && s.opacities && s.shs && s.viewmatrix && s.projmatrix && s.campos,
                  "%s: null scene argument", who);
    SYN3R_REQUIRE(s.tanfovx > 0 && s.tanfovy > 0, "%s: bad field of view", who);
    return SYN3R_OK;
}
}  // namespace syn3r

static int raster_preprocess(const RasterScene& s, int* radii, void* geom, size_t geom_bytes_, long long* num_rendered_host,
                             void* stream_) {
    if (int rc = raster_check_scene("raster_preprocess", s)) return rc;
    SYN3R_REQUIRE(radii, "raster_preprocess: null argument");
    const int N = s.N;
    if (!geom || geom_bytes_ < geom_bytes(N)) {
        set_error("raster_preprocess: geometry buffer %zu < %zu", geom_bytes_, geom_bytes(N));
        return SYN3R_E_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    GeomState g = carve_geom(geom, N);
    Camera cam;
    raster_fill_camera(cam, s.viewmatrix, s.projmatrix, s.campos, s.tanfovx, s.tanfovy, s.H, s.W);
    // every instance keeps the one trace name: the benchmark's per-kernel tables are keyed by it
    with_bools([&](auto aa, auto f3d) {
        SYN3R_LAUNCH_NAMED("k_preprocess", (k_preprocess<decltype(aa)::value, decltype(f3d)::value>), dim3(ceil_div(N, 256)),
                           dim3(256), 0, stream, N, s.sh_degree, s.sh_coeffs, s.means3D, s.scales, s.rotations, s.opacities, s.shs,
                           s.confidence, s.scale_modifier, cam, radii, g, s.raw, s.filter3d);
    }, (s.flags & SYN3R_RASTER_ANTIALIAS) != 0, s.filter3d != nullptr);
    int rc = raster_bin_prepare(g, N, cam.grid_x, cam.grid_y, num_rendered_host != nullptr, stream);
    if (rc) return rc;
    SYN3R_LAUNCH_CHECK("raster_preprocess launch");
    if (num_rendered_host) {
        unsigned total = 0;
        rc = check_hip(hipMemcpyAsync(&total, g.header, 4, hipMemcpyDeviceToHost, stream), "num_rendered copy");
        if (rc) return rc;
        rc = check_hip(hipStreamSynchronize(stream), "num_rendered sync");
        if (rc) return rc;
        *num_rendered_host = (long long)total;
    }
    return SYN3R_OK;
}

extern "C" int syn3r_raster_preprocess(int N, int sh_degree, int sh_coeffs, const float* means3D,
                                       const float* scales, const float* rotations, const float* opacities,
                                       const float* shs, const float* confidence, float scale_modifier,
                                       const float* viewmatrix, const float* projmatrix, const float* campos,
                                       float tanfovx, float tanfovy, int H, int W, int* radii, void* geom,
                                       size_t geom_bytes_, long long* num_rendered_host, void* stream_) {
    return raster_preprocess(raster_scene(N, sh_degree, sh_coeffs, means3D, scales, rotations, opacities, shs, confidence, scale_modifier,
                                          viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, 0, 0, nullptr),
                             radii, geom, geom_bytes_, num_rendered_host, stream_);
}

extern "C" int syn3r_raster_preprocess_raw(int N, int sh_degree, int sh_coeffs, const float* means3D,
                                           const float* log_scales, const float* raw_rotations, const float* opacity_logits,
                                           const float* shs, const float* confidence, float scale_modifier,
                                           const float* viewmatrix, const float* projmatrix, const float* campos,
                                           float tanfovx, float tanfovy, int H, int W, int* radii, void* geom,
                                           size_t geom_bytes_, long long* num_rendered_host, void* stream_) {
    return raster_preprocess(raster_scene(N, sh_degree, sh_coeffs, means3D, log_scales, raw_rotations, opacity_logits, shs, confidence, scale_modifier,
                                          viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, 1, 0, nullptr),
                             radii, geom, geom_bytes_, num_rendered_host, stream_);
}

extern "C" int syn3r_raster_preprocess_ex(int N, int sh_degree, int sh_coeffs, const float* means3D, const float* scales,
                                          const float* rotations, const float* opacities, const float* shs,
                                          const float* confidence, float scale_modifier, const float* viewmatrix,
                                          const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H,
                                          int W, int* radii, void* geom, size_t geom_bytes_, long long* num_rendered_host,
                                          int raw, int flags, void* stream_) {
    return raster_preprocess(raster_scene(N, sh_degree, sh_coeffs, means3D, scales, rotations, opacities, shs, confidence, scale_modifier,
                                          viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, raw, flags, nullptr),
                             radii, geom, geom_bytes_, num_rendered_host, stream_);
}

extern "C" int syn3r_raster_preprocess_f3d(int N, int sh_degree, int sh_coeffs, const float* means3D, const float* scales,
                                           const float* rotations, const float* opacities, const float* shs,
                                           const float* confidence, float scale_modifier, const float* viewmatrix,
                                           const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H,
                                           int W, int* radii, void* geom, size_t geom_bytes_, long long* num_rendered_host,
                                           int raw, int flags, const float* filter3d, void* stream_) {
    return raster_preprocess(raster_scene(N, sh_degree, sh_coeffs, means3D, scales, rotations, opacities, shs, confidence, scale_modifier,
                                          viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, raw, flags, filter3d),
                             radii, geom, geom_bytes_, num_rendered_host, stream_);
}

extern "C" int syn3r_raster_render(int N, int H, int W, const float* bg, const int* radii, void* geom,
                                   size_t geom_bytes_, void* binning, size_t binning_bytes_, void* image,
                                   size_t image_bytes_, long long P, float* out_color, float* out_depth,
                                   float* out_alpha, unsigned** point_list_out, void* stream_) {
    SYN3R_REQUIRE(N > 0 && H > 0 && W > 0 && P >= 0 && P < (1ll << 31), "raster_render: bad sizes N=%d H=%d W=%d P=%lld",
                  N, H, W, P);
    SYN3R_REQUIRE(bg && radii && out_color && out_depth && out_alpha, "raster_render: null argument");
    if (!geom || geom_bytes_ < geom_bytes(N) || !image || image_bytes_ < image_bytes(H, W) || !binning ||
        binning_bytes_ < binning_bytes(P)) {
        set_error("raster_render: state buffer too small (geom %zu/%zu image %zu/%zu binning %zu/%zu)", geom_bytes_,
                  geom_bytes(N), image_bytes_, image_bytes(H, W), binning_bytes_, binning_bytes(P));
        return SYN3R_E_WORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    GeomState g = carve_geom(geom, N);
    ImageState im = carve_image(image, H, W);
    BinningState bn = carve_binning(binning, P);
    const int gx = (W + kTileX - 1) / kTileX, gy = (H + kTileY - 1) / kTileY;
    const size_t tiles = (size_t)gx * gy;
    unsigned* point_list = nullptr;
    const unsigned* tile_order = nullptr;
    if (int rc = raster_bin_lists(g, im, bn, radii, N, gx, gy, P, stream, &point_list, &tile_order)) return rc;
    SYN3R_LAUNCH(k_render, dim3((unsigned)tiles), dim3(kFwdThreads), 0, stream, H, W, gx, gy, im.ranges, point_list,
                       g.splats, bg[0], bg[1], bg[2], im.n_contrib, im.final_T, out_color, out_depth, out_alpha, tile_order);
    SYN3R_LAUNCH_CHECK("raster_render launch");
    if (point_list_out) *point_list_out = point_list;
    return SYN3R_OK;
}

#ifdef SYN3R_RASTER_STATS
extern "C" __attribute__((visibility("default"))) int syn3r_debug_fwd_stats(unsigned long long* out4, int reset) {
    int rc = (int)hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_fwd_stats), sizeof(unsigned long long) * 4);
    if (reset) { unsigned long long z[4] = {0, 0, 0, 0}; rc |= (int)hipMemcpyToSymbol(HIP_SYMBOL(g_fwd_stats), z, sizeof(z)); }
    return rc;
}
#endif
