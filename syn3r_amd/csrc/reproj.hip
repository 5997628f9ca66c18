// Multi-view photometric reprojection term of the trainer (EXTENSION, include/syn3r_hip.h): Monodepth2's per-pixel minimum
// reprojection error (Godard et al., ICCV 2019) without its SSIM part and auto-mask, as the unsupervised-MVS and MVS-guided
// sparse-view 3DGS pipelines use it.  The depth rendered for a target view t carries each pixel into S posed input views; the colour
// found there is compared with the target's own.  Pixel convention of the rasteriser (ndc2pix, raster_fwd.hip): pixel index x sits
// at fx X/Z + (W-1)/2.  Per pixel p = (x, y), D the rendered depth, a the rendered alpha, all fp32:
//   z   = D / a                                              dead when !(a >= alpha_min) or !(D > 0)
//   r   = ((x - cx_t) / fx_t, (y - cy_t) / fy_t, 1)
//   A   = M_s r        X = z A + t_s        q = (fx_s X_x / X_z + cx_s, fy_s X_y / X_z + cy_s)
//   source s is valid when X_z >= 0.01, 0 <= q_x <= W-1 and 0 <= q_y <= H-1
//   e_s = (1/3) sum_c |I_s,c(q) - I_t,c(p)|, I_s(q) bilinear on the cell x0 = min(floor(q_x), W-2), y0 = min(floor(q_y), H-2)
//   e   = min over the valid s of e_s, the lowest s on a tie; no valid source: dead
//   loss = weight * sum_live e / max(N_live, 1)              N_live constant in the gradient
//   dL/dz = weight / N_live * (1/3) sum_c sgn(I_s,c(q) - I_t,c(p)) (dI_s,c/dq_x dq_x/dz + dI_s,c/dq_y dq_y/dz)   sgn(0) = 0
//   dq_x/dz = fx_s (A_x t_z - A_z t_x) / X_z^2     dq_y/dz = fy_s (A_y t_z - A_z t_y) / X_z^2     (cancellation-free: X = z A + t)
//   g_depth = dL/dz / a        g_alpha = -dL/dz z / a        dead pixels: 0 in both
// PROVENANCE: the minimum over sources and the L1 form are recalled from Monodepth2 (not available to check); alpha_min and the
// absence of SSIM and auto-mask are this project's choices: UNPINNED.
//
// Groups of four pixels, the grid rule, VEC and the order of the sums: plane_pass.h (blocks = min(ceil(H G / 256), 1024) of 256
// threads for both passes).
// k_reproj_stats: geometry, gathers, minimum and the UNSCALED per-pixel dL/dz (weight / N_live = 1).  Per source the 48 taps of a
//                 group (4 pixels x 4 corners x 3 channels) are unconditional loads at clamped cells (an invalid pixel reads cell
//                 (0, 0) and drops the values by a select), requested together before the first use (README round 6).  No LDS
//                 stage: neighbouring pixels map to neighbouring q, the taps hit the cache.  The source table (image pointer + 16
//                 floats per source) travels by value, as syn3r_adam_step_multi's pointer tables do.  It leaves, per pixel, 8
//                 bytes: the fp32 dL/dz (0 when dead) and a record word (e's fp32 bits with the two lowest mantissa bits replaced
//                 by the chosen source; 0xffffffff when dead), and ONE row per block (sum e, N_live, N on source 0, sum e on
//                 source 0): per-thread fp32 running sums left to right, then block_rows.
// k_reproj_final: one block: rp_combine (combine_rows), writes parts.
// k_reproj_grad:  elementwise over D, a and the dL/dz plane (no gathers): every block runs rp_combine, scales in fp64, one fp32
//                 rounding per output, writes or ADDS g_depth and g_alpha; block 0 writes parts when asked.
// No float atomics, no host read.  Built without fma contraction (build.py STRICT_FP).
#include "plane_pass.h"

using namespace syn3r;

namespace {

constexpr int kRpThreads = 256;
constexpr int kRpMaxBlocks = 1024;
static_assert(kRpThreads == kPassThreads && kRpMaxBlocks == kPassMaxBlocks, "block_rows / combine_rows: 256 threads, four rows per thread");
constexpr int kRpMaxSources = 4;
constexpr size_t kRpRowBytes = (size_t)kRpMaxBlocks * sizeof(float4);      // head of the workspace; the two planes follow
constexpr unsigned kRpDead = 0xffffffffu;

// per source: M (row-major 3 x 3), t, fx, fy, cx, cy
struct RpView { float m[9]; float t[3]; float fx, fy, cx, cy; };
struct RpTable { const float* img[kRpMaxSources]; RpView v[kRpMaxSources]; };
struct RpTarget { float fx, fy, cx, cy; };

__device__ __forceinline__ float rp_sign(float a, float b) { return a > b ? 1.0f : (a < b ? -1.0f : 0.0f); }
__device__ __forceinline__ bool rp_live(float d, float a, float alpha_min) { return a >= alpha_min && d > 0.0f; }

// what one pixel knows of one source before its taps arrive
struct RpGeo { float fx, fy, dqx, dqy; int cell; bool valid; };

__device__ __forceinline__ RpGeo rp_project(const RpView& v, float rx, float ry, float z, int H, int W) {
    const float Ax = (v.m[0] * rx + v.m[1] * ry) + v.m[2];
    const float Ay = (v.m[3] * rx + v.m[4] * ry) + v.m[5];
    const float Az = (v.m[6] * rx + v.m[7] * ry) + v.m[8];
    const float Xx = z * Ax + v.t[0], Xy = z * Ay + v.t[1], Xz = z * Az + v.t[2];
    const float qx = (v.fx * Xx) / Xz + v.cx, qy = (v.fy * Xy) / Xz + v.cy;
    RpGeo g;
    g.valid = Xz >= 0.01f && qx >= 0.0f && qx <= (float)(W - 1) && qy >= 0.0f && qy <= (float)(H - 1);
    const float sx = g.valid ? qx : 0.0f, sy = g.valid ? qy : 0.0f;         // (a NaN or far q never forms an index)
    int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
    x0 = x0 < W - 2 ? x0 : W - 2;
    y0 = y0 < H - 2 ? y0 : H - 2;
    g.fx = sx - (float)x0;
    g.fy = sy - (float)y0;
    g.cell = y0 * W + x0;
    const float iz2 = Xz * Xz;
    g.dqx = (v.fx * (Ax * v.t[2] - Az * v.t[0])) / iz2;
    g.dqy = (v.fy * (Ay * v.t[2] - Az * v.t[1])) / iz2;
    return g;
}

template <bool VEC>
__global__ void __launch_bounds__(kRpThreads) k_reproj_stats(const float* __restrict__ depth, const float* __restrict__ alpha,
                                                            const float* __restrict__ target, int H, int W, int G, int S,
                                                            const RpTable tab, const RpTarget tk, float alpha_min,
                                                            float4* __restrict__ rows, float* __restrict__ dz_plane,
                                                            unsigned* __restrict__ rec_plane) {
    const size_t plane = (size_t)H * (size_t)W;
    float se = 0.0f, sn = 0.0f, sn0 = 0.0f, se0 = 0.0f;
    plane_walk<kRpThreads>(H, G, [&](int y, int x0) {
        const float4 d4 = load4<VEC>(depth, y, x0, W), a4 = load4<VEC>(alpha, y, x0, W);
        float4 t4[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) t4[c] = load4<VEC>(target + c * plane, y, x0, W);
        const float ry = ((float)y - tk.cy) / tk.fy;
        float z[4], rx[4], best_e[4], best_g[4];
        int best_s[4];
        bool live[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d = row_get(d4, k), a = row_get(a4, k);
            live[k] = rp_live(d, a, alpha_min) && x0 + k < W;
            z[k] = live[k] ? d / a : 1.0f;
            rx[k] = ((float)(x0 + k) - tk.cx) / tk.fx;
            best_e[k] = 0.0f; best_g[k] = 0.0f; best_s[k] = -1;
        }
#pragma unroll 1
        for (int s = 0; s < S; ++s) {
            const RpView& v = tab.v[s];
            const float* __restrict__ img = tab.img[s];
            RpGeo g[4];
            float tap[4][3][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = rp_project(v, rx[k], ry, z[k], H, W);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float* p = img + c * plane + g[k].cell;
                    tap[k][c][0] = p[0]; tap[k][c][1] = p[1]; tap[k][c][2] = p[W]; tap[k][c][3] = p[W + 1];
                }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float fx = g[k].fx, fy = g[k].fy, gx1 = 1.0f - fx, gy1 = 1.0f - fy;
                float ad[3], gr[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float i00 = tap[k][c][0], i01 = tap[k][c][1], i10 = tap[k][c][2], i11 = tap[k][c][3];
                    const float val = gy1 * (gx1 * i00 + fx * i01) + fy * (gx1 * i10 + fx * i11);
                    const float dx = gy1 * (i01 - i00) + fy * (i11 - i10);
                    const float dy = gx1 * (i10 - i00) + fx * (i11 - i01);
                    const float tc = row_get(t4[c], k);
                    ad[c] = fabsf(val - tc);
                    gr[c] = rp_sign(val, tc) * (dx * g[k].dqx + dy * g[k].dqy);
                }
                const float e = ((ad[0] + ad[1]) + ad[2]) / 3.0f;
                const float dz = ((gr[0] + gr[1]) + gr[2]) / 3.0f;
                const bool take = live[k] && g[k].valid && (best_s[k] < 0 || e < best_e[k]);
                best_e[k] = take ? e : best_e[k];
                best_g[k] = take ? dz : best_g[k];
                best_s[k] = take ? s : best_s[k];
            }
        }
        float4 dz4;
        uint4 rec4;
        float gz[4];
        unsigned rc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool on = best_s[k] >= 0;
            gz[k] = on ? best_g[k] : 0.0f;
            rc[k] = on ? ((__float_as_uint(best_e[k]) & ~3u) | (unsigned)best_s[k]) : kRpDead;
            se += on ? best_e[k] : 0.0f;
            sn += on ? 1.0f : 0.0f;
            sn0 += best_s[k] == 0 ? 1.0f : 0.0f;
            se0 += best_s[k] == 0 ? best_e[k] : 0.0f;
        }
        dz4 = make_float4(gz[0], gz[1], gz[2], gz[3]);
        rec4 = make_uint4(rc[0], rc[1], rc[2], rc[3]);
        store4<VEC>(dz_plane, y, x0, W, dz4);
        store4<VEC>((float*)rec_plane, y, x0, W,
                       make_float4(__uint_as_float(rec4.x), __uint_as_float(rec4.y), __uint_as_float(rec4.z), __uint_as_float(rec4.w)));
    });
    if (block_rows(se, sn, sn0, se0)) rows[xcd_remap(blockIdx.x, gridDim.x)] = make_float4(se, sn, sn0, se0);
}

// what the combined rows give: sum e, N_live, N on source 0 (sum e on source 0 is kept in the rows for diagnostics)
struct RpCoef { double se, n, n0; };

__device__ RpCoef rp_combine(const float4* __restrict__ rows, int nrows) {
    RpCoef k;
    combine_rows(rows, nrows, k.se, k.n, k.n0);
    return k;
}

// parts = [loss, mean e over the live pixels, N_live / (H W), share of the live pixels on source 0]
__device__ __forceinline__ void rp_write_parts(const RpCoef& k, int H, int W, float weight, float* __restrict__ parts) {
    const double n1 = k.n > 1.0 ? k.n : 1.0, mean = k.se / n1;
    *(float4*)parts = make_float4((float)((double)weight * mean), (float)mean, (float)(k.n / ((double)H * (double)W)), (float)(k.n0 / n1));
}

__global__ void __launch_bounds__(kRpThreads) k_reproj_final(const float4* __restrict__ rows, int nrows, int H, int W, float weight,
                                                            float* __restrict__ parts) {
    const RpCoef k = rp_combine(rows, nrows);
    if (threadIdx.x == 0) rp_write_parts(k, H, W, weight, parts);
}

template <bool VEC, bool ACCD, bool ACCA>
__global__ void __launch_bounds__(kRpThreads) k_reproj_grad(const float* __restrict__ depth, const float* __restrict__ alpha, int H, int W,
                                                           int G, const float4* __restrict__ rows, int nrows,
                                                           const float* __restrict__ dz_plane, float weight, float alpha_min,
                                                           const float* __restrict__ go, float* __restrict__ grad_depth,
                                                           float* __restrict__ grad_alpha, float* __restrict__ parts) {
    const RpCoef k = rp_combine(rows, nrows);
    if (parts && blockIdx.x == 0 && threadIdx.x == 0) rp_write_parts(k, H, W, weight, parts);
    const double scale = (double)weight * (go ? (double)*go : 1.0) / (k.n > 1.0 ? k.n : 1.0);
    plane_walk<kRpThreads>(H, G, [&](int y, int x0) {
        const float4 d4 = load4<VEC>(depth, y, x0, W), a4 = load4<VEC>(alpha, y, x0, W), z4 = load4<VEC>(dz_plane, y, x0, W);
        float4 od = make_float4(0.f, 0.f, 0.f, 0.f), oa = od;
        if constexpr (ACCD) od = load4<VEC>(grad_depth, y, x0, W);
        if constexpr (ACCA) oa = load4<VEC>(grad_alpha, y, x0, W);
        float gd[4], ga[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = row_get(d4, i), a = row_get(a4, i);
            const bool live = rp_live(d, a, alpha_min);
            const double da = live ? (double)a : 1.0;
            const double g = scale * (double)row_get(z4, i);              // dL/dz (the plane holds 0 for a pixel without a source)
            gd[i] = live ? (float)(g / da) : 0.0f;
            ga[i] = live ? (float)(-(g * ((double)d / da)) / da) : 0.0f;
        }
        float4 vd = make_float4(gd[0], gd[1], gd[2], gd[3]), va = make_float4(ga[0], ga[1], ga[2], ga[3]);
        if constexpr (ACCD) { vd.x = od.x + vd.x; vd.y = od.y + vd.y; vd.z = od.z + vd.z; vd.w = od.w + vd.w; }
        if constexpr (ACCA) { va.x = oa.x + va.x; va.y = oa.y + va.y; va.z = oa.z + va.z; va.w = oa.w + va.w; }
        store4<VEC>(grad_depth, y, x0, W, vd);
        store4<VEC>(grad_alpha, y, x0, W, va);
    });
}

// blocks of both grids: a function of H and W alone
int rp_blocks(int H, int W) { return pass_blocks((long long)H * groups_per_row(W), kRpThreads, kRpMaxBlocks); }

bool rp_shape_ok(int H, int W, int S) { return SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W) && H >= 2 && W >= 2 && S >= 1 && S <= kRpMaxSources; }

float* rp_dz_plane(const void* ws) { return (float*)((char*)ws + kRpRowBytes); }
unsigned* rp_rec_plane(const void* ws, int H, int W) { return (unsigned*)(rp_dz_plane(ws) + (size_t)H * (size_t)W); }

// the checks every entry shares, all before any HIP call
int rp_check(const char* who, const float* depth, const float* alpha, int H, int W, int S, float weight, float alpha_min, const void* ws,
             size_t ws_bytes) {
    SYN3R_REQUIRE(rp_shape_ok(H, W, S), "%s: H=%d, W=%d must be in [2, 2^15] and S=%d in [1, %d]", who, H, W, S, kRpMaxSources);
    SYN3R_REQUIRE(depth && alpha && ws, "%s: null pointer", who);
    SYN3R_REQUIRE(finite_f32(weight) && finite_f32(alpha_min) && alpha_min > 0.0f, "%s: weight must be finite, alpha_min finite and > 0", who);
    return check_workspace(who, ws, ws_bytes, syn3r_photo_reproj_workspace_bytes(H, W, S), "syn3r_photo_reproj_workspace_bytes");
}

// the checks of an entry that runs the statistics pass; fills the table
int rp_check_stats(const char* who, const float* depth, const float* alpha, const float* target, const float* const* sources,
                   const float* views, const float* target_k, int H, int W, int S, const void* ws, size_t ws_bytes, RpTable& tab, RpTarget& tk) {
    SYN3R_REQUIRE(target && sources && views && target_k, "%s: null pointer", who);
    const size_t plane = (size_t)H * (size_t)W * sizeof(float);
    SYN3R_REQUIRE(!ranges_overlap(ws, ws_bytes, depth, plane) && !ranges_overlap(ws, ws_bytes, alpha, plane) &&
                  !ranges_overlap(ws, ws_bytes, target, 3 * plane), "%s: workspace aliases an input", who);
    for (int k = 0; k < 4; ++k) SYN3R_REQUIRE(finite_f32(target_k[k]), "%s: target intrinsics must be finite", who);
    SYN3R_REQUIRE(target_k[0] != 0.0f && target_k[1] != 0.0f, "%s: target focal lengths must not be 0", who);
    tk = RpTarget{target_k[0], target_k[1], target_k[2], target_k[3]};
    for (int s = 0; s < kRpMaxSources; ++s) {
        const int r = s < S ? s : 0;                      // (the unused entries repeat source 0: never read)
        if (s < S) {
            SYN3R_REQUIRE(sources[s], "%s: null image of source %d", who, s);
            SYN3R_REQUIRE(!ranges_overlap(ws, ws_bytes, sources[s], 3 * plane), "%s: workspace aliases source %d", who, s);
            for (int k = 0; k < 16; ++k) SYN3R_REQUIRE(finite_f32(views[16 * s + k]), "%s: view %d must be finite", who, s);
        }
        tab.img[s] = sources[r];
        const float* v = views + 16 * r;
        for (int k = 0; k < 9; ++k) tab.v[s].m[k] = v[k];
        for (int k = 0; k < 3; ++k) tab.v[s].t[k] = v[9 + k];
        tab.v[s].fx = v[12]; tab.v[s].fy = v[13]; tab.v[s].cx = v[14]; tab.v[s].cy = v[15];
    }
    return SYN3R_OK;
}

// the checks of an entry that writes the two gradients
int rp_check_grad(const char* who, const float* depth, const float* alpha, int H, int W, const void* ws, size_t ws_bytes,
                  const float* grad_depth, int acc_depth, const float* grad_alpha, int acc_alpha) {
    if (const int rc = check_grad_target(who, grad_depth, acc_depth, "accumulate_depth")) return rc;
    if (const int rc = check_grad_target(who, grad_alpha, acc_alpha, "accumulate_alpha")) return rc;
    const size_t bytes = (size_t)H * (size_t)W * sizeof(float);
    for (const float* g : {grad_depth, grad_alpha})
        SYN3R_REQUIRE(!ranges_overlap(g, bytes, depth, bytes) && !ranges_overlap(g, bytes, alpha, bytes) &&
                      !ranges_overlap(g, bytes, ws, ws_bytes), "%s: a gradient aliases an input or the workspace", who);
    SYN3R_REQUIRE(!ranges_overlap(grad_depth, bytes, grad_alpha, bytes), "%s: grad_depth and grad_alpha overlap", who);
    return SYN3R_OK;
}

void rp_stats(const float* depth, const float* alpha, const float* target, int H, int W, int S, const RpTable& tab, const RpTarget& tk,
              float alpha_min, void* ws, hipStream_t stream) {
    const dim3 grid((unsigned)rp_blocks(H, W));
    const int G = groups_per_row(W);
    // (the planes of the workspace are 16-byte aligned by construction: with W % 4 == 0 so is every group of them)
    with_bools([&](auto vec) {
        SYN3R_LAUNCH_NAMED("k_reproj_stats", k_reproj_stats<decltype(vec)::value>, grid, dim3(kRpThreads), 0, stream, depth, alpha, target, H, W,
                           G, S, tab, tk, alpha_min, (float4*)ws, rp_dz_plane(ws), rp_rec_plane(ws, H, W));
    }, W % 4 == 0 && aligned16(depth, alpha, target));
}

void rp_grad(const float* depth, const float* alpha, int H, int W, float weight, float alpha_min, const float* grad_loss, const void* ws,
             float* grad_depth, int acc_depth, float* grad_alpha, int acc_alpha, float* parts, hipStream_t stream) {
    const int nb = rp_blocks(H, W), G = groups_per_row(W);
    with_bools([&](auto vec, auto accd, auto acca) {
        SYN3R_LAUNCH_NAMED("k_reproj_grad", (k_reproj_grad<decltype(vec)::value, decltype(accd)::value, decltype(acca)::value>),
                           dim3((unsigned)nb), dim3(kRpThreads), 0, stream, depth, alpha, H, W, G, (const float4*)ws, nb,
                           (const float*)rp_dz_plane(ws), weight, alpha_min, grad_loss, grad_depth, grad_alpha, parts);
    }, W % 4 == 0 && aligned16(depth, alpha, grad_depth, grad_alpha), acc_depth != 0, acc_alpha != 0);
}

}  // namespace

extern "C" size_t syn3r_photo_reproj_workspace_bytes(int H, int W, int S) {
    if (!rp_shape_ok(H, W, S)) return 0;
    return ((kRpRowBytes + (size_t)H * (size_t)W * 8 + 255) / 256) * 256;
}

extern "C" int syn3r_photo_reproj_loss(const float* depth, const float* alpha, const float* target, const float* const* sources,
                                       const float* views, const float* target_k, int H, int W, int S, float weight, float alpha_min,
                                       float* parts, void* ws, size_t ws_bytes, void* stream_) {
    const char* who = "photo_reproj_loss";
    int rc = rp_check(who, depth, alpha, H, W, S, weight, alpha_min, ws, ws_bytes);
    if (rc) return rc;
    if ((rc = check_parts(who, parts))) return rc;
    RpTable tab{};
    RpTarget tk{};
    if ((rc = rp_check_stats(who, depth, alpha, target, sources, views, target_k, H, W, S, ws, ws_bytes, tab, tk))) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    rp_stats(depth, alpha, target, H, W, S, tab, tk, alpha_min, ws, stream);
    SYN3R_LAUNCH(k_reproj_final, dim3(1), dim3(kRpThreads), 0, stream, (const float4*)ws, rp_blocks(H, W), H, W, weight, parts);
    SYN3R_LAUNCH_CHECK("photo_reproj_loss launch");
    return SYN3R_OK;
}

extern "C" int syn3r_photo_reproj_loss_backward(const float* depth, const float* alpha, int H, int W, int S, float weight, float alpha_min,
                                                const float* grad_loss, const void* ws, size_t ws_bytes, float* grad_depth,
                                                int accumulate_depth, float* grad_alpha, int accumulate_alpha, void* stream_) {
    const char* who = "photo_reproj_loss_backward";
    int rc = rp_check(who, depth, alpha, H, W, S, weight, alpha_min, ws, ws_bytes);
    if (rc) return rc;
    if ((rc = rp_check_grad(who, depth, alpha, H, W, ws, ws_bytes, grad_depth, accumulate_depth, grad_alpha, accumulate_alpha))) return rc;
    rp_grad(depth, alpha, H, W, weight, alpha_min, grad_loss, ws, grad_depth, accumulate_depth, grad_alpha, accumulate_alpha, nullptr,
            (hipStream_t)stream_);
    SYN3R_LAUNCH_CHECK("photo_reproj_loss_backward launch");
    return SYN3R_OK;
}

extern "C" int syn3r_photo_reproj_loss_step(const float* depth, const float* alpha, const float* target, const float* const* sources,
                                            const float* views, const float* target_k, int H, int W, int S, float weight,
                                            float alpha_min, const float* grad_loss, float* parts, float* grad_depth,
                                            int accumulate_depth, float* grad_alpha, int accumulate_alpha, void* ws, size_t ws_bytes,
                                            void* stream_) {
    const char* who = "photo_reproj_loss_step";
    int rc = rp_check(who, depth, alpha, H, W, S, weight, alpha_min, ws, ws_bytes);
    if (rc) return rc;
    if ((rc = check_parts(who, parts))) return rc;
    RpTable tab{};
    RpTarget tk{};
    if ((rc = rp_check_stats(who, depth, alpha, target, sources, views, target_k, H, W, S, ws, ws_bytes, tab, tk))) return rc;
    if ((rc = rp_check_grad(who, depth, alpha, H, W, ws, ws_bytes, grad_depth, accumulate_depth, grad_alpha, accumulate_alpha))) return rc;
    {   // (the step entry alone sees the images: a gradient must not overlap the target or a source either)
        const size_t bytes = (size_t)H * (size_t)W * sizeof(float);
        for (const float* g : {(const float*)grad_depth, (const float*)grad_alpha}) {
            SYN3R_REQUIRE(!ranges_overlap(g, bytes, target, 3 * bytes), "%s: a gradient aliases the target image", who);
            for (int s = 0; s < S; ++s)
                SYN3R_REQUIRE(!ranges_overlap(g, bytes, sources[s], 3 * bytes), "%s: a gradient aliases source %d", who, s);
        }
    }
    hipStream_t stream = (hipStream_t)stream_;
    rp_stats(depth, alpha, target, H, W, S, tab, tk, alpha_min, ws, stream);
    rp_grad(depth, alpha, H, W, weight, alpha_min, grad_loss, ws, grad_depth, accumulate_depth, grad_alpha, accumulate_alpha, parts, stream);
    SYN3R_LAUNCH_CHECK("photo_reproj_loss_step launch");
    return SYN3R_OK;
}
