// Prior-free edge-aware depth smoothness (EXTENSION, include/syn3r_hip.h): the form of Monodepth2 (Godard et al., ICCV 2019), which
// DNGaussian-, SparseGS- and RegNeRF-style sparse-view pipelines use as well.  The rendered depth d [H,W] should be piecewise smooth
// and may jump only where the camera's own target image I [3,H,W] has an edge:
//   wx[y,x] = exp(-gamma * mean_c |I_c[y,x+1] - I_c[y,x]|)      wy[y,x] = exp(-gamma * mean_c |I_c[y+1,x] - I_c[y,x]|)
//   m    = mean of d over all H*W pixels
//   S_x  = 1/N_x * sum_{y, x<W-1} wx[y,x] * |d[y,x+1] - d[y,x]|      N_x = H (W-1)
//   S_y  = 1/N_y * sum_{y<H-1, x} wy[y,x] * |d[y+1,x] - d[y,x]|      N_y = (H-1) W
//   loss = weight * (S_x + S_y) / m
//   grad_depth_i = weight * g * [ (dS/dd_i) / m - (S_x + S_y) / (m^2 H W) ]                     (g: device scalar, NULL = 1)
// dS/dd_i is the signed sum over the up to four edges at pixel i with sign(0) = 0; the derivative goes through the mean.  A
// direction without pairs (W == 1 or H == 1) contributes 0.  m <= 0 (an empty render; a NaN mean as well) gives loss 0 and a zero
// gradient, never NaN.  The last column of wx and the last row of wy are absent: never used, whatever they hold.
// PROVENANCE: gamma = 1 and the division by the mean are recalled from Monodepth2, which is not available to check: UNPINNED.
//
// Groups of four pixels, the grid rule, VEC and the order of the sums: plane_pass.h (blocks = min(ceil(H G / 256), 1024) of 256
// threads for all three kernels).  The halo (rows y - 1, y + 1, columns 4 gx - 1, 4 gx + 4) comes through repeated unconditional
// loads, not LDS: measured, profiles/r20/depth_smooth.txt.
//
// k_dsmooth_weights: image in, the two planes out (zeros in the absent column and row); once per camera.  expf, no fast intrinsic.
// k_dsmooth_stats:   one pass over d, wx, wy.  A thread keeps fp32 running sums of S_x N_x, S_y N_y and sum d (4 terms each per
//                    trip, left to right) and leaves ONE row per block (block_rows).  ds_combine: combine_rows and what follows from it.
// k_dsmooth_final:   one block: ds_combine, writes parts.
// k_dsmooth_grad:    GATHER form: the thread that owns pixel i forms i's incident edges itself and writes grad_depth_i once (fp64
//                    arithmetic, one fp32 rounding); no scatter, no float atomics.  Every block runs ds_combine (the same order
//                    everywhere, the same bits), block 0 writes parts when asked.  ACC: the value is ADDED to grad_depth.
// Built without fma contraction (build.py STRICT_FP).
#include "plane_pass.h"

using namespace syn3r;

namespace {

constexpr int kDsThreads = 256;
constexpr int kDsMaxBlocks = 1024;
static_assert(kDsThreads == kPassThreads && kDsMaxBlocks == kPassMaxBlocks, "block_rows / combine_rows: 256 threads, four rows per thread");

// what the combined rows give: the value record and the gradient's coefficients for weight * g = 1
struct DsCoef { double sx, sy, m, loss1, ax, ay, c0; bool empty; };

__device__ __forceinline__ float ds_sel(bool ok, float v) { return ok ? v : 0.0f; }
// sign(a - b) from the comparison itself: exact whatever the subtraction would round or flush to
__device__ __forceinline__ double ds_sign(float a, float b) { return a > b ? 1.0 : (a < b ? -1.0 : 0.0); }

__device__ __forceinline__ float ds_weight1(float gamma, float a0, float b0, float a1, float b1, float a2, float b2) {
    return expf(-gamma * (((fabsf(b0 - a0) + fabsf(b1 - a1)) + fabsf(b2 - a2)) / 3.0f));
}

template <bool VEC>
__global__ void __launch_bounds__(kDsThreads) k_dsmooth_weights(const float* __restrict__ image, int H, int W, int G, float gamma,
                                                               float* __restrict__ weights) {
    const size_t plane = (size_t)H * (size_t)W;
    plane_walk<kDsThreads>(H, G, [&](int y, int x0) {
        const int yd = y + 1 < H ? y + 1 : H - 1, xr = x0 + 4 < W ? x0 + 4 : W - 1;
        float4 c[3], dn[3];
        float r[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            c[k] = load4<VEC>(image + k * plane, y, x0, W);
            dn[k] = load4<VEC>(image + k * plane, yd, x0, W);
            r[k] = image[k * plane + (size_t)y * (size_t)W + xr];
        }
        const bool dy = y + 1 < H;
        float4 wx, wy;
        wx.x = ds_sel(x0 + 1 < W, ds_weight1(gamma, c[0].x, c[0].y, c[1].x, c[1].y, c[2].x, c[2].y));
        wx.y = ds_sel(x0 + 2 < W, ds_weight1(gamma, c[0].y, c[0].z, c[1].y, c[1].z, c[2].y, c[2].z));
        wx.z = ds_sel(x0 + 3 < W, ds_weight1(gamma, c[0].z, c[0].w, c[1].z, c[1].w, c[2].z, c[2].w));
        wx.w = ds_sel(x0 + 4 < W, ds_weight1(gamma, c[0].w, r[0], c[1].w, r[1], c[2].w, r[2]));
        wy.x = ds_sel(dy, ds_weight1(gamma, c[0].x, dn[0].x, c[1].x, dn[1].x, c[2].x, dn[2].x));
        wy.y = ds_sel(dy, ds_weight1(gamma, c[0].y, dn[0].y, c[1].y, dn[1].y, c[2].y, dn[2].y));
        wy.z = ds_sel(dy, ds_weight1(gamma, c[0].z, dn[0].z, c[1].z, dn[1].z, c[2].z, dn[2].z));
        wy.w = ds_sel(dy, ds_weight1(gamma, c[0].w, dn[0].w, c[1].w, dn[1].w, c[2].w, dn[2].w));
        store4<VEC>(weights, y, x0, W, wx);
        store4<VEC>(weights + plane, y, x0, W, wy);
    });
}

template <bool VEC>
__global__ void __launch_bounds__(kDsThreads) k_dsmooth_stats(const float* __restrict__ d, const float* __restrict__ wgt, int H, int W,
                                                             int G, float4* __restrict__ rows) {
    const float* wxp = wgt;
    const float* wyp = wgt + (size_t)H * (size_t)W;
    float sx = 0.0f, sy = 0.0f, sd = 0.0f;
    plane_walk<kDsThreads>(H, G, [&](int y, int x0) {
        const int yd = y + 1 < H ? y + 1 : H - 1, xr = x0 + 4 < W ? x0 + 4 : W - 1;
        const float4 c = load4<VEC>(d, y, x0, W), dn = load4<VEC>(d, yd, x0, W);
        const float4 wx = load4<VEC>(wxp, y, x0, W), wy = load4<VEC>(wyp, y, x0, W);
        const float r = d[(size_t)y * (size_t)W + xr];
        const bool dy = y + 1 < H;
        sx += ds_sel(x0 + 1 < W, wx.x * fabsf(c.y - c.x));
        sx += ds_sel(x0 + 2 < W, wx.y * fabsf(c.z - c.y));
        sx += ds_sel(x0 + 3 < W, wx.z * fabsf(c.w - c.z));
        sx += ds_sel(x0 + 4 < W, wx.w * fabsf(r - c.w));
        sy += ds_sel(dy, wy.x * fabsf(dn.x - c.x));
        sy += ds_sel(dy && x0 + 1 < W, wy.y * fabsf(dn.y - c.y));
        sy += ds_sel(dy && x0 + 2 < W, wy.z * fabsf(dn.z - c.z));
        sy += ds_sel(dy && x0 + 3 < W, wy.w * fabsf(dn.w - c.w));
        sd += c.x;
        sd += ds_sel(x0 + 1 < W, c.y);
        sd += ds_sel(x0 + 2 < W, c.z);
        sd += ds_sel(x0 + 3 < W, c.w);
    });
    if (block_rows(sx, sy, sd)) rows[xcd_remap(blockIdx.x, gridDim.x)] = make_float4(sx, sy, sd, 0.0f);
}

// what every caller derives from the combined rows (the same bits on every thread of every block)
__device__ DsCoef ds_combine(const float4* __restrict__ rows, int nrows, int H, int W) {
    double sx, sy, sd;
    combine_rows(rows, nrows, sx, sy, sd);
    DsCoef k{};
    const double n = (double)H * (double)W, nx = (double)H * (double)(W - 1), ny = (double)(H - 1) * (double)W;
    k.m = sd / n;
    k.empty = !(k.m > 0.0);
    k.sx = nx > 0.0 ? sx / nx : 0.0;
    k.sy = ny > 0.0 ? sy / ny : 0.0;
    if (!k.empty) {
        k.loss1 = (k.sx + k.sy) / k.m;
        k.ax = nx > 0.0 ? 1.0 / (nx * k.m) : 0.0;
        k.ay = ny > 0.0 ? 1.0 / (ny * k.m) : 0.0;
        k.c0 = (k.sx + k.sy) / (k.m * k.m * n);
    }
    return k;
}

// parts = [loss, S_x, S_y, m]
__device__ __forceinline__ void ds_write_parts(const DsCoef& k, float weight, float* __restrict__ parts) {
    *(float4*)parts = make_float4((float)((double)weight * k.loss1), (float)k.sx, (float)k.sy, (float)k.m);
}

__global__ void __launch_bounds__(kDsThreads) k_dsmooth_final(const float4* __restrict__ rows, int nrows, int H, int W, float weight,
                                                             float* __restrict__ parts) {
    const DsCoef k = ds_combine(rows, nrows, H, W);
    if (threadIdx.x == 0) ds_write_parts(k, weight, parts);
}

template <bool VEC, bool ACC>
__global__ void __launch_bounds__(kDsThreads) k_dsmooth_grad(const float* __restrict__ d, const float* __restrict__ wgt, int H, int W,
                                                            int G, const float4* __restrict__ rows, int nrows, float weight,
                                                            const float* __restrict__ go, float* __restrict__ grad,
                                                            float* __restrict__ parts) {
    const DsCoef k = ds_combine(rows, nrows, H, W);
    if (parts && blockIdx.x == 0 && threadIdx.x == 0) ds_write_parts(k, weight, parts);
    const double wg = (double)weight * (go ? (double)*go : 1.0);
    const double ax = wg * k.ax, ay = wg * k.ay, c0 = wg * k.c0;
    const bool empty = k.empty;
    const float* wxp = wgt;
    const float* wyp = wgt + (size_t)H * (size_t)W;
    plane_walk<kDsThreads>(H, G, [&](int y, int x0) {
        const int yu = y > 0 ? y - 1 : 0, yd = y + 1 < H ? y + 1 : H - 1;
        const int xl = x0 > 0 ? x0 - 1 : 0, xr = x0 + 4 < W ? x0 + 4 : W - 1;
        const size_t row = (size_t)y * (size_t)W;
        const float4 c = load4<VEC>(d, y, x0, W), up = load4<VEC>(d, yu, x0, W), dn = load4<VEC>(d, yd, x0, W);
        const float4 wx = load4<VEC>(wxp, y, x0, W), wy = load4<VEC>(wyp, y, x0, W), wu = load4<VEC>(wyp, yu, x0, W);
        const float dl = d[row + xl], dr = d[row + xr], wl = wxp[row + xl];
        float4 old = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (ACC) old = load4<VEC>(grad, y, x0, W);
        const bool hu = y > 0, hd = y + 1 < H;
        // pixel x: its left edge (weight wa, neighbour a), right edge (wb, b), the edges above (wc, e) and below (wd, f)
        auto one = [&](bool has_l, float wa, float a, bool has_r, float wb, float b, float v, float wc, float e, float wd, float f) -> float {
            if (empty) return 0.0f;
            const double ex = (has_l ? (double)wa * ds_sign(v, a) : 0.0) - (has_r ? (double)wb * ds_sign(b, v) : 0.0);
            const double ey = (hu ? (double)wc * ds_sign(v, e) : 0.0) - (hd ? (double)wd * ds_sign(f, v) : 0.0);
            return (float)((ax * ex + ay * ey) - c0);
        };
        float4 o;
        o.x = one(x0 > 0, wl, dl, x0 + 1 < W, wx.x, c.y, c.x, wu.x, up.x, wy.x, dn.x);
        o.y = one(true, wx.x, c.x, x0 + 2 < W, wx.y, c.z, c.y, wu.y, up.y, wy.y, dn.y);
        o.z = one(true, wx.y, c.y, x0 + 3 < W, wx.z, c.w, c.z, wu.z, up.z, wy.z, dn.z);
        o.w = one(true, wx.z, c.z, x0 + 4 < W, wx.w, dr, c.w, wu.w, up.w, wy.w, dn.w);
        if constexpr (ACC) { o.x = old.x + o.x; o.y = old.y + o.y; o.z = old.z + o.z; o.w = old.w + o.w; }
        store4<VEC>(grad, y, x0, W, o);
    });
}

// blocks of all three grids: a function of H and W alone
int ds_blocks(int H, int W) { return pass_blocks((long long)H * groups_per_row(W), kDsThreads, kDsMaxBlocks); }

// argument checks shared by the three loss entries, all before any HIP call (ws: the rows of the statistics pass)
int ds_check(const char* who, const float* depth, const float* weights, int H, int W, float weight, const void* ws, size_t ws_bytes) {
    SYN3R_REQUIRE(SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W), "%s: H=%d, W=%d must be in [1, 2^15]", who, H, W);
    SYN3R_REQUIRE(depth && weights && ws, "%s: null pointer", who);
    SYN3R_REQUIRE(finite_f32(weight), "%s: weight must be finite", who);
    return check_workspace(who, ws, ws_bytes, syn3r_depth_smooth_workspace_bytes(H, W), "syn3r_depth_smooth_workspace_bytes");
}

// the checks of an entry that writes grad_depth
int ds_check_grad(const char* who, const float* depth, const float* weights, int H, int W, const float* grad_depth, int accumulate) {
    if (const int rc = check_grad_target(who, grad_depth, accumulate, "accumulate")) return rc;
    const size_t bytes = (size_t)H * (size_t)W * sizeof(float);
    SYN3R_REQUIRE(!ranges_overlap(grad_depth, bytes, depth, bytes) && !ranges_overlap(grad_depth, bytes, weights, 2 * bytes),
                  "%s: grad_depth aliases an input", who);
    return SYN3R_OK;
}

void ds_stats(const float* depth, const float* weights, int H, int W, void* ws, hipStream_t stream) {
    const dim3 grid((unsigned)ds_blocks(H, W));
    const int G = groups_per_row(W);
    with_bools([&](auto vec) {
        SYN3R_LAUNCH_NAMED("k_dsmooth_stats", k_dsmooth_stats<decltype(vec)::value>, grid, dim3(kDsThreads), 0, stream, depth, weights, H, W,
                           G, (float4*)ws);
    }, W % 4 == 0 && aligned16(depth, weights));
}

void ds_grad(const float* depth, const float* weights, int H, int W, float weight, const float* grad_loss, const void* ws,
             float* grad_depth, int accumulate, float* parts, hipStream_t stream) {
    const int nb = ds_blocks(H, W), G = groups_per_row(W);
    with_bools([&](auto vec, auto acc) {
        SYN3R_LAUNCH_NAMED("k_dsmooth_grad", (k_dsmooth_grad<decltype(vec)::value, decltype(acc)::value>), dim3((unsigned)nb), dim3(kDsThreads),
                           0, stream, depth, weights, H, W, G, (const float4*)ws, nb, weight, grad_loss, grad_depth, parts);
    }, W % 4 == 0 && aligned16(depth, weights, grad_depth), accumulate != 0);
}

}  // namespace

extern "C" int syn3r_depth_edge_weights(const float* image, int H, int W, float gamma, float* weights, void* stream_) {
    SYN3R_REQUIRE(SYN3R_SIDE_OK(H) && SYN3R_SIDE_OK(W), "depth_edge_weights: H=%d, W=%d must be in [1, 2^15]", H, W);
    SYN3R_REQUIRE(image && weights, "depth_edge_weights: null pointer");
    SYN3R_REQUIRE(finite_f32(gamma) && gamma >= 0.0f, "depth_edge_weights: gamma must be finite and >= 0");
    const size_t plane = (size_t)H * (size_t)W * sizeof(float);
    SYN3R_REQUIRE(!ranges_overlap(weights, 2 * plane, image, 3 * plane), "depth_edge_weights: weights aliases an input");
    const dim3 grid((unsigned)ds_blocks(H, W));
    const int G = groups_per_row(W);
    hipStream_t stream = (hipStream_t)stream_;
    with_bools([&](auto vec) {
        SYN3R_LAUNCH_NAMED("k_dsmooth_weights", k_dsmooth_weights<decltype(vec)::value>, grid, dim3(kDsThreads), 0, stream, image, H, W, G,
                           gamma, weights);
    }, W % 4 == 0 && aligned16(image, weights));
    SYN3R_LAUNCH_CHECK("depth_edge_weights launch");
    return SYN3R_OK;
}

extern "C" size_t syn3r_depth_smooth_workspace_bytes(int H, int W) {
    if (!SYN3R_SIDE_OK(H) || !SYN3R_SIDE_OK(W)) return 0;
    return (((size_t)ds_blocks(H, W) * sizeof(float4) + 255) / 256) * 256;
}

extern "C" int syn3r_depth_smooth_loss(const float* depth, const float* weights, int H, int W, float weight, float* parts, void* ws,
                                       size_t ws_bytes, void* stream_) {
    int rc = ds_check("depth_smooth_loss", depth, weights, H, W, weight, ws, ws_bytes);
    if (rc) return rc;
    if ((rc = check_parts("depth_smooth_loss", parts))) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    ds_stats(depth, weights, H, W, ws, stream);
    SYN3R_LAUNCH(k_dsmooth_final, dim3(1), dim3(kDsThreads), 0, stream, (const float4*)ws, ds_blocks(H, W), H, W, weight, parts);
    SYN3R_LAUNCH_CHECK("depth_smooth_loss launch");
    return SYN3R_OK;
}

extern "C" int syn3r_depth_smooth_loss_backward(const float* depth, const float* weights, int H, int W, float weight,
                                                const float* grad_loss, const void* ws, size_t ws_bytes, float* grad_depth,
                                                int accumulate, void* stream_) {
    int rc = ds_check("depth_smooth_loss_backward", depth, weights, H, W, weight, ws, ws_bytes);
    if (rc) return rc;
    rc = ds_check_grad("depth_smooth_loss_backward", depth, weights, H, W, grad_depth, accumulate);
    if (rc) return rc;
    ds_grad(depth, weights, H, W, weight, grad_loss, ws, grad_depth, accumulate, nullptr, (hipStream_t)stream_);
    SYN3R_LAUNCH_CHECK("depth_smooth_loss_backward launch");
    return SYN3R_OK;
}

extern "C" int syn3r_depth_smooth_loss_step(const float* depth, const float* weights, int H, int W, float weight, const float* grad_loss,
                                            float* parts, float* grad_depth, int accumulate, void* ws, size_t ws_bytes, void* stream_) {
    int rc = ds_check("depth_smooth_loss_step", depth, weights, H, W, weight, ws, ws_bytes);
    if (rc) return rc;
    if ((rc = check_parts("depth_smooth_loss_step", parts))) return rc;
    rc = ds_check_grad("depth_smooth_loss_step", depth, weights, H, W, grad_depth, accumulate);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    ds_stats(depth, weights, H, W, ws, stream);
    ds_grad(depth, weights, H, W, weight, grad_loss, ws, grad_depth, accumulate, parts, stream);
    SYN3R_LAUNCH_CHECK("depth_smooth_loss_step launch");
    return SYN3R_OK;
}
