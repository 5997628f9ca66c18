// Shared declarations of the Gaussian rasteriser (forward, backward, sort).
//
// The reference's rasteriser (diff-gaussian-rasterization-confidence inside the
// un-vendored thirdparty/FSGS submodule; call sites model/diffusionGS.py:154,166
// and :139,1640) is NOT in /root/reference: this implementation
// restates the published 3DGS algorithm (Kerbl et al. 2023, "3D Gaussian
// Splatting for Real-Time Radiance Field Rendering", §4-§6 and appendix) with
// the depth / alpha outputs and the per-Gaussian confidence factor the call
// sites require.  Constants the published implementation fixes are named here so
// they can be matched against the CUDA build if it is ever supplied.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace syn3r {

constexpr int kTileX = 16;
constexpr int kTileY = 16;
constexpr int kTilePix = kTileX * kTileY;       // 256 threads = 4 wavefronts
constexpr float kNearClip = 0.2f;               // view-space z cull
constexpr float kFovGuard = 1.3f;               // clamp of t.x/t.z in the EWA Jacobian
constexpr float kLowPass = 0.3f;                // added to the 2D covariance diagonal
constexpr float kMipFloor = 0.000025f;          // anti-aliased splatting: floor of det(cov2D) / det(cov2D + kLowPass I), see mip_rho
constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr float kAlphaMax = 0.99f;
constexpr float kTransmittanceMin = 1e-4f;
constexpr float kLog2e = 1.4426950408889634f;  // the blend kernels' exp(x) is v_exp_f32 of x * log2(e), as __expf forms it (0x3fb8aa3b)

// Per-Gaussian screen-space record gathered by the blend kernels: 3 x 16-byte loads.
struct alignas(16) Splat {
    float x, y;            // pixel-space mean
    float cxx, cxy, cyy;   // conic (inverse 2D covariance)
    float opacity;         // opacity * confidence (* rho with SYN3R_RASTER_ANTIALIAS, mip_rho below)
    float r, g, b;         // view-dependent colour (SH evaluated, clamped)
    float depth;           // view-space z
    float pad0, pad1;
};
static_assert(sizeof(Splat) == 48, "Splat must be 48 bytes");

// Geometry state carved from the caller's buffer (all arrays 256-byte aligned).
struct GeomState {
    unsigned* header;        // [0] = number of (Gaussian, tile) pairs (the EXACT count, [3], when the lists were clipped), [1] = 1 if a render ran out of pair capacity, [2] = entries of the super-tile lists, [3] = sum of the tile rectangles' areas (hierarchical binning)
    float* depths;           // [N]
    float* means2D;          // [N,2]
    float* cov3D;            // [N,6]
    float* conic_opacity;    // [N,4] conic + raw opacity (without confidence, and without the anti-aliasing factor rho)
    float* rgb;              // [N,3]
    unsigned* clamped;       // [N] bit c set if colour channel c was clamped at 0
    unsigned* tiles_touched; // [N]
    unsigned* point_offsets; // [N] exclusive scan of tiles_touched IN DEPTH ORDER (entry i belongs to order[i])
    Splat* splats;           // [N]
    unsigned* dkeys_a;       // [N] depth bits of the visible Gaussians (0xFFFFFFFF otherwise), sort ping
    unsigned* dkeys_b;       // [N] sort pong
    unsigned* order_a;       // [N] Gaussian ids by ascending depth (stable), sort ping
    unsigned* order_b;       // [N] sort pong
    unsigned* order;         // whichever of order_a / order_b holds the result (4 passes: order_a)
    void* sort_scratch;      // argsort histograms
    void* scan_scratch;
};

#ifndef SYN3R_BIN_COUNTERS
#define SYN3R_BIN_COUNTERS 65536
#endif
constexpr size_t kBinCounters = SYN3R_BIN_COUNTERS;          // (chunk, super-tile) counters of the hierarchical binning
constexpr size_t kMaxSuperSlots = 4096;         // ... followed by the super-tile list starts (at most kMaxSuper + 1)
struct ImageState {
    uint2* ranges;           // [tiles] (start, end) into the sorted pair list
    unsigned* n_contrib;     // [H*W] index (1-based, within the tile list) of the last contributor
    float* final_T;          // [H*W]
    unsigned* tile_counts;   // [tiles][4] list length per tile and quarter of its super-tile's list (hierarchical binning)
    unsigned* bin_counters;  // [kBinCounters + kMaxSuperSlots] per (chunk, super-tile) counts, then the list starts
    unsigned* tile_order;    // [tiles] tiles by descending list length
};

struct BinningState {
    unsigned long long* keys_a;   // the rasteriser stores u32 tile ids here (half of each array is used)
    unsigned long long* keys_b;
    unsigned* vals_a;
    unsigned* vals_b;
    void* sort_scratch;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t scan_scratch_bytes(size_t n);
size_t sort_scratch_bytes(size_t n);
int exclusive_scan_u32(const unsigned* in, unsigned* out, size_t n, unsigned* total_out, void* scratch,
                       hipStream_t stream, const unsigned* perm = nullptr);   // perm: scan in[perm[i]]
// stable argsort of n u32 keys (vals_a is NOT read: element i carries i); 4 passes of 8 bits
int argsort_depth_u32(unsigned* keys_a, unsigned* vals_a, unsigned* keys_b, unsigned* vals_b, size_t n, void* scratch,
                      hipStream_t stream, int* result_in_b);
// stable sort of (u32 tile id, u32 Gaussian id) pairs on the low nbits of the key; 7-bit digits
int sort_pairs_by_tile_u32(unsigned* keys_a, unsigned* vals_a, unsigned* keys_b, unsigned* vals_b, size_t n, int nbits,
                           void* scratch, hipStream_t stream, int* result_in_b, const unsigned* n_dev);
int radix_sort_pairs(unsigned long long* keys_a, unsigned* vals_a, unsigned long long* keys_b, unsigned* vals_b,
                     size_t n, int nbits, void* scratch, hipStream_t stream, int* result_in_b,
                     const unsigned* n_dev = nullptr);

// camera passed by value to kernels
struct Camera {
    float view[16];     // world->view, column-major (x' = v[0]x + v[4]y + v[8]z + v[12])
    float proj[16];     // world->clip, column-major
    float campos[3];
    float tanfovx, tanfovy, focal_x, focal_y;
    int H, W, grid_x, grid_y;
};

size_t geom_bytes(int N);
bool raster_tiles_ordered(int N, int gx, int gy);   // did syn3r_raster_render leave ImageState::tile_order for this shape?
size_t image_bytes(int H, int W);
size_t binning_bytes(long long P);
GeomState carve_geom(void* buf, int N);
void raster_fill_camera(Camera& cam, const float* view, const float* proj, const float* campos, float tanfovx, float tanfovy, int H, int W);
ImageState carve_image(void* buf, int H, int W);
BinningState carve_binning(void* buf, long long P);

// What both passes are told about the scene: the common leading parameters of the four projection and the four backward entries
// (include/syn3r_hip.h), in their order, then raw / flags / filter3d from their tails (0 / 0 / null where an entry has none).
struct RasterScene {
    int N, sh_degree, sh_coeffs;
    const float *means3D, *scales, *rotations, *opacities, *shs, *confidence;   // confidence: may be null
    float scale_modifier;
    const float *viewmatrix, *projmatrix, *campos;
    float tanfovx, tanfovy;
    int H, W, raw, flags;
    const float* filter3d;                                                      // may be null
};
inline RasterScene raster_scene(int N, int sh_degree, int sh_coeffs, const float* means3D, const float* scales,
                                const float* rotations, const float* opacities, const float* shs, const float* confidence,
                                float scale_modifier, const float* viewmatrix, const float* projmatrix, const float* campos,
                                float tanfovx, float tanfovy, int H, int W, int raw, int flags, const float* filter3d) {
    return RasterScene{N, sh_degree, sh_coeffs, means3D, scales, rotations, opacities, shs, confidence, scale_modifier,
                       viewmatrix, projmatrix, campos, tanfovx, tanfovy, H, W, raw, flags, filter3d};
}
// SYN3R_OK, or SYN3R_E_INVALID with the error text set ("<who>: ..."): the one scene check of both passes, before anything is launched
int raster_check_scene(const char* who, const RasterScene& s);

// Tile binning (raster_bin.hip).  After k_preprocess: the depth argsort and the tile counts scanned in that order (pair-sort
// shapes), or the plain scan if the caller wants the exact pair count (header[0]) now (hierarchical binning: else nothing).
int raster_bin_prepare(const GeomState& g, int N, int gx, int gy, bool want_count, hipStream_t stream);
// Before k_render: ImageState::ranges and the list they index (pair capacity P); *tile_order: longest list first, or null.
int raster_bin_lists(const GeomState& g, const ImageState& im, const BinningState& bn, const int* radii, int N, int gx, int gy,
                     long long P, hipStream_t stream, unsigned** point_list, const unsigned** tile_order);

#ifdef __HIPCC__
// Conservative reach test used by the blend kernels to build per-wavefront visit lists: can the splat
// (pixel mean (mx,my), conic (A,B,C), opacity op) reach alpha >= kAlphaMin at ANY pixel centre of the
// rectangle [x0,x1] x [y0,y1]?  alpha = op * exp(-q/2) with q the conic's quadratic form, so the question is
// whether min q over the rectangle is <= 2 ln(255 op).  q is convex with its minimum at the mean: inside the
// rectangle the minimum is 0, otherwise it lies on an edge facing the mean, where q is a 1-D parabola whose
// clamped vertex is closed-form.  A margin keeps every pair the per-pixel test could accept despite rounding;
// pairs rejected here contribute exactly nothing in the unculled traversal, so results are unchanged.
__device__ __forceinline__ bool splat_reaches_rect(float mx, float my, float A, float B, float C, float op, float x0,
                                                   float x1, float y0, float y1) {
    if (!(A > 0.0f && C > 0.0f)) return true;              // not a proper conic: let the per-pixel test decide
    const float thr = 2.0f * __logf(255.0f * op);          // q must not exceed this (NaN / negative: unreachable)
    const float dx0 = x0 - mx, dx1 = x1 - mx, dy0 = y0 - my, dy1 = y1 - my;
    const bool inx = dx0 <= 0.0f && dx1 >= 0.0f, iny = dy0 <= 0.0f && dy1 >= 0.0f;
    float qmin = 0.0f;
    if (!(inx && iny)) {
        qmin = 3.0e38f;
        if (!inx) {                                        // the vertical edge facing the mean
            const float dx = dx0 > 0.0f ? dx0 : dx1;
            const float dy = fminf(fmaxf(-B * dx / C, dy0), dy1);
            qmin = A * dx * dx + 2.0f * B * dx * dy + C * dy * dy;
        }
        if (!iny) {                                        // the horizontal edge facing the mean
            const float dy = dy0 > 0.0f ? dy0 : dy1;
            const float dx = fminf(fmaxf(-B * dy / A, dx0), dx1);
            qmin = fminf(qmin, A * dx * dx + 2.0f * B * dx * dy + C * dy * dy);
        }
    }
    return qmin <= thr + (1.0e-3f + 1.0e-4f * thr);
}

// the tiles [x0, x1) x [y0, y1) a splat of this pixel mean and radius touches
__device__ __forceinline__ void tile_rect(float px, float py, int radius, int gx, int gy, int& x0, int& y0, int& x1,
                                          int& y1) {
    x0 = min(gx, max(0, (int)((px - radius) / kTileX)));
    y0 = min(gy, max(0, (int)((py - radius) / kTileY)));
    x1 = min(gx, max(0, (int)((px + radius + kTileX - 1) / kTileX)));
    y1 = min(gy, max(0, (int)((py + radius + kTileY - 1) / kTileY)));
}

// ---- The blend frame: what k_render and k_render_bwd must agree on bit for bit (the backward re-derives the forward's decisions).
// A 16 x 16 tile is a block of TWO wavefronts; wavefront w owns the 16 x 8 half (rows 8w .. 8w+7) and lane l the pixels
// (l & 15, 8w + (l >> 4)) and (.., + 4): per-pixel quantities are float2, for gfx950's packed fp32 arithmetic.
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 splat2(float s) { return (f2){s, s}; }
constexpr int kBlendThreads = 128;
struct BlendFrame {
    int px, py0, py1;              // the lane's pixels (px, py0), (px, py1)
    bool in0, in1;                 // ... inside the image?
    float fx;
    f2 fy;
};
struct BlendHalf { float sx0, sx1, sy0, sy1; };   // pixel centres of the wavefront's 16 x 8 half (splat_reaches_rect)
// (wq, lane) = (threadIdx.x >> 6, threadIdx.x & 63), formed IN the kernel, where the compiler knows the block size: the same code
__device__ __forceinline__ BlendFrame blend_frame(unsigned tile, int wq, int lane, int H, int W, int gx) {
    const int tx = tile % gx, ty = tile / gx;
    const int lx = lane & 15, ly = wq * 8 + (lane >> 4);
    BlendFrame f;
    f.px = tx * kTileX + lx; f.py0 = ty * kTileY + ly; f.py1 = f.py0 + 4;
    f.in0 = f.px < W && f.py0 < H; f.in1 = f.px < W && f.py1 < H;
    f.fx = (float)f.px;
    f.fy = (f2){(float)f.py0, (float)f.py1};
    return f;
}
// (on its own, called where the blend loop starts: formed with the frame it would reorder the kernels' prologues)
__device__ __forceinline__ BlendHalf blend_half(unsigned tile, int wq, int gx) {
    const int tx = tile % gx, ty = tile / gx;
    BlendHalf h;
    h.sx0 = (float)(tx * kTileX); h.sx1 = h.sx0 + 15.0f;
    h.sy0 = (float)(ty * kTileY + wq * 8); h.sy1 = h.sy0 + 7.0f;
    return h;
}
// a fetched 48-byte record into its 3 x float4 LDS slot: a = (x, y, cxx, cxy)  b = (cyy, opacity, r, g)  c = (b, depth, -, -)
__device__ __forceinline__ void stage_splat(float4* sm, int slot, const float4& n0, const float4& n1, const float4& n2) {
    sm[slot * 3 + 0] = n0;
    sm[slot * 3 + 1] = n1;
    sm[slot * 3 + 2] = n2;
}
// the (splat, pixel pair) evaluation: offsets mean - pixel, the exponent and G = exp(power); alpha = min(kAlphaMax, opacity * G)
struct BlendEval { float dx; f2 dy, power, G; };
__device__ __forceinline__ BlendEval blend_eval(const float4& a, const float4& b, const BlendFrame& f) {
    BlendEval e;
    e.dx = a.x - f.fx;
    e.dy = splat2(a.y) - f.fy;
    const float hxx = -0.5f * a.z * e.dx * e.dx, bxy = a.w * e.dx;
    e.power = (-0.5f * b.x) * e.dy * e.dy - bxy * e.dy + hxx;
    const f2 pl = e.power * kLog2e;   // __expf's own multiply, as one packed instruction for the pair: the same bits
    e.G = (f2){__builtin_amdgcn_exp2f(pl.x), __builtin_amdgcn_exp2f(pl.y)};
    return e;
}

// ---- The projection pieces k_preprocess and k_preprocess_bwd share.  The backward forms several of the forward's values again, some
// of them to the bit (rho, coef, the raw route's activations of common.h): those come from ONE function with its roundings spelled out.
constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
static __constant__ float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                      -1.0925484305920792f, 0.5462742152960396f};
static __constant__ float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                                      -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};
// world -> view (three rows) and world -> clip (four) of a column-major 4 x 4 matrix (Camera::view, Camera::proj)
__device__ __forceinline__ float3 xf43(const float* m, float3 p) {
    return make_float3(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]);
}
__device__ __forceinline__ float4 xf44(const float* m, float3 p) {
    return make_float4(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                       m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14], m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15]);
}
// rotation of the quaternion q = (r, x, y, z) (not renormalised here); the kernels form M = R S themselves (Sigma = M M^T)
struct Rot3 { float R00, R01, R02, R10, R11, R12, R20, R21, R22; };
__device__ __forceinline__ Rot3 quat_rotation(float4 q) {
    const float qr = q.x, qx = q.y, qy = q.z, qz = q.w;
    Rot3 o;
    o.R00 = 1.f - 2.f * (qy * qy + qz * qz); o.R01 = 2.f * (qx * qy - qr * qz); o.R02 = 2.f * (qx * qz + qr * qy);
    o.R10 = 2.f * (qx * qy + qr * qz); o.R11 = 1.f - 2.f * (qx * qx + qz * qz); o.R12 = 2.f * (qy * qz - qr * qx);
    o.R20 = 2.f * (qx * qz - qr * qy); o.R21 = 2.f * (qy * qz + qr * qx); o.R22 = 1.f - 2.f * (qx * qx + qy * qy);
    return o;
}
// EWA: the Jacobian J of the projection at the view-space mean t, with t.x / t.z and t.y / t.z clamped to the guarded field of
// view ((tx, ty) = the clamped values times t.z), and the rows of T = J W, W = rotation part of the view matrix (W[r][c] = v[c*4+r])
struct EwaRows { float tx, ty, T00, T01, T02, T10, T11, T12; };
__device__ __forceinline__ EwaRows ewa_rows(const Camera& cam, float t_x, float t_y, float t_z) {
    const float limx = kFovGuard * cam.tanfovx, limy = kFovGuard * cam.tanfovy;
    EwaRows o;
    o.tx = fminf(limx, fmaxf(-limx, t_x / t_z)) * t_z;
    o.ty = fminf(limy, fmaxf(-limy, t_y / t_z)) * t_z;
    const float J00 = cam.focal_x / t_z, J02 = -(cam.focal_x * o.tx) / (t_z * t_z);
    const float J11 = cam.focal_y / t_z, J12 = -(cam.focal_y * o.ty) / (t_z * t_z);
    const float* v = cam.view;
    o.T00 = J00 * v[0] + J02 * v[2]; o.T01 = J00 * v[4] + J02 * v[6]; o.T02 = J00 * v[8] + J02 * v[10];
    o.T10 = J11 * v[1] + J12 * v[2]; o.T11 = J11 * v[5] + J12 * v[6]; o.T12 = J11 * v[9] + J12 * v[10];
    return o;
}
// cov2D = T Sigma T^T with Sigma = (c0 c1 c2; c1 c3 c4; c2 c4 c5): the products Sigma T_0^T = (a0, a1, a2), Sigma T_1^T = (b0, b1, b2)
// (the backward's dL/dT needs them) and the covariance (xx, xy; xy, yy) BEFORE the dilation; both kernels add kLowPass to xx and yy
// where they use it.
struct EwaCov { float a0, a1, a2, b0, b1, b2, xx, yy, xy; };
__device__ __forceinline__ EwaCov ewa_cov(const EwaRows& w, float c0, float c1, float c2, float c3, float c4, float c5) {
    EwaCov o;
    o.a0 = c0 * w.T00 + c1 * w.T01 + c2 * w.T02; o.a1 = c1 * w.T00 + c3 * w.T01 + c4 * w.T02; o.a2 = c2 * w.T00 + c4 * w.T01 + c5 * w.T02;
    o.b0 = c0 * w.T10 + c1 * w.T11 + c2 * w.T12; o.b1 = c1 * w.T10 + c3 * w.T11 + c4 * w.T12; o.b2 = c2 * w.T10 + c4 * w.T11 + c5 * w.T12;
    o.xx = w.T00 * o.a0 + w.T01 * o.a1 + w.T02 * o.a2;
    o.yy = w.T10 * o.b0 + w.T11 * o.b1 + w.T12 * o.b2;
    o.xy = w.T00 * o.b0 + w.T01 * o.b1 + w.T02 * o.b2;
    return o;
}
// AA (SYN3R_RASTER_ANTIALIAS, the published 3DGS `antialiasing` switch = the 2D Mip filter of Mip-Splatting, Yu et al. CVPR 2024): the
// dilation of the 2D covariance (a, b; b, c) to (a + kLowPass, b; b, c + kLowPass) stays and the opacity the blend multiplies carries
//     rho = sqrt(max(r, kMipFloor)),  r = (a c - b^2) / ((a + kLowPass)(c + kLowPass) - b^2),
// so a splat keeps its energy whatever its size on screen.  Conic, radius, tile rectangle, depth key and colour are the same values as
// without AA (same expressions), so the tile lists are too.  In fp32 the first determinant can cancel to zero or below (needles):
// fmaxf drops a NaN operand and puts those on the floor, so rho is finite whatever the cancellation in r did.  The constants 0.3 and
// 0.000025 are RECALLED from the published code, which is not available to check against: UNPINNED.
__device__ __forceinline__ float mip_rho(float r) { return sqrtf(fmaxf(r, kMipFloor)); }
// r from the covariance before the dilation.  The forward and the backward must agree to the bit on which side of kMipFloor a Gaussian
// lies (the forward's rho is a constant there, the backward's gradient through rho zero), so every rounding is spelled out: r does not
// depend on how the compiler contracts either kernel's own determinant (`det` / `den`, the conic's, which may fuse differently in the two).
__device__ __forceinline__ float mip_ratio(float a, float b, float c) {
    const float bb = __fmul_rn(b, b);
    const float d0 = __fmaf_rn(a, c, -bb);
    const float d1 = __fmaf_rn(__fadd_rn(a, kLowPass), __fadd_rn(c, kLowPass), -bb);
    return __fdiv_rn(d0, d1);
}

// F3D (the `_f3d` entries with a filter: the 3D smoothing filter of Mip-Splatting, section 4.1): a Gaussian with activated scales s_i
// and filter f (csrc/filter3d.hip: sqrt(variance) / its largest sampling rate over the training cameras) is rendered with
// q_i = sqrt(s_i^2 + f^2)  and its opacity times  coef = prod_i s_i / q_i  (= sqrt(det Sigma / det(Sigma + f^2 I)): the rotation
// drops out); radii, tile lists and depth keys are those of the filtered Gaussian, and with AA rho comes from the FILTERED covariance.
// coef is the product of the three per-axis ratios r_i, never a ratio of determinants: s = 1e-6 against f = 1e-2 gives r = 1e-4 and
// coef = 1e-12, where s^6 would have left fp32.  Every rounding is spelled out, so the backward's coef is the forward's bits.  f = 0
// (no camera saw any Gaussian) leaves q = s, r = 1, also for s = 0.
struct F3dScales { float q0, q1, q2, r0, r1, r2, coef, ff; };
__device__ __forceinline__ F3dScales f3d_scales(float s0, float s1, float s2, float f) {
    F3dScales o;
    o.ff = __fmul_rn(f, f);
    o.q0 = sqrtf(__fmaf_rn(s0, s0, o.ff)); o.q1 = sqrtf(__fmaf_rn(s1, s1, o.ff)); o.q2 = sqrtf(__fmaf_rn(s2, s2, o.ff));
    o.r0 = o.q0 > 0.0f ? __fdiv_rn(s0, o.q0) : 1.0f;
    o.r1 = o.q1 > 0.0f ? __fdiv_rn(s1, o.q1) : 1.0f;
    o.r2 = o.q2 > 0.0f ? __fdiv_rn(s2, o.q2) : 1.0f;
    o.coef = __fmul_rn(__fmul_rn(o.r0, o.r1), o.r2);
    return o;
}
// x times what the blend opacity carries besides the opacity and the confidence: coef (1 without F3D), then rho (1 without AA), in
// THIS order - the forward's Splat::opacity is mode_factors(op, coef, rho) * cf, and the bits depend on the order (a factor 1 is
// exact and folds away).  GeomState::conic_opacity[3] keeps the plain op in every mode; the backward forms rho and coef again.
__device__ __forceinline__ float mode_factors(float x, float coef, float rho) { return x * coef * rho; }

#ifdef SYN3R_RASTER_STATS     // developer build, per blend kernel: [0] lane tests, [1] wavefront visits, [2] visits with an active pixel, [3] active pixels
#define RASTER_STAT(arr, i, n) do { if (lane == 0) atomicAdd(&arr[i], (unsigned long long)(n)); } while (0)
#else
#define RASTER_STAT(arr, i, n)
#endif
#endif

}  // namespace syn3r
