// Mip-Splatting's 3D smoothing filter (Yu et al., CVPR 2024, section 4.1), the per-Gaussian filter size: syn3r_filter3d_compute.
//
// A Gaussian k reconstructed from N cameras cannot carry detail finer than the densest sampling any of them gave it: with the
// view-space point (x, y, z) of k in camera n, the sampling rate is  nu_k = max over the cameras that SEE k of fx_n / z  (the
// paper's Eq. 6; the released code's min depth / max focal when every focal length is the same), and the filter the projection
// kernels apply (f3d_scales, raster_common.h) is  filter_k = sqrt(variance) / nu_k = sqrt(variance) min_n z / fx_n.  A camera sees
// the point iff z > near and its pixel (fx x / z + W / 2, fy y / z + H / 2) lies in [-margin W, (1 + margin) W] x [-margin H,
// (1 + margin) H].  A Gaussian no camera sees takes the LARGEST filter among the seen ones (the released code's rule); if none is
// seen every filter is 0.  variance = 0.2, near = 0.2 and margin = 0.15 are the caller's arguments: RECALLED from the released
// Mip-Splatting code (compute_3D_filter), which is not available to check against - UNPINNED, as the anti-aliasing constants.
// The reference's trainer (FSGS, not vendored) is not known to have the filter: an option of this port.
//
// MI355X mapping: one thread per Gaussian; the camera loop's index is wave-uniform and the table read-only, so its 16 floats per
// camera arrive through the scalar cache, once per wavefront.  The largest filter is reduced over the wavefront (wave_max), over the
// block's four wavefronts in LDS, and leaves the block as ONE vector atomicMax on the float's bit pattern (the values are positive:
// the patterns order as unsigned integers).  A second launch gives the unseen Gaussians that maximum.  No host read, no
// synchronisation: the entry is stream-ordered like every other launch of a training step.
#include "common.h"

using namespace syn3r;

namespace {

constexpr int kThreads = 256;
constexpr size_t kWsBytes = 256;     // one word (the bit pattern of the largest filter), padded to the allocation granule

__global__ void __launch_bounds__(kThreads) k_filter3d(const float* __restrict__ xyz, int n, const float* __restrict__ cams,
                                                       int n_cams, float sd, float near, float margin,
                                                       float* __restrict__ filter_out, unsigned* __restrict__ ws_max) {
    __shared__ float s_part[kThreads / 64];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    float best = -1.0f;                  // min over the seeing cameras of z / fx; negative: unseen so far
    if (i < n) {
        const float px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
        for (int c = 0; c < n_cams; ++c) {
            const float* m = cams + 16 * (size_t)c;          // rows of [R | t] (world -> view), then fx, fy, W, H
            const float x = m[0] * px + m[1] * py + m[2] * pz + m[3];
            const float y = m[4] * px + m[5] * py + m[6] * pz + m[7];
            const float z = m[8] * px + m[9] * py + m[10] * pz + m[11];
            const float fx = m[12], fy = m[13], W = m[14], H = m[15];
            if (!(z > near)) continue;
            const float u = fx * x / z + 0.5f * W, v = fy * y / z + 0.5f * H;
            const bool seen = u >= -margin * W && u <= (1.0f + margin) * W && v >= -margin * H && v <= (1.0f + margin) * H;
            if (!seen) continue;
            const float zf = z / fx;
            best = best < 0.0f ? zf : fminf(best, zf);
        }
    }
    const float f = best < 0.0f ? -1.0f : sd * best;       // sd = sqrt(variance); fx > 0 and z > near > 0: f >= 0
    if (i < n) filter_out[i] = f;                           // unseen: negative, k_filter3d_fill replaces it
    const float wmax = wave_max(fmaxf(f, 0.0f));
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = wmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        float bmax = s_part[0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) bmax = fmaxf(bmax, s_part[w]);
        if (bmax > 0.0f) atomicMax(ws_max, __float_as_uint(bmax));
    }
}

__global__ void __launch_bounds__(kThreads) k_filter3d_fill(float* __restrict__ filter_out, int n,
                                                            const unsigned* __restrict__ ws_max) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (filter_out[i] < 0.0f) filter_out[i] = __uint_as_float(*ws_max);      // none seen at all: the memset's 0
}

}  // namespace

extern "C" size_t syn3r_filter3d_workspace_bytes(int n) { return SYN3R_DIM_OK(n) ? kWsBytes : 0; }

extern "C" int syn3r_filter3d_compute(const float* xyz, int n, const float* cams, int n_cams, float variance, float near,
                                      float margin, float* filter_out, void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(xyz && cams && filter_out && ws, "filter3d_compute: null pointer");
    SYN3R_REQUIRE(SYN3R_DIM_OK(n), "filter3d_compute: needs 1 .. %d Gaussians, got n=%d", SYN3R_DIM_MAX, n);
    SYN3R_REQUIRE(SYN3R_DIM_OK(n_cams), "filter3d_compute: needs 1 .. %d cameras, got n_cams=%d", SYN3R_DIM_MAX, n_cams);
    SYN3R_REQUIRE(variance > 0.0f && variance < 3.0e38f, "filter3d_compute: variance must be positive and finite");
    SYN3R_REQUIRE(near > 0.0f && near < 3.0e38f, "filter3d_compute: near must be positive and finite");
    SYN3R_REQUIRE(margin >= 0.0f && margin < 3.0e38f, "filter3d_compute: margin must be non-negative and finite");
    if (ws_bytes < kWsBytes) {
        set_error("filter3d_compute: workspace too small (%zu < %zu)", ws_bytes, kWsBytes);
        return SYN3R_E_WORKSPACE;
    }
    SYN3R_REQUIRE(((uintptr_t)ws & 3) == 0, "filter3d_compute: workspace must be 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    unsigned* ws_max = (unsigned*)ws;
    if (int rc = check_hip(hipMemsetAsync(ws_max, 0, sizeof(unsigned), stream), "filter3d_compute memset")) return rc;
    const int blocks = ceil_div(n, kThreads);
    SYN3R_LAUNCH(k_filter3d, dim3(blocks), dim3(kThreads), 0, stream, xyz, n, cams, n_cams, sqrtf(variance), near, margin, filter_out,
                 ws_max);
    SYN3R_LAUNCH(k_filter3d_fill, dim3(blocks), dim3(kThreads), 0, stream, filter_out, n, (const unsigned*)ws_max);
    SYN3R_LAUNCH_CHECK("filter3d_compute");
    return SYN3R_OK;
}
