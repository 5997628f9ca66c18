/*
 * syn3r_hip.h — C-ABI of libsyn3r_hip.so: the MI355X (gfx950) hot path of SYN3R.
 *
 * The reference (DecaYale/SYN3R) is pure Python; it has no FFI of its own
 * (SURVEY.md §8b).  Every entry point below states which reference Python
 * function (file:line under /root/reference) it replaces.  A maintainer binds
 * these with ctypes (INTEGRATION.md shows the stubs); syn3r_amd/_lib.py is that
 * binding for this repo.
 *
 * Conventions
 *   - extern "C", plain pointers + sizes, no torch types.
 *   - every pointer is a DEVICE pointer unless the parameter is documented
 *     "host"; small matrices (4x4 poses, 3x3 intrinsics) are passed BY VALUE
 *     through host pointers and copied into kernel arguments.
 *   - the caller owns every buffer; the library never allocates or frees
 *     user tensors.  Scratch comes from a caller-provided workspace whose size
 *     is returned by the matching *_workspace_bytes query.
 *   - every call is asynchronous on the hipStream_t passed as `stream`
 *     (a void* here so that the header needs no HIP include).
 *   - return value: 0 = ok, negative = error (SYN3R_E_*); the message is
 *     available from syn3r_last_error() (thread-local).
 *   - no process-wide settings: the library reads no environment variable and keeps no mutable state
 *     shared between host threads that changes what a call computes or which kernel it launches.  What
 *     state there is: the thread-local error string, the per-thread test hook and split-K workspace
 *     (syn3r_gemm_set_tile, syn3r_gemm_set_splitk_workspace), the opt-in tracer (syn3r_trace_*), handles
 *     the caller creates (syn3r_unet_create), and per-device launch attributes set on first use.
 */
#ifndef SYN3R_HIP_H
#define SYN3R_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYN3R_OK 0
#define SYN3R_E_INVALID (-1)   /* bad argument (null pointer, non-positive size, unsupported mode) */
#define SYN3R_E_WORKSPACE (-2) /* workspace too small */
#define SYN3R_E_HIP (-3)       /* a HIP runtime call failed */

/* dtype tags for entry points that accept fp16 or fp32 activations */
#define SYN3R_F32 0
#define SYN3R_F16 1

const char* syn3r_last_error(void);
/* library/ABI version: major*10000 + minor*100 + patch */
int syn3r_version(void);
/* name of the GPU architecture the code objects were built for ("gfx950") */
const char* syn3r_arch(void);

/*
 * Per-kernel timing for bench.py's roofline line: while enabled, every kernel
 * launch is bracketed by HIP events recorded on the launch stream.
 * syn3r_trace_report synchronises them, writes one "kernel calls total_ms"
 * line per kernel into buf and clears the trace.  on = 2 additionally puts
 * the contraction shape into the kernel name (per-shape tuning tables).
 * The switch, the filter and the recorded spans form a SESSION owned by the
 * thread that called syn3r_trace_enable; there is no process-wide switch.
 * Another thread records into that session only after syn3r_trace_attach
 * (session) with the pointer syn3r_trace_session() returned on the owner
 * (NULL detaches) - e.g. PyTorch's autograd thread around a backward launch.
 * syn3r_trace_report reports the calling thread's own session.
 */
int syn3r_trace_enable(int on);
void* syn3r_trace_session(void);
int syn3r_trace_attach(void* session);
/* restrict the tracer to kernels whose name contains one of the comma-separated substrings ("" = all):
 * two event records per launch cost a few microseconds, which matters for 30-microsecond kernels */
int syn3r_trace_filter(const char* substrings);
int syn3r_trace_report(char* buf, size_t cap);

/* ------------------------------------------------------------------------
 * Geometry (solver_utils/)
 * ------------------------------------------------------------------------ */

/*
 * inverse_warp + consistency_check_with_depth, fused.
 * Replaces solver_utils/forward_warp.py:187-279 (inverse_warp) and the
 * consistency.py:44-91 call it makes at forward_warp.py:257.
 *
 * Batched over `nb` target views that share one source view:
 *   img          [3,H,W]   f32  source image (closest view)
 *   depth        [H,W]     f32  source depth
 *   depth_pseudo [nb,H,W]  f32  target-view depths
 *   pose12       host [nb,16] f32 row-major  pose1 @ inverse(pose2)   (forward_warp.py:217)
 *   pose21       host [nb,16] f32 row-major  pose2 @ inverse(pose1)   (consistency.py:37 on the way back)
 *   K, Kinv      host [9] f32 row-major      intrinsics and torch.inverse(K) (consistency.py:21)
 *   bandwidth    reprojection bandwidth (20 or 10 in the reference)
 * Outputs (all [nb,...]):
 *   warped_img [nb,3,H,W] f32, warped_depth [nb,H,W] f32,
 *   mask_warp, mask_depth, mask, mask_inv, mask_depth_strict, mask_reproj : [nb,H,W] u8 (0/1, = torch.bool)
 *   warped_masked_img [nb,3,H,W] f32, soft_mask_reproj [nb,H,W] f32,
 *   reproj_error [nb,H,W] f32 (may be NULL; the reference does not return it)
 * workspace: syn3r_inverse_warp_workspace_bytes(nb) bytes (min/max slots).
 */
size_t syn3r_inverse_warp_workspace_bytes(int nb);
int syn3r_inverse_warp(const float* img, const float* depth, const float* depth_pseudo,
                       const float* pose12, const float* pose21, const float* K, const float* Kinv,
                       float bandwidth, int nb, int H, int W,
                       float* warped_img, float* warped_depth, uint8_t* mask_warp, uint8_t* mask_depth,
                       uint8_t* mask, float* warped_masked_img, uint8_t* mask_inv,
                       uint8_t* mask_depth_strict, uint8_t* mask_reproj, float* soft_mask_reproj,
                       float* reproj_error, void* workspace, size_t workspace_bytes, void* stream);

/*
 * consistency_check_with_depth alone (solver_utils/consistency.py:44-91).
 *   T12 = pose2 @ inverse(pose1), T21 = pose1 @ inverse(pose2) (host, [16] f32 row-major)
 *   K1inv = inverse(K1); K1, K2 host [9].
 *   depth1, depth2 [H,W] f32 -> err [H,W] f32
 */
int syn3r_reproj_error(const float* depth1, const float* depth2, const float* T12, const float* T21,
                       const float* K1, const float* K1inv, const float* K2, int H, int W, float* err,
                       void* stream);

/*
 * Orchestrator post-processing of a batch of inverse warps, on the device.
 * Replaces the per-frame host code of `warp_images_bw` (model/diffusionGS.py:1447-1483): binary mask
 * 1 - mask_reproj >= 0.5, cv2.dilate 5x5 (default border), cond = uint8(warped * (1 - ero)) / 255 (the uint8
 * round trip of :1469,1475), the (h, H/h, w, W/w) block-mean pooling of the hard mask (threshold 0.2) and of
 * the soft reprojection uncertainty 1 - soft_mask_reproj.
 *   mask_reproj [n,H,W] u8, warped_img [n,3,H,W] f32 (0..255), soft_mask_reproj [n,H,W] f32 (outputs of
 *   syn3r_inverse_warp) -> ero [n,H,W] u8 (0/1), cond_image, cond_ori [n,H,W,3] f32, soft [n,H,W] f32,
 *   masks, soft_pool [n,h,w] f32.  H % h == 0, W % w == 0.
 */
int syn3r_warp_post(const uint8_t* mask_reproj, const float* warped_img, const float* soft_mask_reproj,
                    int n, int H, int W, int h, int w, uint8_t* ero, float* cond_image, float* cond_ori,
                    float* soft, float* masks, float* soft_pool, void* stream);

/*
 * Uncertainty fusion + condition-image selection (model/diffusionGS.py:821-862):
 *   conf = exp(-(|cond_ori - gs|_2 / 0.5)^3) * (sum_c cond_ori > 0);  u = 1 - conf * (1 - soft);
 *   cond_image = clip(u > 0.5 ? gs : cond_ori, 0, 1);  masks = block mean of u.
 *   cond_ori, gs_images [n,H,W,3] f32, soft [n,H,W] f32 -> uncertainty [n,H,W], cond_image [n,H,W,3], masks [n,h,w].
 */
int syn3r_fuse_uncertainty(const float* cond_ori, const float* gs_images, const float* soft, int n, int H, int W,
                           int h, int w, float* uncertainty, float* cond_image, float* masks, void* stream);

/*
 * forward_warp: depth-weighted bilinear splat.
 * Replaces solver_utils/forward_warp.py:141-182 (forward_warp),
 * :7-38 (compute_transformed_points) and :42-127 (bilinear_splatting).
 * float64 throughout, as the numpy reference.
 *   frame1 [H,W,3] f64 (0..255), mask1 [H,W] u8 or NULL, depth1 [H,W] f64
 *   T host [16] f64 = transformation2 @ inv(transformation1); K1inv, K2 host [9] f64
 * Outputs: warped [H,W,3] u8, mask2 [H,W] u8, flow12 [H,W,2] f64
 * workspace: syn3r_forward_warp_workspace_bytes(H,W) (f64 accumulators (H+2)x(W+2)x4 + scalars).
 * Accumulation uses f64 hardware atomics (order-dependent in the last bits; the
 * u8 output is insensitive to that except at exact .5 ties).
 */
size_t syn3r_forward_warp_workspace_bytes(int H, int W);
int syn3r_forward_warp(const double* frame1, const uint8_t* mask1, const double* depth1, const double* T,
                       const double* K1inv, const double* K2, int H, int W, uint8_t* warped, uint8_t* mask2,
                       double* flow12, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Modified Euler scheduler (diffusers/schedulers/scheduling_euler_discrete.py)
 * ------------------------------------------------------------------------ */

/*
 * step_interp (scheduling_euler_discrete.py:633-814), fused:
 * v-prediction x0, per-frame quantile mask (radix select instead of the
 * reference's full sort + host sync), closed-form guidance gradient
 * (SURVEY.md §8a S2), Euler update.
 *   model_output [F,C,h,w]  vdtype (SYN3R_F16 / SYN3R_F32)
 *   sample       [F,C,h,w]  sdtype (upcast to f32 as :711)
 *   cond         [F,C,h,w]  f32 = temp_cond_latents[1]
 *   mask         [F-2,C,h,w] f32 (the reference's `mask`; valid = (1-mask)>0.5)
 *   lambda_row   host [F] f64 = lambda_ts[step_i]  (F <= 64)
 *   sigma f32 = sigmas[step_i]; dt f32 = sigmas[step_i+1] - sigma (:800)
 *   c_out f32 = -sigma/(sigma^2+1)^0.5, denom f32 = sigma^2+1, sqrt_sigma f32 = sigma^0.5,
 *                 all computed by the caller with the reference's own 0-dim fp32
 *                 CPU tensor arithmetic (:728,:792) so that the roundings agree
 * Outputs:
 *   prev_sample [F,C,h,w] vdtype; pred_x0 [F,C,h,w] f32 (may be NULL);
 *   grad [F,C,h,w] f32 (only when compute_grad; else may be NULL)
 * workspace: syn3r_step_workspace_bytes(F,C,h,w).
 */
size_t syn3r_step_workspace_bytes(int F, int C, int h, int w);
int syn3r_step_interp(const void* model_output, int vdtype, const void* sample, int sdtype,
                      const float* cond, const float* mask, const double* lambda_row, float sigma,
                      float dt, float c_out, float denom, float sqrt_sigma, float lr, int compute_grad,
                      void* prev_sample, float* pred_x0, float* grad, int F, int C, int h, int w,
                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * step_interp_prob_uncertain (scheduling_euler_discrete.py:1343-1515):
 * same quantile, soft replacement of x0 by the conditioning latents, first
 * and last frame hard-set, Euler update.  Arguments as syn3r_step_interp.
 */
int syn3r_step_replace(const void* model_output, int vdtype, const void* sample, int sdtype,
                       const float* cond, const float* mask, const double* lambda_row, float sigma,
                       float dt, float c_out, float denom, void* prev_sample, float* pred_x0,
                       int F, int C, int h, int w, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Gaussian rasteriser (diff-gaussian-rasterization-confidence)
 *
 * The reference consumes it through gsTrainer.render_view(cam) ->
 * {'render','depth','alpha'} (model/diffusionGS.py:154,166) and differentiates
 * it inside gsTrainer.training()/finetune() (:139,1640).  Its CUDA source is an
 * un-vendored submodule: these entry points follow the
 * published 3DGS rasteriser interface (forward: preprocess + tile binning +
 * radix sort + blend; backward: blend backward + preprocess backward).
 *
 * Layouts: means3D [N,3], scales [N,3], rotations [N,4] (r,x,y,z), opacities [N],
 * shs [N,sh_coeffs,3], confidence [N] or NULL (=1); all f32, device.
 * viewmatrix / projmatrix: host [16] f32, column-major (the transposed
 * world_view_transform / full_proj_transform of FSGS cameras); campos host [3].
 * State buffers (geom, binning, image) are caller-owned byte buffers sized by
 * the *_bytes queries; they carry the forward's intermediates to the backward.
 * They need not be initialised: stage 1 clears what the later stages accumulate
 * into or test (the four header words of geom, whatever N is).
 * ------------------------------------------------------------------------ */
size_t syn3r_raster_geom_bytes(int N);
size_t syn3r_raster_image_bytes(int H, int W);
size_t syn3r_raster_binning_bytes(long long P);

/*
 * Stage 1: project every Gaussian and count the tiles it touches (shapes that
 * take stage 2's pair-sort path also argsort the Gaussians by depth here).
 * radii [N] i32 out.  If num_rendered_host != NULL the
 * number of (Gaussian, tile) pairs P is summed, copied to it and the stream is
 * synchronised (the reference implementation performs the same device->host
 * read to size its binning buffers); with NULL nothing synchronises and stage 2
 * counts the pairs on the device against the capacity it is given.
 */
int syn3r_raster_preprocess(int N, int sh_degree, int sh_coeffs, const float* means3D, const float* scales,
                            const float* rotations, const float* opacities, const float* shs,
                            const float* confidence, float scale_modifier, const float* viewmatrix,
                            const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H,
                            int W, int* radii, void* geom, size_t geom_bytes, long long* num_rendered_host,
                            void* stream);
/*
 * The same stage on the trainer's PARAMETERS: log_scales [N,3], raw_rotations [N,4] (unnormalised), opacity_logits [N] - the
 * published activations (exp / normalize / sigmoid: GaussianModel.get_scaling / get_rotation / get_opacity, applied before every
 * render inside gsTrainer.training() / finetune(), model/diffusionGS.py:139,1640) happen inside the projection kernel, in
 * syn3r_gaussian_activate's arithmetic: bit for bit the state syn3r_gaussian_activate + syn3r_raster_preprocess leave, one launch
 * and three intermediate tensors less per training iteration.  Pair it with syn3r_raster_backward_raw.
 */
int syn3r_raster_preprocess_raw(int N, int sh_degree, int sh_coeffs, const float* means3D, const float* log_scales,
                                const float* raw_rotations, const float* opacity_logits, const float* shs,
                                const float* confidence, float scale_modifier, const float* viewmatrix,
                                const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H,
                                int W, int* radii, void* geom, size_t geom_bytes, long long* num_rendered_host,
                                void* stream);

/*
 * Stage 2: the per-tile lists of Gaussians in depth order - entry for entry the
 * result of the published "duplicate (tile<<32 | depth) keys, sort, find tile
 * ranges", built here by filtering the Gaussians through super-tiles of 4x4 or
 * 8x8 tiles (whose short lists are sorted by (depth bits, index) in LDS) and then
 * per tile (csrc/raster_bin.hip; images with more than 512 super-tiles take the
 * argsort + pair sort) - then the blend.  P is the pair CAPACITY of
 * `binning` (an estimate is fine: a list that does not fit sets the overflow
 * flag in the geometry header and is truncated, never written past the buffer).
 * bg host [3].  out_color [3,H,W], out_depth [1,H,W] (sum of alpha*T*z),
 * out_alpha [1,H,W] (1 - final transmittance).  *point_list_out (host pointer
 * to a device pointer, may be NULL) receives the sorted Gaussian-index list
 * inside `binning`, needed by the backward.
 */
int syn3r_raster_render(int N, int H, int W, const float* bg, const int* radii, void* geom, size_t geom_bytes,
                        void* binning, size_t binning_bytes, void* image, size_t image_bytes, long long P,
                        float* out_color, float* out_depth, float* out_alpha, unsigned** point_list_out,
                        void* stream);

/*
 * Backward of both stages.  dL_dcolor [3,H,W]; dL_ddepth, dL_dalpha [H,W] or NULL.
 * Outputs: dL_dmeans3D [N,3], dL_dscales [N,3], dL_drotations [N,4],
 * dL_dopacities [N], dL_dshs [N,sh_coeffs,3], dL_dmeans2D [N,3] (NDC-space
 * gradient of the projected mean, used by densification), dL_dconfidence [N] or NULL.
 */
size_t syn3r_raster_backward_workspace_bytes(int N);
int syn3r_raster_backward(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                          const float* scales, const float* rotations, const float* opacities, const float* shs,
                          const float* confidence, float scale_modifier, const float* viewmatrix,
                          const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H, int W,
                          const float* bg, const int* radii, void* geom, size_t geom_bytes,
                          const unsigned* point_list, void* image, size_t image_bytes, const float* dL_dcolor,
                          const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans3D, float* dL_dscales,
                          float* dL_drotations, float* dL_dopacities, float* dL_dshs, float* dL_dmeans2D,
                          float* dL_dconfidence, void* workspace, size_t workspace_bytes, void* stream);
/*
 * Backward of a forward that started with syn3r_raster_preprocess_raw: the same three parameter tensors in, the gradients
 * with respect to THEM out (syn3r_gaussian_activate_backward's chain rule applied where the activated gradients are formed:
 * d_log_scales = d_scales * scales, d_raw_rotations = (g - qhat (qhat . g)) / max(|q|, 1e-12), d_logits = d_opacities * s (1 - s);
 * the same bits as syn3r_raster_backward followed by syn3r_gaussian_activate_backward).
 */
int syn3r_raster_backward_raw(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                              const float* log_scales, const float* raw_rotations, const float* opacity_logits,
                              const float* shs, const float* confidence, float scale_modifier, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H, int W,
                              const float* bg, const int* radii, void* geom, size_t geom_bytes,
                              const unsigned* point_list, void* image, size_t image_bytes, const float* dL_dcolor,
                              const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans3D, float* dL_dlog_scales,
                              float* dL_draw_rotations, float* dL_dopacity_logits, float* dL_dshs, float* dL_dmeans2D,
                              float* dL_dconfidence, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Rendering modes of the projection stage: syn3r_raster_preprocess_ex / syn3r_raster_backward_ex carry them in `flags`.
 * Any other bit is rejected (SYN3R_E_INVALID, message in syn3r_last_error(), nothing launched).
 *
 * SYN3R_RASTER_ANTIALIAS - anti-aliased splatting.  With (a, b; b, c) the projected 2D covariance of a Gaussian before the
 * 0.3 px^2 dilation, h = 0.3, A = a + h, C = c + h, d0 = a c - b^2, d1 = A C - b^2, r = d0 / d1 and
 *     rho = sqrt(max(r, 0.000025)),
 * the opacity the blend multiplies is opacity * rho * confidence instead of opacity * confidence: the dilation no longer adds
 * energy, a splat deposits (up to the floor) the alpha of its undilated footprint whatever its size on screen.  Conic, radius,
 * tile rectangle, depth key and colour are untouched, so radii and the tile lists are those of a render without the flag.
 * Backward, G = dL/d(blend opacity): dL/dopacity = G confidence rho (then the sigmoid's chain rule on the raw route),
 * dL/dconfidence = G opacity rho, dL/drho = G opacity confidence, dL/dr = dL/drho / (2 rho) if r > 0.000025 else 0, and
 *     dr/da = (c d1 - C d0) / d1^2,  dr/dc = (a d1 - A d0) / d1^2,  dr/db = -2 b (d1 - d0) / d1^2
 * are added to the covariance gradients before they go on into the 3D covariance, the Jacobian, the mean, scales and rotations.
 * In fp32 d0 can cancel to zero or below for needle-shaped Gaussians: those sit on the floor (rho = 0.005, no gradient through
 * rho); nothing becomes NaN.  The geometry buffer holds the opacity WITHOUT rho; the backward forms rho again.
 * Provenance: the `antialiasing` switch of the published 3DGS rasteriser (GaussianRasterizationSettings.antialiasing), which is
 * the 2D Mip filter of Mip-Splatting (Yu et al., CVPR 2024).  The constants 0.3 and 0.000025 are RECALLED from the published
 * code, which is not available to check against: UNPINNED.  FSGS' confidence fork (the rasteriser the reference calls, not
 * vendored) is not known to have the filter: the flag is an option, and with flags = 0 every bit is what the four entries above
 * compute.
 */
#define SYN3R_RASTER_ANTIALIAS 1
/*
 * syn3r_raster_preprocess / syn3r_raster_preprocess_raw with rendering modes: `raw` = 0 takes the activated tensors (scales,
 * rotations, opacities), `raw` = 1 the trainer's parameters (log-scales, raw quaternions, logits) in the same three arguments;
 * `flags` = 0 or SYN3R_RASTER_ANTIALIAS (formula and provenance above).  The two old entries are this one with flags = 0.
 * The backward of the render MUST be syn3r_raster_backward_ex with the SAME `raw` and `flags`.
 */
int syn3r_raster_preprocess_ex(int N, int sh_degree, int sh_coeffs, const float* means3D, const float* scales,
                               const float* rotations, const float* opacities, const float* shs,
                               const float* confidence, float scale_modifier, const float* viewmatrix,
                               const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H,
                               int W, int* radii, void* geom, size_t geom_bytes, long long* num_rendered_host,
                               int raw, int flags, void* stream);
/*
 * syn3r_raster_backward / syn3r_raster_backward_raw with rendering modes; arguments as theirs, then `raw` and `flags` as
 * syn3r_raster_preprocess_ex.  `raw` and `flags` MUST be the ones the forward of this render was given: with
 * SYN3R_RASTER_ANTIALIAS the gradients of opacity, confidence, means, scales and rotations carry the rho terms above, and the
 * state buffers do not record which mode wrote them.  The two old entries are this one with flags = 0.
 */
int syn3r_raster_backward_ex(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                             const float* scales, const float* rotations, const float* opacities, const float* shs,
                             const float* confidence, float scale_modifier, const float* viewmatrix,
                             const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H, int W,
                             const float* bg, const int* radii, void* geom, size_t geom_bytes,
                             const unsigned* point_list, void* image, size_t image_bytes, const float* dL_dcolor,
                             const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans3D, float* dL_dscales,
                             float* dL_drotations, float* dL_dopacities, float* dL_dshs, float* dL_dmeans2D,
                             float* dL_dconfidence, void* workspace, size_t workspace_bytes, int raw, int flags,
                             void* stream);

/*
 * 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024, section 4.1), the other half of the method next to
 * SYN3R_RASTER_ANTIALIAS: every Gaussian is bounded from below by the sampling rate of the cameras that trained it, so that a
 * render from closer than any training view shows no needles or holes.
 *
 * syn3r_filter3d_compute - the per-Gaussian filter.  xyz [n,3]; cams [n_cams,16] DEVICE floats, per camera the 12 entries of the
 * world-to-view matrix [R | t] row by row (x = c0 px + c1 py + c2 pz + c3, y from c4..c7, z from c8..c11), then fx, fy, W, H in
 * pixels.  Camera c SEES Gaussian k iff z > near and (fx x / z + W / 2, fy y / z + H / 2) lies in [-margin W, (1 + margin) W] x
 * [-margin H, (1 + margin) H].  The sampling rate is nu_k = max over the seeing cameras of fx / z (the paper's Eq. 6; the released
 * code's min depth / max focal when all focal lengths agree) and
 *     filter_out[k] = sqrt(variance) / nu_k.
 * A Gaussian no camera sees gets the LARGEST filter among the seen ones (the released code's rule); if none is seen at all every
 * filter is 0.  Never NaN or inf for finite inputs.  variance = 0.2, near = 0.2, margin = 0.15 are RECALLED from the released
 * Mip-Splatting code (compute_3D_filter), which is not available to check against: UNPINNED, hence arguments.
 * ws: syn3r_filter3d_workspace_bytes(n) bytes of device scratch (0 for n outside 1 .. 2^24).  Two launches and a 4-byte memset on
 * `stream`; no host read, no synchronisation.  Rejected on the host before any HIP call: null pointers, n or n_cams outside
 * 1 .. 2^24, variance / near not positive, margin negative (SYN3R_E_INVALID), a short workspace (SYN3R_E_WORKSPACE).
 */
size_t syn3r_filter3d_workspace_bytes(int n);
int syn3r_filter3d_compute(const float* xyz, int n, const float* cams, int n_cams, float variance, float near, float margin,
                           float* filter_out, void* ws, size_t ws_bytes, void* stream);
/*
 * syn3r_raster_preprocess_ex with the filter: arguments as there, then `filter3d` ([N] device floats >= 0, or NULL) before the
 * stream.  NULL is syn3r_raster_preprocess_ex bit for bit; `raw` and `flags` are validated exactly as there.  With a filter f and the
 * ACTIVATED scales s_i (raw = 1: after the exp) the Gaussian is rendered with
 *     q_i = sqrt(s_i^2 + f^2)   (the covariance is built from scale_modifier q_i)   and   coef = prod_i s_i / q_i
 * on its opacity: the blend multiplies opacity * coef * confidence, with SYN3R_RASTER_ANTIALIAS opacity * coef * rho * confidence
 * where rho comes from the FILTERED covariance.  coef = sqrt(det Sigma / det(Sigma + f^2 I)) is formed as the product of the three
 * ratios, so a scale of 1e-6 under a filter of 1e-2 is 1e-12, not a NaN.  Radii, tile lists and depth keys are those of the
 * filtered Gaussian and differ from an unfiltered render; the geometry buffer holds the opacity WITHOUT coef (and without rho).
 */
int syn3r_raster_preprocess_f3d(int N, int sh_degree, int sh_coeffs, const float* means3D, const float* scales,
                                const float* rotations, const float* opacities, const float* shs,
                                const float* confidence, float scale_modifier, const float* viewmatrix,
                                const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H,
                                int W, int* radii, void* geom, size_t geom_bytes, long long* num_rendered_host,
                                int raw, int flags, const float* filter3d, void* stream);
/*
 * syn3r_raster_backward_ex with the filter; `raw`, `flags` and `filter3d` MUST be the forward's (NULL: syn3r_raster_backward_ex
 * bit for bit).  With G = dL/d(blend opacity): dL/dopacity = G coef [rho] confidence, dL/dconfidence = G opacity coef [rho], the
 * rho terms of SYN3R_RASTER_ANTIALIAS carry coef, and
 *     dL/ds_i = dL/dq_i s_i / q_i + G opacity confidence [rho] coef f^2 / (s_i q_i^2),
 * evaluated without the division by s_i (raw = 1: dL/dlog s_i = dL/dq_i s_i^2 / q_i + G opacity confidence [rho] coef f^2 / q_i^2).
 * coef is formed again with the forward's arithmetic.  The filter receives no gradient.
 */
int syn3r_raster_backward_f3d(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                              const float* scales, const float* rotations, const float* opacities, const float* shs,
                              const float* confidence, float scale_modifier, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H, int W,
                              const float* bg, const int* radii, void* geom, size_t geom_bytes,
                              const unsigned* point_list, void* image, size_t image_bytes, const float* dL_dcolor,
                              const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans3D, float* dL_dscales,
                              float* dL_drotations, float* dL_dopacities, float* dL_dshs, float* dL_dmeans2D,
                              float* dL_dconfidence, void* workspace, size_t workspace_bytes, int raw, int flags,
                              const float* filter3d, void* stream);
/*
 * syn3r_raster_backward_f3d with the ABSOLUTE screen-space gradient of AbsGS (Ye et al., "AbsGS: Recovering Fine Details for 3D
 * Gaussian Splatting", 2024, section 3.2; `dL_dmean2D_abs` of its released rasteriser and gsplat's `absgrad` - both RECALLED, not
 * available to check against: UNPINNED).  Arguments as there, then `dL_dmeans2D_abs` ([N,2] device floats, 8-byte aligned, or NULL)
 * before the stream; NULL is syn3r_raster_backward_f3d exactly (the same kernels, the same number of launches).  Per pixel p that
 * blends Gaussian i the gradient of the loss with respect to the projected mean is g_p = (gx_p, gy_p); dL_dmeans2D[i, :2] is
 * sum_p g_p, in which the pulls of the pixels on either side of a large Gaussian cancel, and
 *     dL_dmeans2D_abs[i] = (sum_p |gx_p|, sum_p |gy_p|)
 * in the same units (NDC: the factors W / 2 and H / 2 applied).  It is summed inside the blend backward (two spare slots of the
 * gradient record: syn3r_raster_backward_workspace_bytes does not change), on both parameter routes (`raw`) and in every mode
 * (`flags`, `filter3d`: the blend opacity carries rho and coef); culled Gaussians (radii <= 0) receive zeros.  The other outputs
 * are those of syn3r_raster_backward_f3d up to the order of the float atomics.  One small launch more than without it.
 */
int syn3r_raster_backward_abs(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                              const float* scales, const float* rotations, const float* opacities, const float* shs,
                              const float* confidence, float scale_modifier, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H, int W,
                              const float* bg, const int* radii, void* geom, size_t geom_bytes,
                              const unsigned* point_list, void* image, size_t image_bytes, const float* dL_dcolor,
                              const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans3D, float* dL_dscales,
                              float* dL_drotations, float* dL_dopacities, float* dL_dshs, float* dL_dmeans2D,
                              float* dL_dconfidence, void* workspace, size_t workspace_bytes, int raw, int flags,
                              const float* filter3d, float* dL_dmeans2D_abs, void* stream);
/*
 * syn3r_raster_backward_abs with the gradient of the loss with respect to the CAMERA: an EXTENSION with no counterpart in the
 * reference or in the published rasteriser (gsplat's `pose_opt` and MonoGS differentiate their own parametrisations), for a trainer
 * that refines its camera poses.  Arguments as there, then `dL_dcamera` (35 device floats, or NULL) and `accumulate` before the
 * stream; NULL is syn3r_raster_backward_abs exactly (the same kernels, the same number of launches).  It composes with every mode
 * (`raw`, `flags`, `filter3d`, `dL_dmeans2D_abs` given or NULL) and leaves every other output as it is.
 * Layout: dL/dviewmatrix[16], dL/dprojmatrix[16], dL/dcampos[3], each in the storage order of its input (column-major 4 x 4, as
 * the render reads them).  The THREE INPUTS ARE TAKEN AS INDEPENDENT, exactly as the entry takes them: that projmatrix is a
 * projection times viewmatrix and campos the centre of viewmatrix is the caller's knowledge, and so is the chain rule through it
 * (syn3r_amd/gs/pose.py: tangent_from_raw).  viewmatrix enters through the view-space mean (EWA Jacobian, depth output) and through
 * its rotation part W in T = J W; projmatrix through the x, y and w rows of the clip-space mean; campos through the SH view
 * direction.  The slots the render never reads are exact zeros: view 3, 7, 11, 15 (fourth row) and proj 2, 6, 10, 14 (clip z).
 * Per Gaussian 27 terms are formed by a second launch of the projection backward compiled WITHOUT its stores (the per-Gaussian
 * outputs are written by the usual instance and are bit for bit those of syn3r_raster_backward_abs), summed per block without atomics
 * and added over the blocks in a fixed order with fp64 accumulators by a one-block kernel: the result is the same bits in every launch
 * for the same gradient records.  Two launches more than without it.  accumulate == 0 stores
 * it; accumulate != 0 adds it to what `dL_dcamera` holds, one fp32 add per slot (a trainer that sums several steps of one camera).
 * The workspace must hold syn3r_raster_backward_cam_workspace_bytes(N) when dL_dcamera is given (the size of the other entries plus
 * one 128-byte row per 256 Gaussians); with NULL syn3r_raster_backward_workspace_bytes(N) is enough.  P == 0: zeros.
 */
size_t syn3r_raster_backward_cam_workspace_bytes(int N);
int syn3r_raster_backward_cam(int N, int sh_degree, int sh_coeffs, long long P, const float* means3D,
                              const float* scales, const float* rotations, const float* opacities, const float* shs,
                              const float* confidence, float scale_modifier, const float* viewmatrix,
                              const float* projmatrix, const float* campos, float tanfovx, float tanfovy, int H, int W,
                              const float* bg, const int* radii, void* geom, size_t geom_bytes,
                              const unsigned* point_list, void* image, size_t image_bytes, const float* dL_dcolor,
                              const float* dL_ddepth, const float* dL_dalpha, float* dL_dmeans3D, float* dL_dscales,
                              float* dL_drotations, float* dL_dopacities, float* dL_dshs, float* dL_dmeans2D,
                              float* dL_dconfidence, void* workspace, size_t workspace_bytes, int raw, int flags,
                              const float* filter3d, float* dL_dmeans2D_abs, float* dL_dcamera, int accumulate,
                              void* stream);

/*
 * Stable LSD radix sort of (u64 key, u32 value) pairs on bits [0, nbits) — the
 * tile/depth sort of the rasteriser (cub::DeviceRadixSort::SortPairs in the
 * published implementation).  Ping-pongs between the two buffer pairs;
 * *result_in_tmp (host) tells which pair holds the sorted output.
 */
size_t syn3r_sort_pairs_workspace_bytes(long long n);
int syn3r_sort_pairs(unsigned long long* keys, unsigned* vals, unsigned long long* keys_tmp, unsigned* vals_tmp,
                     long long n, int nbits, void* workspace, size_t workspace_bytes, int* result_in_tmp,
                     void* stream);

/* ------------------------------------------------------------------------
 * SVD spatio-temporal UNet operators (fp16 storage, fp32 accumulation)
 *
 * Activations are channels-last token matrices: a tensor the reference holds as
 * [B*F, C, h, w] (or [B, C, F, h, w]) is the row-major fp16 matrix
 * [B*F*h*w, C] with row = ((b*F + f)*h + y)*w + x.  With that layout every
 * permute/reshape of the reference's forward
 * (diffusers/models/unets/unet_spatio_temporal_condition.py:356-489,
 * resnet.py:691-721, transformers/transformer_temporal.py:277-379,
 * attention.py:478-533) is an index calculation inside a kernel.
 * ------------------------------------------------------------------------ */

/*
 * out[M,N] = s_acc*(A[M,K] . W[N,K]^T + bias[n] + rowvec[m / rows_per_vec, n])
 *            + s_res*residual[m,n] + s_aux*aux[m,n]
 * nn.Linear / 1x1 convolutions (attention_processor.py:187-202, resnet.py:316,
 * transformer_temporal.py:236,273) with the adds that follow them fused.
 * W is the nn.Linear weight as stored ([out_features, in_features]).
 * rows_per_vec = -P selects rowvec[m mod P] instead (the batch-interleaved context of the temporal
 * cross-attention, transformer_temporal.py:310-317, for a batch of P).  rv_group_rows = G > 0 (with
 * rows_per_vec < 0): the rows come in groups of G, each emulating a SEPARATE batch-of-P call of the reference:
 * row m adds rowvec[(m / G) * P + m mod P] (the forward- and backward-in-time passes of a denoising step,
 * SVD_2pass_prob_uncertain.py:661-742, in one launch).  rv_group_rows = 0: one group.
 * K % 64 == 0; strides in elements, multiples of 8; pointers 16-byte aligned;
 * bias / rowvec / residual / aux may be NULL.
 * gn_partials / gn_partials_bytes / gn_written (host, may be NULL): GroupNorm partial sums of the output, see
 * "GroupNorm statistics out of the PRODUCER's epilogue" below; (NULL, 0, NULL) = no request.
 */
int syn3r_gemm_f16(const void* A, long long lda, const void* W, void* out, long long ldc, const void* bias,
                   const void* rowvec, long long ldrv, int rows_per_vec, int rv_group_rows, const void* residual, long long ldr,
                   const void* aux, long long ldaux, float s_acc, float s_res, float s_aux, int M, int N, int K,
                   void* gn_partials, size_t gn_partials_bytes, int* gn_written, void* stream);

/* out[M,N] = [A1 | A2][M, K1+K2] . W[N, K1+K2]^T + bias: the contraction reads the two halves of a channel concatenation
 * in place (resnet.py:316 conv_shortcut applied to torch.cat([hidden, skip], dim=1), unet_3d_blocks.py up blocks), so the
 * concatenated tensor is never written.  K1, K2 % 64 == 0; served by the persistent 256 x 320 kernel only:
 * syn3r_gemm_2src_supported() != 0 is the admission test (otherwise concatenate and call syn3r_gemm_f16).
 * gn_partials / gn_partials_bytes / gn_written: as for syn3r_gemm_f16. */
int syn3r_gemm_2src_supported(int M, int N, int K1, int K2, long long lda1, long long lda2);
int syn3r_gemm_2src_f16(const void* A1, long long lda1, int K1, const void* A2, long long lda2, int K2, const void* W,
                        void* out, long long ldc, const void* bias, int M, int N, void* gn_partials, size_t gn_partials_bytes,
                        int* gn_written, void* stream);

/* Test / tuning hook, PER CALLING THREAD (thread-local: the library holds no state shared between host threads): the
 * contraction kernel family this thread's next launches use.  0 = chosen per shape (default); -128 / -256 = the 160-column
 * LDS-DMA kernel of that block height; -320 = the persistent 256 x 320 kernel wherever it admits the shape; -322 = the
 * software-pipelined persistent 256 x 320 kernel (dense, two-source and implicit-GEMM convolution modes) wherever it admits
 * the shape.  This hook and the split-K workspace below are the library's only settings, both per calling thread; it reads no
 * environment variable (dispatch switches for A/B measurements exist in -DSYN3R_TUNING developer builds only).  They stay
 * per-thread settings rather than arguments: the hook has to reach launches made deep inside a host's operators, and the
 * workspace is set once per forward, not per launch. */
int syn3r_gemm_set_tile(int bm);

/* Split-K scratch, PER CALLING THREAD (round 4).  With a workspace set, the contractions (syn3r_gemm_f16, syn3r_gemm_2src_f16
 * when no part would straddle K1, net.2 of syn3r_feedforward_f16, syn3r_conv2d3x3_f16, syn3r_tconv3_f16) whose tile grid would leave more than half of the CUs idle (level 3 of the SVD UNet at F = 14: 4 032 rows) run
 * as two or four equal K parts - one block per (tile, part), fp32 partial tiles in the workspace - followed by a small
 * launch that sums the parts IN ORDER and applies the epilogue (same arithmetic as the one-pass epilogue; the fp32 sum is
 * associated differently, so results differ from the one-pass launch in the last bits).  Up to 4 * M * N * 4 bytes are used per launch
 * (a launch that needs more runs in one pass); the workspace must stay valid until the launches that used it have completed and
 * must not be shared by launches in flight on different streams.  (NULL, 0) turns split-K off (the default). */
int syn3r_gemm_set_splitk_workspace(void* workspace, size_t bytes);

/*
 * FeedForward's first projection fused with its GEGLU gate (attention.py:608-665, activations.py GEGLU):
 * out[M,D] = h * gelu_erf(g) with [h | g] = A[M,K] . W[2D,K]^T + bias, h and g rounded to fp16 first as
 * the reference's projection output is.  Wpacked / bias_packed hold the rows of W regrouped per tile of
 * 80 output columns as [80 hidden rows | 80 gate rows] (zero rows past D): ceil(D/80)*160 rows
 * (syn3r_amd.unet.ops.pack_geglu).
 */
int syn3r_gemm_geglu_f16(const void* A, long long lda, const void* Wpacked, const void* bias_packed, void* out,
                         long long ldc, int M, int D, int K, void* stream);

/*
 * FeedForward(dim, activation_fn="geglu").forward (diffusers attention.py:608-665, activations.py GEGLU): 
 *   out = s_acc * (geglu(x @ W1^T + b1) @ W2^T + b2) + s_res * residual + s_aux * aux
 * in two launches (syn3r_gemm_geglu_f16, syn3r_gemm_f16) whose intermediate, the gated hidden activation
 * [M, D], lives in `workspace` in a tiled layout ([ceil(M/128)][D/64][128][64]: the second projection reads its A
 * operand as contiguous 16 KB tile images instead of rows at a multi-KB pitch).
 *   x [M, C_in] (row stride ldx); w1_packed / b1_packed: GEGLU packing of syn3r_gemm_geglu_f16 ([80 hidden | 80 gate]
 *   row groups); D = hidden width (multiple of 64); w2 [C_out, D]; b2 [C_out] or NULL; residual / aux [M, C_out] or NULL.
 */
size_t syn3r_feedforward_workspace_bytes(int M, int D);
int syn3r_feedforward_f16(const void* x, long long ldx, const void* w1_packed, const void* b1_packed, int D,
                          const void* w2, const void* b2, void* out, long long ldc, const void* residual,
                          long long ldr, const void* aux, long long ldaux, float s_acc, float s_res, float s_aux,
                          int M, int C_in, int C_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * syn3r_feedforward_f16 with net.0 on the persistent 256 x 256 tile (round 6, k_gemm_g256: a second look-ahead stage for the
 * A operand, LDS-free epilogue into the tiled hidden activation; attention.py:608-665, activations.py GEGLU).
 *   w1_packed64 / b1_packed64: the rows of net.0.proj regrouped per 64-wide hidden chunk j as [hidden 64j..64j+63 | gate
 *   64j..64j+63] ([2 D, C_in] / [2 D]).  Shapes: syn3r_feedforward_p64_supported(M, D, C_in) (M % 128 == 0, M >= 256,
 *   D % 128 == 0, C_in >= 128 a multiple of 64), x with dense rows (ldx == C_in); everything else as syn3r_feedforward_f16,
 *   whose results it reproduces bit for bit (same accumulation order, same gate).
 */
int syn3r_feedforward_p64_supported(int M, int D, int C_in);
int syn3r_feedforward_p64_f16(const void* x, long long ldx, const void* w1_packed64, const void* b1_packed64, int D,
                              const void* w2, const void* b2, void* out, long long ldc, const void* residual,
                              long long ldr, const void* aux, long long ldaux, float s_acc, float s_res, float s_aux,
                              int M, int C_in, int C_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same FeedForward.forward (attention.py:608-665, GEGLU of activations.py) in ONE kernel for C_in = C_out = 320
 * (the level-0 transformer blocks of SVD): the gated hidden activation never leaves the CU, no workspace.
 *   w1_chunked [D/64][128][320]: rows of net.0.proj regrouped per 64-wide hidden chunk j as
 *       4 x [hidden 64j+16q..+15 | gate 64j+16q..+15], q = 0..3;  b1_chunked [D/64][128] likewise
 *   w2 [320, D] (net.2.weight as stored), b2 [320] or NULL; epilogue as syn3r_gemm_f16 (bias, residual, aux, scales).
 * Other channel counts are rejected (SYN3R_E_INVALID): use syn3r_feedforward_f16.
 */
int syn3r_feedforward_fused_f16(const void* x, long long ldx, const void* w1_chunked, const void* b1_chunked, int D,
                                const void* w2, const void* b2, void* out, long long ldc, const void* residual,
                                long long ldr, const void* aux, long long ldaux, float s_acc, float s_res, float s_aux,
                                int M, int C, void* stream);

/*
 * LayerNorm + FeedForward in that kernel: the `norm3(hidden_states)` -> `ff(...)` pair of BasicTransformerBlock.forward and
 * TemporalBasicTransformerBlock.forward (attention.py:376-392, 519-530) for C = 320.  x is the UN-normalised activation; the
 * kernel normalises its resident 128-row x tile with (ln_gamma, ln_beta [320], ln_eps) - fp32 statistics, the arithmetic and
 * summation order of syn3r_layernorm_f16, so the result equals syn3r_layernorm_f16 followed by syn3r_feedforward_fused_f16
 * bit for bit - and the normalised activation is never written to memory.  `residual` is typically x itself.
 */
int syn3r_feedforward_fused_ln_f16(const void* x, long long ldx, const void* ln_gamma, const void* ln_beta, float ln_eps,
                                   const void* w1_chunked, const void* b1_chunked, int D, const void* w2, const void* b2,
                                   void* out, long long ldc, const void* residual, long long ldr, const void* aux,
                                   long long ldaux, float s_acc, float s_res, float s_aux, int M, int C, void* stream);

/*
 * (hidden + add vector) -> LayerNorm -> FeedForward -> + (hidden + add vector) in that kernel: the head of
 * TemporalBasicTransformerBlock.forward for C = 320 (attention.py:500-517: `residual = hidden_states` after the frame-position
 * embedding was added by the caller, transformer_temporal.py:339; `norm_in`; `ff_in`; `+ residual`).  x is the activation BEFORE
 * the embedding is added, addvec [rows, 320] holds one embedding row per rows_per_vec consecutive rows of x.  The kernel adds the
 * vector to its resident x tile (an fp16 tensor add, rounded as the reference's), normalises it, and its epilogue adds the
 * same fp16 sum as the residual: bit for bit syn3r_layernorm_f16(x, addvec, want the sum) followed by syn3r_feedforward_fused_f16 with
 * that sum as the residual, without the two [M, 320] round trips.  aux / scales as syn3r_feedforward_fused_f16.
 */
int syn3r_feedforward_fused_addln_f16(const void* x, long long ldx, const void* addvec, int rows_per_vec, const void* ln_gamma,
                                      const void* ln_beta, float ln_eps, const void* w1_chunked, const void* b1_chunked, int D,
                                      const void* w2, const void* b2, void* out, long long ldc, const void* aux, long long ldaux,
                                      float s_acc, float s_res, float s_aux, int M, int C, void* stream);

/*
 * LayerNorm + bias-free projection in ONE kernel for C = 320: `norm1(hidden_states)` followed by `attn1.to_q / to_k / to_v`
 * (attention.py:340-352 and 509-512; attention_processor.py to_q / to_k / to_v, stored here as one [960, 320] matrix) of the
 * level-0 transformer blocks.  out [M, N] = LayerNorm(x [M, 320]; ln_gamma, ln_beta, ln_eps) . W[N, 320]^T, N a multiple of 320.
 * The x tile of a block stays on chip (normalised there with the arithmetic of syn3r_layernorm_f16, so the normalised values
 * are the ones that launch would have written), the normalised activation is never written to memory.  Same fp32 accumulation
 * order along K as syn3r_gemm_f16.  Other channel counts are rejected (SYN3R_E_INVALID): syn3r_layernorm_f16 + syn3r_gemm_f16.
 */
int syn3r_layernorm_linear320_f16(const void* x, long long ldx, const void* ln_gamma, const void* ln_beta, float ln_eps,
                                  const void* W, void* out, long long ldc, int M, int N, int C, void* stream);

/*
 * 3x3 Conv2d on NHWC fp16 (resnet.py:274,290; downsampling.py:116-148 with stride 2;
 * upsampling.py:172-183 with upsample != 0: nearest-2x of the input fused into the gather).
 * pad_lo = 1: padding 1 on every side.  pad_lo = 0: the VAE encoder's Downsample2D(padding=0), which pads
 * (0,1,0,1) — nothing before the first row/column, one zero row/column after the last (downsampling.py:140-143).
 * X [NB,Hi,Wi,Cin], W [Cout, 3, 3, Cin] (= the Conv2d weight permuted to OHWI), Cin % 64 == 0.
 * out [NB*Ho*Wo, Cout] with the gemm epilogue (aux excluded); Ho = (Hg + pad_lo - 2) / stride + 1.
 * gn_partials / gn_partials_bytes / gn_written: as for syn3r_gemm_f16 (M = NB*Ho*Wo, N = Cout).
 */
int syn3r_conv2d3x3_f16(const void* X, const void* W, void* out, long long ldc, const void* bias,
                        const void* rowvec, long long ldrv, int rows_per_vec, const void* residual, long long ldr,
                        float s_acc, float s_res, int NB, int Hi, int Wi, int Cin, int Cout, int stride, int upsample,
                        int pad_lo, void* gn_partials, size_t gn_partials_bytes, int* gn_written, void* stream);

/*
 * The same nearest-2x upsample + 3x3 convolution (upsampling.py:172-183) as FOUR 2x2 convolutions at input resolution, one per
 * output parity: after the upsample the 3x3 window of output pixel (2i + py, 2j + px) covers input pixels
 * (i + py - 1 + a, j + px - 1 + b), a, b in {0, 1}, and the nine taps collapse onto them with summed weights - K = 4 Cin instead
 * of 9 Cin.  The zero padding of the upsampled image falls on input row / column -1 or Hi / Wi: borders need no special weights.
 *
 * syn3r_pack_upsample4_f16 (pure host code, no GPU call; once per loaded model): w [Cout, 3, 3, Cin] fp16 (OHWI, as
 * syn3r_conv2d3x3_f16 takes it) -> w4 [4][Cout][2][2][Cin] fp16, phase p = 2 py + px.  Filter rows ty fall on block row a as
 * py = 0: {0} | {1, 2}, py = 1: {0, 1} | {2} (columns the same with px); a folded weight is the sum of its 1, 2 or 4 source taps
 * in fp32, in ascending (ty, tx) order, rounded once to fp16 (nearest even).  The result differs from the 9-tap form by that one
 * rounding of the weights (about 2e-4 relative rms of the output at UNet widths, under half an fp16 output step).
 *
 * syn3r_conv2d3x3_up4_f16: X [NB, Hi, Wi, Cin], w4 as packed, bias [Cout] or NULL -> out [NB, 2 Hi, 2 Wi, Cout] (dense rows of
 * Cout).  Accumulation in fp32 with k = (channel chunk of 64, tap) ascending, bias added, one rounding to fp16.  No row vector,
 * residual or aux: `residual` must be NULL (the 9-tap entry has the general epilogue).  Refused with SYN3R_E_INVALID and a
 * message: Cin % 64 != 0 (a k-tile is 64 channels of one tap; in particular every Cin % 16 != 0), Cout % 8 != 0,
 * NB Hi Wi >= 2^24, a non-NULL residual.  gn_partials / gn_partials_bytes / gn_written: as for syn3r_gemm_f16 with
 * M = 4 NB Hi Wi, N = Cout, written when also Hi Wi % 32 == 0; the 32-row block lb of phase p of image n is slot
 * (4 n + p) (Hi Wi / 32) + lb of the buffer - its rows are 32 pixels of ONE phase, not 32 consecutive output rows: every image
 * still owns 4 Hi Wi / 32 consecutive slots, which is all syn3r_groupnorm_pre_f16 (samples = images) relies on.
 */
int syn3r_pack_upsample4_f16(const void* w, void* w4, int Cout, int Cin);
int syn3r_conv2d3x3_up4_f16(const void* X, const void* w4, void* out, const void* bias, const void* residual, int NB, int Hi, int Wi,
                            int Cin, int Cout, void* gn_partials, size_t gn_partials_bytes, int* gn_written, void* stream);

/*
 * (3,1,1) Conv3d over frames, padding (1,0,0) (resnet.py:571-597) on [B,F,HW,Cin] fp16.
 * W [Cout, 3, Cin] (= the Conv3d weight [Cout,Cin,3,1,1] permuted), Cin % 64 == 0.
 * gn_partials / gn_partials_bytes / gn_written: as for syn3r_gemm_f16 (M = B*F*HW, N = Cout).
 */
int syn3r_tconv3_f16(const void* X, const void* W, void* out, long long ldc, const void* bias, const void* rowvec,
                     long long ldrv, int rows_per_vec, const void* residual, long long ldr, float s_acc, float s_res,
                     int B, int F, int HW, int Cin, int Cout, void* gn_partials, size_t gn_partials_bytes, int* gn_written,
                     void* stream);

/*
 * Self-attention over the S tokens of each of nseq sequences, head dim 64, scale 1/8
 * (F.scaled_dot_product_attention at attention_processor.py:1279).  q/k/v point at column 0 of
 * head 0 inside row-major matrices with row stride ld (e.g. the three thirds of a fused QKV
 * projection); out [nseq*S, ldo], head hd at columns [64 hd, 64 hd + 64).
 */
int syn3r_attention_f16(const void* q, const void* k, const void* v, long long ld, void* out, long long ldo,
                        int nseq, int S, int heads, void* stream);

/*
 * Temporal self-attention (attention.py:491-508): for every (b, pixel) the F <= 32 tokens at rows
 * (b*F + f)*HW + pixel attend to each other.  Same operand convention as syn3r_attention_f16.
 */
int syn3r_attention_temporal_f16(const void* q, const void* k, const void* v, long long ld, void* out,
                                 long long ldo, int B, int F, int HW, int heads, void* stream);

/*
 * GroupNorm(32 groups) [+ SiLU] on [samples, rows, C] fp16 (statistics per sample and group over
 * rows x C/32).  2D norms: samples = B*F, rows = h*w; the 3D norms of TemporalResnetBlock
 * (resnet.py:574,588): samples = B, rows = F*h*w.
 */
size_t syn3r_groupnorm_workspace_bytes(int samples, int rows);
int syn3r_groupnorm_f16(const void* x, void* y, int samples, int rows, int C, const void* gamma, const void* beta,
                        float eps, int silu, void* workspace, size_t workspace_bytes, void* stream);
/* The same on the channel concatenation [x1 (C1 channels) | x2 (C2 channels)] read in place (the norm1 of an up block's
 * resnet, resnet.py:272 on torch.cat([hidden, skip], dim=1)); y is [samples, rows, C1 + C2].  C1, C2 % 8 == 0. */
int syn3r_groupnorm_2src_f16(const void* x1, int C1, const void* x2, int C2, void* y, int samples, int rows,
                             const void* gamma, const void* beta, float eps, int silu, void* workspace,
                             size_t workspace_bytes, void* stream);
/*
 * GroupNorm statistics out of the PRODUCER's epilogue (round 6).  Every GroupNorm input of the UNet is the output of a
 * contraction (resnet.py:272,286,574,588: conv1 + temb -> norm2, conv2 + shortcut -> the temporal norm1, the AlphaBlender
 * output -> the next norm1; transformer_temporal.py:235), whose epilogue holds the values in registers: the statistics
 * pass over the activation (one full extra read) is not launched.
 *
 * The request and its answer are arguments of the producing call: syn3r_gemm_f16 / syn3r_gemm_2src_f16 / syn3r_conv2d3x3_f16 /
 * syn3r_tconv3_f16 given gn_partials = buf (16-byte aligned) and gn_partials_bytes = bytes also write, for their [M, N] fp16
 * output as stored,
 *     buf[((m / 32) * 2 + q) * (N / 10) + n / 10]   (float; q = 0: sum of x, q = 1: sum of x^2)
 * over rows [32 rb, 32 rb + 32) and columns [10 u, 10 u + 10) - if M % 32 == 0, N % 80 == 0, bytes >=
 * syn3r_gn_partials_bytes(M, N) and the kernel chosen for the shape has the lean epilogue (the persistent 256-row
 * kernels).  *gn_written (host, may be NULL) is set on every return of these four entries, errors included: 1 if the launched
 * kernel writes buf, else 0 - buf is then left untouched and the consumer runs syn3r_groupnorm_f16 as before.  It is known at
 * launch time: no synchronisation.  (NULL, 0) = no request; a pointer without a size, a size without a pointer or a misaligned
 * pointer is SYN3R_E_INVALID.  Fixed summation order: bitwise reproducible run to run.
 *
 * syn3r_groupnorm_pre_f16: syn3r_groupnorm_f16 / _2src_f16 (x2 = NULL, C2 = 0: one source) with the statistics folded from
 * such partial sums (part1 for x1, part2 for x2).  rows % 32 == 0, (C1 + C2) / 32 and C1 multiples of 10.  Same workspace.
 */
size_t syn3r_gn_partials_bytes(int M, int N);
int syn3r_groupnorm_pre_f16(const void* x1, int C1, const void* part1, const void* x2, int C2, const void* part2, void* y,
                            int samples, int rows, const void* gamma, const void* beta, float eps, int silu,
                            void* workspace, size_t workspace_bytes, void* stream);

/*
 * LayerNorm over C of [M, C] fp16.  If addvec != NULL, addvec[m / rows_per_vec, :] is added first
 * (fp16 add: `hidden_states + emb`, transformer_temporal.py:355) and, if xsum != NULL, the sum is
 * also written there (it is the temporal block's residual, attention.py:490).
 */
int syn3r_layernorm_f16(const void* x, void* y, void* xsum, const void* addvec, int rows_per_vec, long long M,
                        int C, const void* gamma, const void* beta, float eps, void* stream);

/* GEGLU gate (activations.py GEGLU.forward): y[M,D] = x[:, :D] * gelu_erf(x[:, D:]) for x [M, 2D]. */
int syn3r_geglu_f16(const void* x, void* y, long long M, int D, void* stream);

/* Row softmax of an fp16 matrix in fp32 arithmetic: y[m,:] = softmax(scale * x[m,:]); x may equal y.
 * The single-head, 512-wide attention of the VAE mid blocks (attention_processor.py:1222-1299 through
 * vae.py:119-129 and unet_3d_blocks.py:1794-1805) is two syn3r_gemm_f16 calls around this kernel. */
int syn3r_softmax_rows_f16(const void* x, void* y, long long M, int N, long long ld, float scale, void* stream);

/* TemporalDecoder.time_conv_out (autoencoder_kl_temporal_decoder.py:78-84,156-160): Conv3d(3,3,(3,1,1)) over
 * frames.  x [B*F*HW, ldx] fp16 channels-last (first 3 columns used), w [3,3,3] = weight[co][ci][dt] and bias [3]: fp32 HOST
 * pointers (30 floats, passed as kernel arguments) -> out [B*F, 3, HW] fp32 (the NCHW frames the decoder returns). */
int syn3r_time_conv_out(const void* x, long long ldx, const float* w, const float* bias, float* out, int B, int F,
                        long long HW, void* stream);

/* ------------------------------------------------------------------------
 * Trainer-loop pieces adjacent to the rasteriser.  The reference runs them inside FSGS'
 * gsTrainer.training()/finetune() (call sites model/diffusionGS.py:139, 1640; submodule not vendored) as
 * torch elementwise chains; the published 3DGS step is Ll1 = |render - gt|.mean() and
 * torch.optim.Adam(eps = 1e-15).
 * ------------------------------------------------------------------------ */

/* loss[0] = weight * mean(|image - target|) over n floats (device scalar; deterministic two-level sum).
 * ws: syn3r_l1_loss_workspace_bytes(n) bytes of device scratch. */
size_t syn3r_l1_loss_workspace_bytes(long long n);
int syn3r_l1_loss(const float* image, const float* target, long long n, float weight, float* loss, void* ws,
                  size_t ws_bytes, void* stream);
/* grad_image[i] = grad_loss[0] * weight / n * sign(image[i] - target[i]); grad_loss is a DEVICE scalar
 * (NULL = 1), so autograd's upstream gradient never visits the host. */
int syn3r_l1_loss_backward(const float* image, const float* target, long long n, float weight,
                           const float* grad_loss, float* grad_image, void* stream);

/* mse[0] = mean((image - target)^2) over n floats (device scalar, same deterministic two-level sum and workspace
 * as syn3r_l1_loss): the MSE behind the PSNR column of the per-scene metric record (the reference
 * tabulates PSNR/SSIM/LPIPS in scripts/summarize_dl3dv.py:11-80 from FSGS' metrics.py, not vendored). */
int syn3r_image_mse(const float* image, const float* target, long long n, float* mse, void* ws, size_t ws_bytes,
                    void* stream);

/* The published 3DGS photometric loss in one pass:
 *   loss3[0] = weight * ((1 - lambda_dssim) * mean|I - G| + lambda_dssim * (1 - SSIM(I, G))), loss3[1] = L1, loss3[2] = SSIM
 * I, G [C,H,W] fp32; SSIM with the 11x11 Gaussian window (sigma 1.5), zero padding 5, C1 = 0.01^2, C2 = 0.03^2, mean
 * over all C*H*W.  ws (syn3r_photo_loss_workspace_bytes) also receives the three derivative maps the backward
 * reads, so the SAME workspace must be passed to syn3r_photo_loss_backward, which writes
 * grad_image = grad_loss[0] * d loss3[0] / d I  (grad_loss: device scalar, NULL = 1). */
size_t syn3r_photo_loss_workspace_bytes(int C, int H, int W);
int syn3r_photo_loss(const float* image, const float* target, int C, int H, int W, float lambda_dssim, float weight,
                     float* loss3, void* ws, size_t ws_bytes, void* stream);
int syn3r_photo_loss_backward(const float* image, const float* target, int C, int H, int W, float lambda_dssim,
                              float weight, const float* grad_loss, const void* ws, float* grad_image, void* stream);
/* Value AND gradient in two launches (a training step wants both): syn3r_photo_loss followed by syn3r_photo_loss_backward on the
 * same arguments, except that loss3 is written by the gradient pass (its first block forms the forward's sums; the gradient does
 * not depend on them) instead of by a single-block launch between the passes.  Same bits in loss3 and grad_image. */
int syn3r_photo_loss_step(const float* image, const float* target, int C, int H, int W, float lambda_dssim, float weight,
                          const float* grad_loss, float* loss3, float* grad_image, void* ws, size_t ws_bytes, void* stream);

/* EXTENSION (not in the reference, which weights a whole pseudo-view by the scalar cam_confidence, model/diffusionGS.py:1631):
 * the photometric loss with a per-pixel weight map m [H,W] fp32 shared by all channels (meant to lie in [0,1] and be finite;
 * not validated on the device; it is data - no gradient with respect to it).  With ssim(c,p) the published SSIM map exactly
 * as syn3r_photo_loss forms it - the map weights the per-pixel SSIM VALUE, it does not enter the window moments - and all
 * means over the C*H*W elements (NOT divided by sum(m): a constant map m = k is the scalar weight k * weight, a map of ones
 * is syn3r_photo_loss):
 *   loss4[1] = mean(m |I - G|), loss4[2] = mean(m ssim), loss4[3] = mean(m),
 *   loss4[0] = weight * ((1 - lambda_dssim) * loss4[1] + lambda_dssim * (loss4[3] - loss4[2]))
 *   grad_image(c,q) = grad_loss[0] * weight / (C*H*W) * [ (1 - lambda_dssim) m(q) sign(I - G)(c,q)
 *                     - lambda_dssim (win*(m d_mu1) + 2 I(c,q) win*(m d_sg1) + G(c,q) win*(m d_sg12))(c,q) ]
 * d_mu1, d_sg1, d_sg12: the derivative maps of the SSIM value the forward stores, win*: the 11x11 separable window.
 * Arguments as the three entries above plus map (H*W floats, device); loss4: 4 floats; ws:
 * syn3r_photo_loss_map_workspace_bytes (3 sums per tile instead of 2), shared by forward and backward.  A null map, a null
 * image or non-positive sizes are rejected (syn3r_last_error).  syn3r_photo_loss_map_step: same bits as
 * syn3r_photo_loss_map + syn3r_photo_loss_map_backward. */
size_t syn3r_photo_loss_map_workspace_bytes(int C, int H, int W);
int syn3r_photo_loss_map(const float* image, const float* target, const float* map, int C, int H, int W, float lambda_dssim,
                         float weight, float* loss4, void* ws, size_t ws_bytes, void* stream);
int syn3r_photo_loss_map_backward(const float* image, const float* target, const float* map, int C, int H, int W,
                                  float lambda_dssim, float weight, const float* grad_loss, const void* ws, float* grad_image,
                                  void* stream);
int syn3r_photo_loss_map_step(const float* image, const float* target, const float* map, int C, int H, int W, float lambda_dssim,
                              float weight, const float* grad_loss, float* loss4, float* grad_image, void* ws, size_t ws_bytes,
                              void* stream);
/* The L1 pair with the same map: element i of the n = C * plane floats belongs to pixel i % plane (plane = H*W, so the flat index
 * finds its pixel; n must be a multiple of plane):
 *   loss[0] = weight * mean(m |image - target|) over n;  grad_image[i] = grad_loss[0] * weight / n * m[i % plane] * sign(image[i] - target[i])
 * ws: syn3r_l1_loss_workspace_bytes(n).  Same rejections. */
int syn3r_l1_loss_map(const float* image, const float* target, const float* map, long long n, long long plane, float weight,
                      float* loss, void* ws, size_t ws_bytes, void* stream);
int syn3r_l1_loss_map_backward(const float* image, const float* target, const float* map, long long n, long long plane,
                               float weight, const float* grad_loss, float* grad_image, void* stream);

/* FSGS' depth-correlation regulariser (Zhu et al., ECCV 2024, "geometry guidance"; the reference's batch scripts switch FSGS'
 * depth terms on, bash_scripts/batch_{llff,dl3dv}_train.sh --svd_depth_warmup 1; FSGS' trainer is not vendored) on one rendered
 * depth map d and one monocular prior p, n = H*W fp32 values each:
 *   branch A: t = -p;  branch B: t = 1 / (p + offset);  r_X = S_dt / sqrt(S_dd S_tt) (centred sums, clamped to [-1, 1])
 *   loss = weight * min(1 - r_A, 1 - r_B) (SYN3R_DCORR_MIN; A on a tie) or one branch (SYN3R_DCORR_A / _B)
 * The two-transform minimum and offset = 200 are recalled from FSGS' train.py (not available): UNPINNED, hence arguments.
 * A branch with S_dd == 0 or S_tt == 0 has r = 0, loss 1 and a zero gradient (no NaN).  fp64 centred moments merged in a fixed
 * order: bitwise repeatable.  parts (device, 16-byte aligned, 4 floats): [loss, r_A, r_B (0 in mode A), branch (0 = A, 1 = B)].
 * ws: syn3r_depth_corr_loss_workspace_bytes(n) bytes (0 for n outside [2, 2^30]); it holds the statistics the backward
 * reads, so syn3r_depth_corr_loss_backward takes the SAME workspace.  Rejections: SYN3R_E_INVALID, or SYN3R_E_WORKSPACE for
 * a short workspace. */
#define SYN3R_DCORR_MIN 0
#define SYN3R_DCORR_A 1
#define SYN3R_DCORR_B 2
size_t syn3r_depth_corr_loss_workspace_bytes(long long n);
/* value only: two launches (statistics, one-block combine) */
int syn3r_depth_corr_loss(const float* depth, const float* prior, long long n, float weight, float offset, int mode, float* parts,
                          void* ws, size_t ws_bytes, void* stream);
/* grad_depth = grad_loss[0] * d loss / d depth through the chosen branch (grad_loss: device scalar, NULL = 1); one launch */
int syn3r_depth_corr_loss_backward(const float* depth, const float* prior, long long n, float weight, float offset, int mode,
                                   const float* grad_loss, const void* ws, size_t ws_bytes, float* grad_depth, void* stream);
/* Value AND gradient in two launches: the statistics pass, then the gradient pass, whose block 0 writes parts (every block of
 * it combines the statistics in the same fixed order).  Same bits as syn3r_depth_corr_loss + syn3r_depth_corr_loss_backward. */
int syn3r_depth_corr_loss_step(const float* depth, const float* prior, long long n, float weight, float offset, int mode,
                               const float* grad_loss, float* parts, float* grad_depth, void* ws, size_t ws_bytes, void* stream);

/* The same term PATCH-WISE (EXTENSION in the spirit of SparseGS' patch-based Pearson and DNGaussian's local depth normalisation:
 * a monocular prior is one monotone transform of the depth only locally).  d and p are H x W fp32 maps, P the patch size,
 * (oy, ox) the origin of the patch grid, 0 <= oy, ox < P.  Patch (i, j) covers rows oy + iP .. oy + (i+1)P - 1 and columns
 * ox + jP .. ox + (j+1)P - 1; only the K = floor((H - oy) / P) * floor((W - ox) / P) patches inside the image count, K >= 1.
 * Per patch k, over its P^2 pixels, the rules of the global term above:
 *   r_A = Pearson(d, -p), r_B = Pearson(d, 1 / (p + offset)) from centred sums, clamped to [-1, 1]; a branch with S_dd == 0 or
 *   S_tt == 0 has r = 0, loss 1 and a zero gradient (no NaN); L_k = min(1 - r_A, 1 - r_B) (SYN3R_DCORR_MIN, A on a tie) or one
 *   branch (SYN3R_DCORR_A / _B); the branch is chosen per patch.
 *   loss = weight / K * sum_k L_k
 *   grad_depth_i = weight * grad_loss[0] / K * -[ (t_i - t_mean) / sqrt(S_dd S_tt) - r (d_i - d_mean) / S_dd ]  with patch k's
 *   sums and means for i in patch k; pixels in no full patch contribute nothing and have a zero gradient.
 * Flat patches stay in K, so K depends on the geometry alone.  The two transforms and offset = 200 are recalled from FSGS'
 * train.py (not available): UNPINNED, hence arguments; the patch grid is this library's own.
 * fp64 throughout, sums shifted by the first element, fixed merge orders, no float atomics, no host read: the loss and the gradient
 * are bitwise repeatable for a given shape.  parts (device, 16-byte aligned, 4 floats): [loss, mean over patches of the chosen r,
 * share of patches on branch B, share of flat patches].
 * accumulate 0: every pixel of grad_depth is written (zeros outside the full patches; the buffer may hold anything);
 * accumulate 1: the gradient is ADDED to grad_depth inside the patches and the rest is left alone (the global and the patch-wise
 * term then share one buffer without an add launch).
 * ws: syn3r_depth_corr_local_workspace_bytes(H, W, P, oy, ox) bytes, 16-byte aligned (0 for arguments the entries reject); it
 * holds one finished 64-byte record per patch, which the backward reads: syn3r_depth_corr_local_loss_backward takes the SAME
 * workspace and the same mode and offset as the call that filled it.
 * Rejections before any HIP call (SYN3R_E_INVALID): null pointers, H or W outside [1, 2^15], P outside [2, 256], oy or ox outside
 * [0, P), K = 0, an unknown mode, a non-finite weight or offset, accumulate not 0 or 1, a misaligned parts or workspace; a short
 * workspace is SYN3R_E_WORKSPACE. */
size_t syn3r_depth_corr_local_workspace_bytes(int H, int W, int P, int oy, int ox);
/* value only: the statistics launch and a one-block sum */
int syn3r_depth_corr_local_loss(const float* depth, const float* prior, int H, int W, int P, int oy, int ox, float weight, float offset,
                                int mode, float* parts, void* ws, size_t ws_bytes, void* stream);
/* the gradient launch on the records of syn3r_depth_corr_local_loss (grad_loss: device scalar, NULL = 1) */
int syn3r_depth_corr_local_loss_backward(const float* depth, const float* prior, int H, int W, int P, int oy, int ox, float weight,
                                         float offset, int mode, const float* grad_loss, const void* ws, size_t ws_bytes,
                                         float* grad_depth, int accumulate, void* stream);
/* Value AND gradient in two launches: the statistics, then the gradient, whose first block also writes parts.  Same bits as
 * syn3r_depth_corr_local_loss + syn3r_depth_corr_local_loss_backward. */
int syn3r_depth_corr_local_loss_step(const float* depth, const float* prior, int H, int W, int P, int oy, int ox, float weight,
                                     float offset, int mode, const float* grad_loss, float* parts, float* grad_depth, int accumulate,
                                     void* ws, size_t ws_bytes, void* stream);

/* Prior-free edge-aware depth smoothness (EXTENSION: the reference has none; the form of Monodepth2, Godard et al., ICCV 2019, which
 * DNGaussian-, SparseGS- and RegNeRF-style sparse-view pipelines use as well): the rendered depth d [H,W] fp32 should be piecewise
 * smooth and may jump only where the camera's own target image has an edge.  It needs no depth prior.
 *   weights = [wx, wy], two fp32 planes [2,H,W] from the image I [3,H,W] (syn3r_depth_edge_weights):
 *     wx[y,x] = exp(-gamma * mean_c |I_c[y,x+1] - I_c[y,x]|)      wy[y,x] = exp(-gamma * mean_c |I_c[y+1,x] - I_c[y,x]|)
 *     (fp32, expf; the last column of wx and the last row of wy are written as zeros)
 *   m    = mean of d over all H*W pixels
 *   S_x  = 1/N_x * sum_{y, x<W-1} wx[y,x] * |d[y,x+1] - d[y,x]|      N_x = H (W-1)
 *   S_y  = 1/N_y * sum_{y<H-1, x} wy[y,x] * |d[y+1,x] - d[y,x]|      N_y = (H-1) W
 *   loss = weight * (S_x + S_y) / m
 *   grad_depth_i = weight * grad_loss[0] * [ (dS/dd_i) / m - (S_x + S_y) / (m^2 H W) ]      (grad_loss: device scalar, NULL = 1)
 * dS/dd_i is the signed sum over the up to four edges at pixel i, sign(0) = 0; the derivative goes through the mean.  A direction
 * without pairs (W == 1 or H == 1) contributes 0.  m <= 0 (an empty render) gives loss 0 and a zero gradient, never NaN.  The loss
 * entries treat the last column of wx and the last row of wy as absent, whatever they hold.  gamma = 1 and the division by the
 * mean are recalled from Monodepth2 (not available): UNPINNED, hence gamma is an argument.
 * The statistics pass keeps fp32 running sums per thread, adds them over the wave and the block's waves in a fixed order and leaves
 * one row per block in ws; the rows are added in fp64 in a fixed order.  The gradient is a gather (every pixel forms its own edges,
 * fp64, one fp32 rounding): no float atomics.  The grid is a function of H and W alone: bitwise repeatable for a given shape.
 * Rows go through 16-byte accesses when every pointer is 16-byte aligned and W % 4 == 0, anything else through scalar ones, with
 * the same bits.  parts (device, 16-byte aligned, 4 floats): [loss, S_x, S_y, m].
 * accumulate 0: every pixel of grad_depth is written (the buffer may hold anything); accumulate 1: the gradient is ADDED to it (the
 * depth terms then share one buffer without an add launch).
 * ws: syn3r_depth_smooth_workspace_bytes(H, W) bytes (0 for H or W outside [1, 2^15]), 16-byte aligned; it holds the rows the
 * backward reads, so syn3r_depth_smooth_loss_backward takes the SAME workspace.
 * Rejections before any HIP call (SYN3R_E_INVALID): null pointers, H or W outside [1, 2^15], a non-finite weight or gamma, gamma < 0,
 * accumulate not 0 or 1, a misaligned parts or workspace, weights (syn3r_depth_edge_weights) or grad_depth overlapping an input; a
 * short workspace is SYN3R_E_WORKSPACE. */
int syn3r_depth_edge_weights(const float* image, int H, int W, float gamma, float* weights /* [2,H,W] */, void* stream);
size_t syn3r_depth_smooth_workspace_bytes(int H, int W);
/* value only: two launches (statistics, one-block combine) */
int syn3r_depth_smooth_loss(const float* depth, const float* weights, int H, int W, float weight, float* parts, void* ws,
                            size_t ws_bytes, void* stream);
/* the gradient launch on the rows of syn3r_depth_smooth_loss */
int syn3r_depth_smooth_loss_backward(const float* depth, const float* weights, int H, int W, float weight, const float* grad_loss,
                                     const void* ws, size_t ws_bytes, float* grad_depth, int accumulate, void* stream);
/* Value AND gradient in two launches: the statistics, then the gradient, every block of which combines the rows in the same fixed
 * order and whose block 0 writes parts.  Same bits as syn3r_depth_smooth_loss + syn3r_depth_smooth_loss_backward. */
int syn3r_depth_smooth_loss_step(const float* depth, const float* weights, int H, int W, float weight, const float* grad_loss,
                                 float* parts, float* grad_depth, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* Multi-view photometric reprojection term (EXTENSION: the reference has none; Monodepth2's per-pixel minimum reprojection error,
 * Godard et al., ICCV 2019, without its SSIM part and auto-mask, as unsupervised-MVS and MVS-guided sparse-view 3DGS pipelines use
 * it).  Not to be confused with syn3r_reproj_error above, which serves the diffusion conditioning and is not differentiable.
 * depth D and alpha a [H,W] fp32 are a render of the target view, target I_t [3,H,W] fp32 its photograph, sources[s] (HOST array of
 * S DEVICE pointers) the photographs I_s [3,H,W] of S posed input views of the same H, W, 1 <= S <= 4.  views (HOST, S x 16 floats):
 * per source M_s (3 x 3, row-major), t_s, fx_s, fy_s, cx_s, cy_s with [M_s | t_s] = w2c_s c2w_t; target_k (HOST, 4 floats):
 * fx_t, fy_t, cx_t, cy_t.  The tables travel to the kernel by value, as syn3r_adam_step_multi's do: no per-step copy or stacking
 * of images.  Pixel convention of the rasteriser: pixel index x sits at fx X/Z + (W-1)/2, so cx = (W-1)/2, fx = W / (2 tan(FoVx/2)).
 * Per pixel p = (x, y):
 *   z = D / a                                                    dead when !(a >= alpha_min) or !(D > 0)
 *   r = ((x - cx_t) / fx_t, (y - cy_t) / fy_t, 1)       A = M_s r       X = z A + t_s
 *   q = (fx_s X_x / X_z + cx_s, fy_s X_y / X_z + cy_s)           source s valid: X_z >= 0.01, 0 <= q_x <= W-1, 0 <= q_y <= H-1
 *   e_s = (1/3) sum_c |I_s,c(q) - I_t,c(p)|     bilinear on the cell x0 = min(floor(q_x), W-2), y0 = min(floor(q_y), H-2)
 *   e = min over the valid s of e_s (the lowest s on a tie); a pixel with no valid source is dead
 *   loss = weight * sum_live e / max(N_live, 1)                  (N_live is a constant of the gradient)
 *   dL/dz = weight * grad_loss[0] / N_live * (1/3) sum_c sgn(I_s,c(q) - I_t,c(p)) (dI_s,c/dq_x dq_x/dz + dI_s,c/dq_y dq_y/dz)
 *   dq_x/dz = fx_s (A_x t_z - A_z t_x) / X_z^2       dq_y/dz = fy_s (A_y t_z - A_z t_y) / X_z^2       sgn(0) = 0
 *   grad_depth = dL/dz / a        grad_alpha = -dL/dz z / a      dead pixels: 0 in both; N_live = 0: loss 0, zero gradients
 * through the chosen source only, dI/dq the bilinear cell's own derivative (grad_loss: device scalar, NULL = 1).  The minimum and
 * the L1 form are recalled from Monodepth2 (not available); no SSIM, no auto-mask and alpha_min are this library's choices: UNPINNED.
 * The statistics pass does the geometry, the gathers and the minimum in fp32 and leaves in ws one row per block (sum e, N_live,
 * N on source 0, sum e on source 0: per-thread running sums, added over the wave and the block's waves in a fixed order) and 8
 * bytes per pixel: the unscaled dL/dz, and a record word = the fp32 bits of e with the two lowest mantissa bits replaced by the
 * chosen source (0xffffffff: dead).  The gradient pass is elementwise: it adds the rows in fp64 in a fixed order, scales, and
 * writes (accumulate 0: every pixel, the buffer may hold anything) or ADDS (accumulate 1) each of the two gradients; it repeats no
 * gather.  No float atomics, no host read; the grid is a function of H and W alone: bitwise repeatable for a given shape.  Rows go
 * through 16-byte accesses when every plane pointer is 16-byte aligned and W % 4 == 0, anything else through scalar ones, with the
 * same bits.  parts (device, 16-byte aligned, 4 floats): [loss, mean e over live pixels, N_live / (H W), share of live pixels on
 * source 0].
 * ws: syn3r_photo_reproj_workspace_bytes(H, W, S) bytes (0 for a rejected shape), 16-byte aligned: 16 KiB of rows, then the dL/dz
 * plane [H,W] fp32, then the record plane [H,W] uint32.  syn3r_photo_reproj_loss_backward takes the SAME workspace.
 * Rejections before any HIP call (SYN3R_E_INVALID): H or W outside [2, 2^15], S outside [1, 4], null pointers, a non-finite weight,
 * view or intrinsic, a zero target focal length, alpha_min not finite or <= 0, an accumulate flag not 0 or 1, a misaligned parts or
 * workspace, a gradient overlapping depth, alpha, the other gradient or the workspace (the step entry: the target or a source image as well; the
 * backward entry does not see the images), the workspace overlapping an input; a short
 * workspace is SYN3R_E_WORKSPACE. */
size_t syn3r_photo_reproj_workspace_bytes(int H, int W, int S);
/* value only: two launches (statistics, one-block combine) */
int syn3r_photo_reproj_loss(const float* depth, const float* alpha, const float* target, const float* const* sources,
                            const float* views, const float* target_k, int H, int W, int S, float weight, float alpha_min,
                            float* parts, void* ws, size_t ws_bytes, void* stream);
/* the gradient launch on what syn3r_photo_reproj_loss left in ws */
int syn3r_photo_reproj_loss_backward(const float* depth, const float* alpha, int H, int W, int S, float weight, float alpha_min,
                                     const float* grad_loss, const void* ws, size_t ws_bytes, float* grad_depth, int accumulate_depth,
                                     float* grad_alpha, int accumulate_alpha, void* stream);
/* Value AND both gradients in two launches: the statistics, then the gradient, whose block 0 also writes parts.  Same bits as
 * syn3r_photo_reproj_loss + syn3r_photo_reproj_loss_backward. */
int syn3r_photo_reproj_loss_step(const float* depth, const float* alpha, const float* target, const float* const* sources,
                                 const float* views, const float* target_k, int H, int W, int S, float weight, float alpha_min,
                                 const float* grad_loss, float* parts, float* grad_depth, int accumulate_depth, float* grad_alpha,
                                 int accumulate_alpha, void* ws, size_t ws_bytes, void* stream);

/* Per-camera affine exposure compensation (EXTENSION: the reference has none; the published 3DGS code base has since grown a
 * per-image exposure model, gsplat an appearance optimisation).  A is 3 x 4 fp32, row-major, 12 floats in DEVICE memory; image,
 * out, grad_out and grad_image are [3,H,W] fp32 planes:
 *   out_c(p)        = A[c][0] image_0(p) + A[c][1] image_1(p) + A[c][2] image_2(p) + A[c][3]     (added left to right, no clamp)
 *   grad_image_k(p) = sum_c A[c][k] grad_out_c(p)
 *   grad_A[c][k]    = sum_p grad_out_c(p) image_k(p)        grad_A[c][3] = sum_p grad_out_c(p)
 * The convention is this library's own: a 3 x 3 block times the colour as a COLUMN, then the offset.  The published code multiplies
 * a row vector by the transposed 3 x 3 block - recalled, not available to check against: UNPINNED.
 * syn3r_exposure_apply is one launch.  syn3r_exposure_backward is two: a pass over the six input planes that writes grad_image and
 * leaves one row of 12 fp32 partial sums per block in ws (per-thread running sums, added over the wave, then over the block's waves
 * in a fixed order), and a one-block kernel that adds the rows in a fixed order in fp64 and stores grad_A (accumulate == 0) or adds
 * to it (accumulate != 0).  No atomics, the grid depends on H * W alone: bitwise repeatable for a given shape.  Planes whose
 * pointers are 16-byte aligned with H * W % 4 == 0 go through 16-byte accesses, anything else (4-byte aligned) through scalar ones.
 * ws: syn3r_exposure_backward_workspace_bytes(H, W) bytes (0 for H or W outside [1, 2^15]), 16-byte aligned.
 * Rejections before any HIP call: null pointers, H or W outside [1, 2^15], misaligned pointers, out / grad_image overlapping an
 * input (SYN3R_E_INVALID), a short workspace (SYN3R_E_WORKSPACE).  The parameter update is syn3r_adam_step on the 12 floats. */
int syn3r_exposure_apply(const float* image, const float* A, int H, int W, float* out, void* stream);
size_t syn3r_exposure_backward_workspace_bytes(int H, int W);
int syn3r_exposure_backward(const float* image, const float* A, const float* grad_out, int H, int W, float* grad_image, float* grad_A,
                            int accumulate, void* ws, size_t ws_bytes, void* stream);

/* 3DGS-MCMC density control (EXTENSION: the reference has none; Kheradmand et al., NeurIPS 2024, "3D Gaussian Splatting as Markov
 * Chain Monte Carlo").  Every constant below is RECALLED from the paper and its released code, neither available to check against:
 * UNPINNED.  Parameters are the RAW ones of the trainer: xyz [n,3], log-scales [n,3], (w, x, y, z) quaternions [n,4] (normalised
 * here, / max(|q|, 1e-12)), opacity logits [n], fp32, contiguous, DEVICE memory.  n in [1, 2^24] is checked first in every entry.
 *
 * Random numbers are Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) with counter
 * (index, 0, tag, step) and key (seed & 0xffffffff, seed >> 32); tag 0 = noise, 1 = sampling.  There is no generator state: the
 * draw of an index depends on (seed, step, tag, index) alone, not on n, the grid or earlier calls.
 *
 * syn3r_mcmc_noise (one launch, in place): xyz_i += scale * gate(o_i) * Sigma_i eps_i with Sigma_i = R diag(exp(ls)^2) R^T,
 *   o_i = sigmoid(logit_i), gate(o) = 1 / (1 + exp(-100 (0.005 - o))), and eps_i three of the four Box-Muller normals of the four
 *   words x0..x3 of index i: u(x) = ((x >> 8) + 1) 2^-24 in (0, 1], v(x) = (x >> 8) 2^-24, (eps0, eps1) = sqrt(-2 ln u(x0)) (cospi,
 *   sinpi)(2 v(x1)), eps2 = sqrt(-2 ln u(x2)) cospi(2 v(x3)).  eps is fp32 arithmetic; everything after it is fp64, rounded to fp32
 *   once (off-diagonal entries of Sigma cancel).  xyz must not overlap an input; rotations 16-byte aligned.
 * syn3r_mcmc_reg_step (two launches, no atomics): loss_out[0] = opacity_reg * mean_i sigmoid(logit_i), loss_out[1] = scale_reg *
 *   mean over 3n of exp(ls); grad_opacity[i] += opacity_reg / n * o (1 - o), grad_log_scales[j] += scale_reg / (3n) * exp(ls_j): the
 *   gradients with respect to the raw parameters, ADDED in place.  The sums: fp32 per thread, over the wave, over the block's four
 *   waves in a fixed order, one row per block in ws, then one block in fp64.  The grid depends on n alone: bitwise repeatable.
 *   ws: syn3r_mcmc_reg_step_workspace_bytes(n) bytes (0 for n outside [1, 2^24]), 16-byte aligned.
 * syn3r_mcmc_weights (one launch): weights[i] = 0 where logit_i <= dead_logit (dead: decided on the logit, exactly), else
 *   (unsigned) rintf(sigmoid(logit_i) * 65536), at most 65536 and at least 328 for dead_logit = logit(0.005).
 * syn3r_mcmc_sample (three launches, integers only): the exclusive prefix sums of weights (32 bits inside chunks of 4096 elements,
 *   64-bit chunk bases: the total reaches 2^40) and, for every destination d in [0, n + m_extra): src[d] = -1 if d < n and
 *   weights[d] != 0, or if the total is 0; else r = mulhi64((x0 << 32) | x1, total) with the words of index d and src[d] = the one
 *   i with excl[i] <= r < excl[i] + weights[i].  counts[i] = the number of destinations that drew i (integer atomics: independent
 *   of order).  Every element of src [n + m_extra] and counts [n] is written.  weights must not exceed 65536 (larger values give
 *   draws from a wrong distribution, never an index outside [0, n)).  m_extra in [0, 2^24].
 *   ws: syn3r_mcmc_sample_workspace_bytes(n) bytes, 16-byte aligned.
 * syn3r_mcmc_relocate (two launches, in place): a source i with counts[i] > 0 and ratio = min(counts[i] + 1, 51) takes
 *   o' = clamp(1 - (1 - o)^(1 / ratio), min_opacity, 1 - 2^-23) and scale' = scale * o / sum_{j=1..ratio} sum_{k=0..j-1} C(j-1, k)
 *   (-1)^k o'^(k+1) / sqrt(k+1) (evaluated as sum_m C(ratio, m) (-1)^(m-1) o'^m / sqrt(m) in fp64); every destination d < n with
 *   src[d] >= 0 becomes a copy of its source - position, rotation, the feature row of feature_row_len floats - with the source's new
 *   logit and log-scales.  The first launch writes the destinations from the sources' OLD values, the second rewrites the sources;
 *   a source must not itself be a destination (true of syn3r_mcmc_sample's output: a source has a non-zero weight, a destination a
 *   zero one).  moments: a HOST array of 10 device pointers, exp_avg then exp_avg_sq of xyz, features, opacity, log-scales,
 *   rotations; any may be NULL.  The moments of every touched row (source or destination) are set to zero.
 * Rejections before any HIP call: n outside [1, 2^24], null pointers, misaligned pointers, outputs overlapping inputs, NaN scalars,
 * min_opacity outside (0, 1) (SYN3R_E_INVALID), a short workspace (SYN3R_E_WORKSPACE). */
int syn3r_mcmc_noise(float* xyz, const float* log_scales, const float* rotations, const float* opacity_logits, int n, float scale,
                     unsigned long long seed, int step, void* stream);
size_t syn3r_mcmc_reg_step_workspace_bytes(int n);
int syn3r_mcmc_reg_step(const float* opacity_logits, const float* log_scales, int n, float opacity_reg, float scale_reg,
                        float* grad_opacity, float* grad_log_scales, float* loss_out, void* ws, size_t ws_bytes, void* stream);
int syn3r_mcmc_weights(const float* opacity_logits, int n, float dead_logit, unsigned* weights, void* stream);
size_t syn3r_mcmc_sample_workspace_bytes(int n);
int syn3r_mcmc_sample(const unsigned* weights, int n, int m_extra, unsigned long long seed, int step, int* src, unsigned* counts,
                      void* ws, size_t ws_bytes, void* stream);
int syn3r_mcmc_relocate(int n, const int* src, const unsigned* counts, float* xyz, float* features, int feature_row_len,
                        float* opacity_logits, float* log_scales, float* rotations, void* const* moments, float min_opacity,
                        void* stream);

/* One torch.optim.Adam update (no weight decay, no amsgrad) of n fp32 parameters in place, in torch's
 * operation order: exp_avg.lerp_(g, 1-beta1); exp_avg_sq = beta2*exp_avg_sq + (1-beta2)*g*g;
 * param -= lr/(1-beta1^step) * exp_avg / (sqrt(exp_avg_sq)/sqrt(1-beta2^step) + eps).  step is 1-based. */
int syn3r_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, float lr,
                    float beta1, float beta2, float eps, int step, void* stream);
/* The same update of up to 8 tensors in ONE launch (the trainer's parameter groups: torch's _multi_tensor_adam; element for
 * element the arithmetic of syn3r_adam_step).  Host arrays of `count` entries: device pointers, element counts, learning rates,
 * eps and 1-based steps per tensor; beta1 / beta2 are shared. */
int syn3r_adam_step_multi(int count, float* const* params, const float* const* grads, float* const* exp_avgs,
                          float* const* exp_avg_sqs, const long long* numels, const float* lrs, float beta1, float beta2,
                          const float* epss, const int* steps, void* stream);
/* syn3r_adam_step_multi with TWO learning rates inside a row of a tensor: the published 3DGS optimiser behind
 * gsTrainer.training() / finetune() (model/diffusionGS.py:139,1640) holds the SH coefficients as two torch.optim.Adam groups,
 * f_dc at feature_lr and f_rest at feature_lr / 20; here they are ONE contiguous [N, M, 3] tensor (the rasteriser takes one `shs`
 * pointer), so the kernel picks the rate by position: element i of tensor k uses lrs[k] when i % row_lens[k] < head_lens[k], else
 * lrs_tail[k] (the features: row_len = 3 M, head_len = 3).  row_lens[k] == 0: no split, lrs[k] everywhere, lrs_tail[k] unread
 * (lrs_tail may be NULL when no tensor is split).  Everything else as syn3r_adam_step_multi, bit for bit.  Refused besides that
 * entry's cases: row_len < 0, head_len outside 0..row_len, numel % row_len != 0, a split tensor of 2^31 elements or more. */
int syn3r_adam_step_multi_rows(int count, float* const* params, const float* const* grads, float* const* exp_avgs,
                               float* const* exp_avg_sqs, const long long* numels, const float* lrs, const float* lrs_tail,
                               const int* row_lens, const int* head_lens, float beta1, float beta2,
                               const float* epss, const int* steps, void* stream);

/* The parameter activations of the published 3DGS model that FSGS' trainer applies before every render inside
 * gsTrainer.training() / finetune() (model/diffusionGS.py:139,1640; GaussianModel.get_scaling / get_rotation / get_opacity):
 * scales = exp(log_scales) [N,3], rotations_n = rotations / max(|rotations|_2, 1e-12) [N,4], opacities = sigmoid(logits) [N],
 * in one launch; and their chain rule (torch's formulas) in one launch: d_log_scales = d_scales * scales,
 * d_rotations = (g - qhat (qhat . g)) / max(|q|, 1e-12), d_opacity_logits = d_opacities * s (1 - s).  fp32, caller-owned. */
int syn3r_gaussian_activate(int N, const float* log_scales, const float* rotations, const float* opacity_logits, float* scales,
                            float* rotations_n, float* opacities, void* stream);
int syn3r_gaussian_activate_backward(int N, const float* rotations, const float* scales, const float* rotations_n,
                                     const float* opacities, const float* d_scales, const float* d_rotations_n,
                                     const float* d_opacities, float* d_log_scales, float* d_rotations, float* d_opacity_logits,
                                     void* stream);

/* The per-iteration statistics of the published adaptive density control (3DGS section 5.2; GaussianModel.add_densification_stats
 * as FSGS' loop behind gsTrainer.training() applies it), for the Gaussians the render saw (radii[i] > 0), in one launch and without
 * the host synchronisations of boolean-mask indexing: grad_accum[i] += |viewspace_grad[i, :2]|_2 (sqrt(gx*gx + gy*gy), fp32),
 * denom[i] += 1, max_radii[i] = max(max_radii[i], radii[i]).  viewspace_grad [N,3] fp32; radii [N] i32; the rest [N] fp32. */
int syn3r_densification_stats(int N, const int* radii, const float* viewspace_grad, float* grad_accum, float* denom,
                              float* max_radii, void* stream);
/* The same (the published 3DGS add_densification_stats) and, for the same Gaussians and in the same launch, the statistic AbsGS
 * (section 3.2; UNPINNED, see syn3r_raster_backward_abs) takes the split decision on:
 * grad_accum_abs[i] += |abs_grad[i]|_2 (sqrt(ax*ax + ay*ay), fp32).  abs_grad [N,2] fp32 = syn3r_raster_backward_abs' dL_dmeans2D_abs;
 * grad_accum_abs [N] fp32. */
int syn3r_densification_stats_abs(int N, const int* radii, const float* viewspace_grad, const float* abs_grad, float* grad_accum,
                                  float* grad_accum_abs, float* denom, float* max_radii, void* stream);

/* out[i] = mean of the three smallest squared Euclidean distances from point i to the OTHER points of the cloud
 * (points [n,3] fp32, n >= 4): the quantity FSGS' GaussianModel.create_from_pcd takes from `distCUDA2` of the
 * simple-knn CUDA extension to initialise the Gaussian scales (reached from reset_gaussians_from_pcd,
 * model/diffusionGS.py:1685-1687; the extension is an un-vendored submodule).  Exact search (Morton
 * order + bounding-box pruning), d2 = (dx*dx + dy*dy) + dz*dz without fused multiply-add, sum (b0 + b1) + b2 ascending.
 * ws: syn3r_knn3_workspace_bytes(n) bytes of 256-byte aligned device scratch. */
size_t syn3r_knn3_workspace_bytes(int n);
int syn3r_knn3_mean_dist2(const float* points, int n, float* out, void* ws, size_t ws_bytes, void* stream);

/* The directed 3-nearest-neighbour graph of a cloud (points [n,3] fp32, 4 <= n <= 2^24): for point i the three OTHER points with
 * the smallest d2 = (dx*dx + dy*dy) + dz*dz (no fused multiply-add), ascending by the pair (d2, original index) - the index breaks
 * ties, so the answer is unique.  dist2 [n,3] fp32, index [n,3] int32.  ((dist2[i,0] + dist2[i,1]) + dist2[i,2]) / 3 is
 * syn3r_knn3_mean_dist2's out[i] bit for bit (same search, same boxes; that entry keeps only the distances).  Replaces the
 * neighbour query behind FSGS' proximity-guided densification (Zhu et al., ECCV 2024, section 3.2: "a directed graph connecting
 * each Gaussian to its K = 3 nearest neighbours"; switched by --use_proximity_densify in bash_scripts/batch_{llff,dl3dv}_train.sh;
 * FSGS' trainer is not vendored).  ws: syn3r_knn3_graph_workspace_bytes(n) bytes, 256-byte aligned (0 for n outside the range). */
size_t syn3r_knn3_graph_workspace_bytes(int n);
int syn3r_knn3_graph(const float* points, int n, float* dist2, int* index, void* ws, size_t ws_bytes, void* stream);

/* FSGS' proximity-guided Gaussian unpooling on that graph (same section of the paper; what FSGS' densification does between the
 * split and the prune when --use_proximity_densify is set; source not available, so every constant is an argument: UNPINNED).
 *   count: Gaussian i is a source iff ((dist2[i,0] + dist2[i,1]) + dist2[i,2]) / 3 > score_thresh AND
 *          max_c log_scales[i,c] > log_scale_thresh (raw log-scales against a host-computed log(threshold); -inf switches the second
 *          test off).  Leaves the number of sources S in *count (device, one int32) and flags + ordered offsets in ws.
 *   emit:  for the S sources in ascending index order and for each its neighbours nearest first, row 3 * rank + t of the outputs:
 *          xyz = (xyz_src + xyz_dst) * 0.5f, log-scales / opacity logit / confidence of the DESTINATION, rotation (1, 0, 0, 0); one row
 *          per directed edge, 3 S rows, no de-duplication.  SH coefficients of the new Gaussians are zero: the caller's buffers.
 *          The order is fixed by an ordered scan (no atomics): two runs are bitwise equal.
 * The host reads *count ONCE between the two calls (the only synchronisation) and passes it as n_sources; capacity = rows the output
 * buffers hold: capacity < 3 * n_sources is SYN3R_E_INVALID with nothing written (the kernel also drops rows >= capacity).
 * ws: syn3r_gaussian_unpool_workspace_bytes(n) bytes, 256-byte aligned, the SAME buffer for both calls.  Rejected on the host
 * before any HIP call: null pointers, n outside [4, 2^24], a misaligned workspace, NaN thresholds (SYN3R_E_INVALID), a short
 * workspace (SYN3R_E_WORKSPACE; syn3r_knn3_graph likewise). */
size_t syn3r_gaussian_unpool_workspace_bytes(int n);
int syn3r_gaussian_unpool_count(const float* dist2, const float* log_scales, int n, float score_thresh, float log_scale_thresh,
                                int* count, void* ws, size_t ws_bytes, void* stream);
int syn3r_gaussian_unpool_emit(const float* xyz, const float* log_scales, const float* opacity_logits, const float* confidence,
                               const int* index, int n, int n_sources, int capacity, float* out_xyz, float* out_log_scales,
                               float* out_opacity_logits, float* out_rotations, float* out_confidence, const void* ws,
                               size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * LPIPS (VGG16) perceptual loss term of the trainer (the reference raises `opt.use_lpips_loss` around every refine,
 * model/diffusionGS.py:1690,1697; the loss lives in un-vendored FSGS and calls the `lpips` package: the PUBLISHED
 * definition is restated, csrc/lpips.hip).  Activations are channels-last fp16 [H*W, C].
 * ------------------------------------------------------------------------ */
/* 3x3 convolution, stride 1, padding 1, + bias, with the activation options VGG needs: relu != 0: out = max(out, 0);
 * relu_mask (nullable) [NB*Hi*Wi, Cout]: out zeroed where mask <= 0 (the ReLU backward of the layer below, fused into the
 * backward-data convolution, which is this same kernel on the transposed, flipped weights).  Cin % 64 == 0, Cout % 8 == 0. */
int syn3r_conv2d3x3_act_f16(const void* X, const void* W, void* out, const void* bias, int relu, const void* relu_mask,
                            int NB, int Hi, int Wi, int Cin, int Cout, void* stream);
/* image [3,H,W] fp32 in [0,1] -> LPIPS input scaling ((2x-1) - shift) / scale -> [H*W, 64] fp16 (channels 3..63 zero) */
int syn3r_lpips_image_f16(const float* img, int H, int W, void* out, void* stream);
/* gradient wrt that [H*W, 64] tensor (carrying loss_scale) -> d loss / d image [3,H,W] fp32 */
int syn3r_lpips_image_bwd(const void* grad64, int H, int W, float loss_scale, float* d_img, void* stream);
/* nn.MaxPool2d(2, 2) on [H,W,C] fp16 -> [H/2,W/2,C], and its backward (gradient to the first maximum of each window) */
int syn3r_maxpool2_f16(const void* x, int H, int W, int C, void* y, void* stream);
int syn3r_maxpool2_bwd_f16(const void* x, const void* gy, int H, int W, int C, void* gx, void* stream);
/* One LPIPS layer: value[0] (=, or += with accumulate) mean_p sum_c w_c (a_c/(|a|+1e-10) - b_c/(|b|+1e-10))^2 for feature
 * maps a, b [P, C] fp16, C in {64,128,256,512}, w [C] fp32 device; and its gradient wrt a times gscale into grad_a [P, C]. */
size_t syn3r_lpips_layer_workspace_bytes(long long P, int C);
int syn3r_lpips_layer_f16(const void* a, const void* b, const float* w, long long P, int C, int accumulate, float* value,
                          void* ws, size_t ws_bytes, void* stream);
int syn3r_lpips_layer_bwd_f16(const void* a, const void* b, const float* w, long long P, int C, float gscale, int accumulate,
                              void* grad_a, void* stream);
/* Split activations (the "fp16x2" precision of gs/lpips.py): a forward activation v - the fp32 accumulator after bias and ReLU -
 * is stored as the fp16 pair hi = half(v), lo = half(v - float(hi)), channels-last [H*W, 2C] with the hi plane in channels
 * [0, C) and the lo plane in [C, 2C).  Gradients stay single fp16 tensors [H*W, C] carrying the loss scale.
 * The 3x3 convolution for such tensors.  Its INPUT X [NB*Hi*Wi, Cin] is read as the plain kernel reads it: a split tensor of C
 * channels is passed as Cin = 2C under weights duplicated along Cin ([W | W]: fp32 accumulation sums W.hi + W.lo before the one
 * rounding); the image tensor keeps Cin = 64.  split_out != 0: out [NB*Hi*Wi, ld_out >= 2 Cout] receives the pair of
 * max(acc + bias, 0) (relu != 0) or of acc + bias; relu_mask must be null.  split_out == 0: out [.., ld_out >= Cout] is one
 * fp16 result, zeroed where relu_mask [.., ld_mask] <= 0 (nullable; backward-data on the transposed, flipped weights: the mask is
 * the hi plane of the split activation below, ld_mask = twice its channel count).  Cin % 64 == 0, Cout % 8 == 0, strides % 8 == 0. */
int syn3r_conv2d3x3_split_f16(const void* X, const void* W, void* out, long long ld_out, const void* bias, int relu, int split_out,
                              const void* relu_mask, long long ld_mask, int NB, int Hi, int Wi, int Cin, int Cout, void* stream);
/* image [3,H,W] fp32 in [0,1] -> [H*W, 64] fp16 with the three scaled channels as pairs: hi in channels 0..2, lo in 3..5, rest zero */
int syn3r_lpips_image_split_f16(const float* img, int H, int W, void* out, void* stream);
/* nn.MaxPool2d(2, 2) on a split map x [H,W,2C] -> y [H/2,W/2,2C]: cells compared as float(hi) + float(lo), the winning pair copied
 * (first maximum of the window); its backward takes the same x, gy [H/2,W/2,C] fp16 and writes gx [H,W,C] fp16.  C % 8 == 0. */
int syn3r_maxpool2_split_f16(const void* x, int H, int W, int C, void* y, void* stream);
int syn3r_maxpool2_bwd_split_f16(const void* x, const void* gy, int H, int W, int C, void* gx, void* stream);
/* The LPIPS layer and its backward on split feature maps a, b [P, 2C] (read as float(hi) + float(lo)); grad_a [P, C] fp16, saturated
 * to the fp16 range like the fp16 entry's.  Same workspace. */
int syn3r_lpips_layer_split_f16(const void* a, const void* b, const float* w, long long P, int C, int accumulate, float* value,
                                void* ws, size_t ws_bytes, void* stream);
int syn3r_lpips_layer_bwd_split_f16(const void* a, const void* b, const float* w, long long P, int C, float gscale, int accumulate,
                                    void* grad_a, void* stream);

/* Statistical outlier removal of a point cloud: what model/diffusionGS.py:321 asks of open3d
 * (`down_pcd.remove_statistical_outlier(nb_neighbors=20, std_ratio=3.0)`; open3d 0.17.0 is not in the reference tree, the
 * published algorithm is restated in csrc/knn.hip).  points [n,3] float64 (open3d holds doubles).  Outputs, all device
 * memory: avg_dist [n] float64 = mean distance to the nb_neighbors nearest points (the point itself included, as the k-d
 * tree query returns it); keep [n] bytes = 0 < avg < mean + std_ratio * std; stats [4] = {mean, std (n-1), threshold,
 * valid count}.  nb_neighbors must be 20 (the reference's call).  ws: syn3r_pcd_outlier_workspace_bytes(n), 256-byte aligned. */
size_t syn3r_pcd_outlier_workspace_bytes(int n);
int syn3r_pcd_statistical_outlier(const double* points, int n, int nb_neighbors, double std_ratio, double* avg_dist,
                                  unsigned char* keep, double* stats, void* ws, size_t ws_bytes, void* stream);

/* Forward / backward optical-flow cycle-consistency mask: the test behind
 * `gsTrainer.generate_corresp_mask(gs_renderings, svd_outputs, dist_thresh=3, desc_only=False)` (model/diffusionGS.py:377;
 * the FSGS wrapper and GMFlow are absent, see csrc/warp.hip).  flow_fw / flow_bw [n,2,H,W] fp32 (A->B and B->A, channel 0 =
 * dx); mask [n,H,W] fp32 in {0,1}: |fw(x) + bw(x + fw(x))| < thresh and x + fw(x) inside the image; dist (nullable)
 * [n,H,W] = that cycle error (+inf outside). */
int syn3r_flow_cycle_mask(const float* flow_fw, const float* flow_bw, int n, int H, int W, float thresh, float* mask, float* dist,
                          void* stream);

/*
 * The whole UNet forward as ONE call: `self.unet(latent_model_input, t, encoder_hidden_states=image_embeddings,
 * added_time_ids=added_time_ids, return_dict=False)[0]` (model/SVD_2pass_prob_uncertain_post.py:763,786;
 * UNetSpatioTemporalConditionModel.forward, diffusers/models/unets/unet_spatio_temporal_condition.py:356-489) for hosts that
 * are not Python.  The launch sequence is the one syn3r_amd/unet/model.py issues (same operators, same order, same results).
 *
 * syn3r_unet_create: reads `<weights_dir>/config.json` and `<weights_dir>/diffusion_pytorch_model[.<variant>].safetensors`
 *   (the `unet/` directory of a diffusers checkpoint: what `from_pretrained(<local dir>, torch_dtype=float16, variant="fp16")`
 *   reads at model/diffusionGS.py:1089; variant may be NULL; F16 / F32 / BF16 tensors, kept in fp16), repacks the weights for the
 *   kernels and uploads them to the CURRENT device.  One handle per device; a handle is not re-entrant (one forward at a time).
 * syn3r_unet_workspace_bytes: exact scratch need of one forward of that shape (0 on a bad shape).
 * syn3r_unet_forward, all pointers device memory on the handle's device:
 *   sample [B, F, in_channels, h, w] fp16; timestep (the scheduler's continuous timestep); encoder_hidden_states
 *   [ehs_rows, cross_attention_dim] fp16 with ehs_rows = B, or 1 for one context shared by the batch; added_time_ids
 *   [B, 3] fp32 (fps, motion bucket, noise augmentation); out [B, F, out_channels, h, w] fp16.  ctx_group: 0 = the batch is
 *   one call of the reference; G > 0 = B / G independent calls of batch G stacked (the two passes of a denoising step: the
 *   reference's batch-interleaved temporal context is applied per group).  h, w multiples of 8, F <= 32.
 *   workspace: syn3r_unet_workspace_bytes(...) bytes, 256-byte aligned.  Every launch goes to `stream`; nothing synchronises
 *   except the first forward of a new (F, B), which allocates the per-block frame-position embeddings (hipMalloc).
 */
typedef struct syn3r_unet syn3r_unet;
int syn3r_unet_create(const char* weights_dir, const char* variant, syn3r_unet** out);
int syn3r_unet_destroy(syn3r_unet* unet);
size_t syn3r_unet_workspace_bytes(syn3r_unet* unet, int B, int F, int h, int w, int ehs_rows);
int syn3r_unet_forward(syn3r_unet* unet, const void* sample, double timestep, const void* encoder_hidden_states, int ehs_rows,
                       const float* added_time_ids, void* out, int B, int F, int h, int w, int ctx_group, void* workspace,
                       size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SYN3R_HIP_H */
