"""`DiffusionGS` — the reference orchestrator's call surface (`model/diffusionGS.py:39,1668`) on the HIP hot path.

`DiffusionGS(GSTrainer, num_input_views, save_dir, diffusion_type, interp_type, debug, input_args).run(refine_cycles)`
keeps the reference's constructor, method names, artefact names (`dense_views…cyc{c}_view{i}.pt` with keys `views`,
`poses`; a third key `confidence_maps` only with the `args.pixel_confidence` extension) and control flow:

    init_GS -> for each cycle: densify_views (per view pair: _interpolate_between_gs_v3 -> svd_render) -> refine_GS

What runs where: the rasteriser behind `gsTrainer.render_view` / `training`, the inverse warps, the UNet and the
scheduler steps are HIP kernels; poses, masks and the lambda schedule are host numerics (`syn3r_amd.orchestrator`).
Everything stays on the device between stages (the reference round-trips through numpy and PNG files,
diffusionGS.py:151-169,1447-1475).  Point-cloud densification (`num_views_for_pcd_densification > 1`): the
two networks it needs (GMFlow behind `gsTrainer.generate_corresp_mask`, dust3r as `gsTrainer.dust3r`) are trainer
attributes supplied by the caller, exactly where the reference keeps them; everything around them — key-frame selection,
the keep rule, the pair graph, the cloud filter — is built here.
CLIP and the temporal VAE are passed in as modules (`svd_components`), see `pipeline/svd_2pass.py`.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import List, Optional

import numpy as np
import torch

from . import orchestrator as O
from .gs.camera import Camera
from .pipeline.svd_2pass import StableVideoDiffusionPipeline
from .schedulers.scheduling_euler_discrete import SVD_XT_SCHEDULER_CONFIG, EulerDiscreteScheduler


def _resize_linear(x: np.ndarray, height: int, width: int) -> np.ndarray:
    """cv2.resize(..., INTER_LINEAR) (diffusionGS.py:804-805): pixel-centre-aligned bilinear, no antialiasing."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    chw = t[None, None] if t.dim() == 2 else t.permute(2, 0, 1)[None]
    out = torch.nn.functional.interpolate(chw, size=(height, width), mode="bilinear", align_corners=False)
    return (out[0, 0] if t.dim() == 2 else out[0].permute(1, 2, 0)).numpy()


def _resize_nearest(x: np.ndarray, height: int, width: int) -> np.ndarray:
    """cv2.resize(..., INTER_NEAREST) (diffusionGS.py:1387-1406): source index floor(dst * scale)."""
    ys = np.minimum((np.arange(height) * (x.shape[0] / height)).astype(np.int64), x.shape[0] - 1)
    xs = np.minimum((np.arange(width) * (x.shape[1] / width)).astype(np.int64), x.shape[1] - 1)
    return x[ys][:, xs]


def _resize_linear_t(x: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """`_resize_linear` on a device tensor ([H,W] or [C,H,W]), result on the device."""
    chw = x[None, None] if x.dim() == 2 else x[None]
    out = torch.nn.functional.interpolate(chw.float(), size=(height, width), mode="bilinear", align_corners=False)
    return out[0, 0] if x.dim() == 2 else out[0]


def _resize_nearest_t(x: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """`_resize_nearest` on a device tensor [H,W] (same source-index rule)."""
    ys = torch.from_numpy(np.minimum((np.arange(height) * (x.shape[0] / height)).astype(np.int64), x.shape[0] - 1)).to(x.device)
    xs = torch.from_numpy(np.minimum((np.arange(width) * (x.shape[1] / width)).astype(np.int64), x.shape[1] - 1)).to(x.device)
    return x.index_select(0, ys).index_select(1, xs)


def _pixel_confidence(runner) -> bool:
    """`args.pixel_confidence` (EXTENSION, default 0): keep the interpolation's fused uncertainty as per-pixel confidence maps."""
    return bool(getattr(getattr(runner, "args", None), "pixel_confidence", 0))


class DiffusionGS:
    def __init__(self, GSTrainer, num_input_views=12, save_dir=None, diffusion_type="2Pass", interp_type="forward_warp",
                 debug=False, input_args=None, svd_components: Optional[dict] = None, num_inference_steps: int = 100,
                 diffusion_size=(576, 1024)):
        self.args = input_args
        self.cam_confidence = self.args.cam_confidence
        self.pseudo_cam_sampling_rate = self.args.pseudo_cam_sampling_rate
        self.fps_keyframe_sampling = getattr(self.args, "fps_keyframe_sampling", 0)
        # EXTENSION (off by default, not in the reference): per-pixel confidence maps of the pseudo-views, see densify_views
        self._pair_confidence_maps = None            # of the pair _interpolate_between_gs_v3 handled last (one entry per frame)
        self.dense_confidence_maps = None            # parallel to densify_views' dense_views
        self.debug = debug
        self.gsTrainer = GSTrainer
        self.dust3r = getattr(GSTrainer, "dust3r", None)
        self.num_input_views = num_input_views
        self.save_dir = save_dir
        self.interp_type = interp_type
        assert self.interp_type in ["forward_warp", "backward_warp"]
        self.densify_type = self.args.densify_type
        self.refine_epoch = 0
        self.latent_num = 1
        cam0 = self.get_TrainCameras()[0]
        self.gs_height, self.gs_width = int(cam0.image_height), int(cam0.image_width)
        K, _ = cam0.get_calib_matrix_nerf()
        self.gs_intrinsics = K.numpy()
        self.diffusion_height, self.diffusion_width = diffusion_size
        sx, sy = self.diffusion_width / self.gs_width, self.diffusion_height / self.gs_height
        self.diffusion_intrinsics = self.gs_intrinsics.copy()        # diffusionGS.py:72-87
        self.diffusion_intrinsics[0] *= sx
        self.diffusion_intrinsics[1] *= sy
        # only these two are accepted by the reference (diffusionGS.py:115-124)
        if diffusion_type == "2PassProbUncertain":
            self.variant = "replace"
        elif diffusion_type == "2PassProbUncertainPost":
            self.variant = "post"
        else:
            raise NotImplementedError(f"diffusion_type {diffusion_type} not supported")
        self.diffusion_type = diffusion_type
        self.svd_components = svd_components
        self.num_inference_steps = num_inference_steps
        self.device = cam0.world_view_transform.device

    # ------------------------------------------------------------------ GS side
    def get_TrainCameras(self, ordered=False):
        return self.gsTrainer.scene.getTrainCameras()

    def init_GS(self, cycle=0):
        """diffusionGS.py:137-141 — HOT LOOP A."""
        self.gsTrainer.training(0, epoch_indicator=cycle)

    def render_GS(self, idx=None, pose=None, return_alpha=False):
        """diffusionGS.py:143-172 -> (w2c pose, image, depth[, alpha]).  As the reference: a TRAINING view returns
        its ground-truth image HWC in [0,255]; a free pose returns the render CHW in [0,1]."""
        assert (idx is None and pose is not None) or (idx is not None and pose is None)
        if idx is not None:
            cam = self.get_TrainCameras()[idx]
            pose = cam.world_view_transform.transpose(0, 1).cpu().numpy()
            image = cam.get_image().permute([1, 2, 0]).cpu().numpy() * 255
            res = self.gsTrainer.render_view(cam)
        else:
            tpl = self.get_TrainCameras()[0]
            cam = Camera(colmap_id=-1, R=pose[:3, :3].T, T=pose[:3, 3], FoVx=tpl.FoVx, FoVy=tpl.FoVy,
                         image=tpl.original_image, gt_alpha_mask=None, image_name=None, uid=None,
                         data_device=self.device, cam_confidence=1.0)
            res = self.gsTrainer.render_view(cam)
            image = res["render"].detach().squeeze().cpu().numpy()
        depth = res["depth"].detach().squeeze().cpu().numpy()
        if return_alpha:
            return pose, image, depth, res["alpha"].detach().squeeze().cpu().numpy()
        return pose, image, depth

    def _render_device(self, pose):
        """`render_GS(pose=...)` without the host round trip: (render [3,H,W] in [0,1], depth [H,W]) as device tensors.
        The reference copies every render to numpy (diffusionGS.py:168-169) and back (:1438-1441); with ~350 renders per
        view pair at the scene's resolution those copies were most of the orchestrator's own time (tools/pair_profile.py)."""
        tpl = self.get_TrainCameras()[0]
        cam = Camera(colmap_id=-1, R=pose[:3, :3].T, T=pose[:3, 3], FoVx=tpl.FoVx, FoVy=tpl.FoVy, image=None,
                     gt_alpha_mask=None, image_name=None, uid=None, data_device=self.device, cam_confidence=1.0)
        cam.image_height, cam.image_width = self.gs_height, self.gs_width
        with torch.no_grad():
            res = self.gsTrainer.render_view(cam)
        return res["render"].detach(), res["depth"].detach()[0]

    # ------------------------------------------------------------------ SVD side
    def svd_render(self, image_l, image_r, masks, cond_image, output_path, lambda_ts, num_frames=25, save_prefix=""):
        """diffusionGS.py:1088-1116.  The reference re-downloads the checkpoint by model name on every call; here the
        modules are supplied once (`svd_components`: vae, image_encoder, unet) and stay resident."""
        if not self.svd_components:
            raise RuntimeError("svd_render needs svd_components: a local checkpoint directory (str / Path: loaded once with "
                               "StableVideoDiffusionPipeline.from_pretrained) or {'vae':…, 'image_encoder':…, 'unet':…} "
                               "modules; the reference fetches stabilityai/stable-video-diffusion-img2vid-xt by name")
        c = self.svd_components
        if isinstance(c, (str, os.PathLike)):
            # model/diffusionGS.py:1089 with a local directory; loaded on the first call, the modules stay resident
            loaded = StableVideoDiffusionPipeline.from_pretrained(c, torch_dtype=torch.float16, variant="fp16",
                                                                  pipeline=self.variant, device=self.device)
            c = self.svd_components = dict(vae=loaded.vae, image_encoder=loaded.image_encoder, unet=loaded.unet,
                                           dtype=torch.float16, scheduler_config=loaded.scheduler_config)
        # a fresh scheduler per call (the reference builds a fresh pipeline per call), from the checkpoint's own
        # scheduler/scheduler_config.json when the components came from a directory, else the SVD-XT values
        sched = (EulerDiscreteScheduler.from_config(c["scheduler_config"]) if c.get("scheduler_config")
                 else EulerDiscreteScheduler(**SVD_XT_SCHEDULER_CONFIG))
        pipe = StableVideoDiffusionPipeline(c["vae"], c["image_encoder"], c["unet"], sched, variant=self.variant,
                                            device=self.device)
        assert isinstance(cond_image, list)
        frames = pipe([image_l], temp_cond=cond_image + [image_r], mask=masks, lambda_ts=lambda_ts, num_frames=num_frames,
                      decode_chunk_size=8, num_inference_steps=self.num_inference_steps, latent_num=self.latent_num,
                      output_type="np", dtype=c.get("dtype", torch.float16)).frames[0]
        return [frames[i] for i in range(frames.shape[0])]          # [H,W,3] float in [0,1] per frame

    def _interpolate_between_gs_v3(self, idx1, idx2, replace=True, perturb_interp_poses=True):
        """diffusionGS.py:774-923.  With `args.pixel_confidence` (EXTENSION) the fused uncertainty of the inner frames is kept
        instead of discarded: `self._pair_confidence_maps` = `O.confidence_maps_from_uncertainty` of it, one entry per returned
        frame (None for the two end frames; all None on the forward_warp branch, which has no soft uncertainty).  The return
        value is the same either way."""
        self._pair_confidence_maps = None
        pose1, image1, depth1 = self.render_GS(idx1)
        pose2, image2, depth2 = self.render_GS(idx2)
        interpolated_poses = list(O.pose_interpolation(pose1, pose2))
        if perturb_interp_poses:
            sel = O._perturb_and_select_interp_poses(interpolated_poses, [pose1, pose2], K=self.gs_intrinsics,
                                                     render=self._render_device, perturb_num=5, device=self.device)
            interpolated_poses = [pose1] + sel[1:-1] + [pose2]
        Hd, Wd = self.diffusion_height, self.diffusion_width
        # the 25 pseudo-views at the diffusion resolution (cv2.resize INTER_LINEAR of render and depth, :800-805), kept on
        # the device: HWC images / HW depths
        pseudo_images, pseudo_depths, depth_dev = [], [], {}
        for k, p in enumerate(interpolated_poses):
            im, dp = self._render_device(p)
            pseudo_images.append(_resize_linear_t(im, Hd, Wd).permute(1, 2, 0).contiguous())
            pseudo_depths.append(_resize_linear_t(dp, Hd, Wd))
            depth_dev[id(p)] = dp
        rs = lambda x: _resize_nearest(x, Hd, Wd)
        if self.interp_type == "forward_warp":
            if _pixel_confidence(self):
                self._pair_confidence_maps = [None] * len(interpolated_poses)
            return self._finish_forward_warp(interpolated_poses, image1, image2, depth1, depth2, pseudo_images, replace)
        # warps, mask post-processing and the uncertainty fusion stay on the device: one
        # batched warp per end view + two post-processing launches; the condition images go to the pipeline as
        # device tensors
        wd = O.warp_images_bw_device(
            self.diffusion_intrinsics, interpolated_poses, rs(image1), rs(image2), rs(depth1), rs(depth2),
            render_depth=lambda p: _resize_nearest_t(depth_dev[id(p)], Hd, Wd), device=self.device,      # (rendered above)
            h=Hd // 8, w=Wd // 8)
        image_o, image_o2 = rs(image1) / 255.0, rs(image2) / 255.0
        gs_images = torch.stack(pseudo_images[1:-1])
        masks, cond_dev, unc = O.fuse_uncertainty_device(wd["cond_images_ori"], gs_images, wd["soft_masks_reproj_ori"],
                                                         h=Hd // 8, w=Wd // 8)
        if _pixel_confidence(self):
            self._pair_confidence_maps = O.confidence_maps_from_uncertainty(unc, self.gs_height, self.gs_width)
        masks = masks.cpu()
        cond_image = list(cond_dev.permute(0, 3, 1, 2))               # CHW in [0,1], as preprocess_images accepts
        lambda_ts = O.search_hypers_v2(masks, None, type="double_end", diffusion_steps=self.num_inference_steps)
        frames = self.svd_render(image_o, image_o2, masks, cond_image, None, lambda_ts, num_frames=len(interpolated_poses))
        return self._frames_to_gs(frames, image_o, image_o2, replace), interpolated_poses, pseudo_images

    def _frames_to_gs(self, frames, image_o, image_o2, replace):
        """diffusionGS.py:909-916: end frames replaced by the input views, every frame resized to the GS resolution, CHW
        in [0,1].  The reference does this step ON PIL IMAGES (the pipeline returns PIL frames; `fr.resize((W, H))` =
        PIL's default bicubic filter, two uint8 passes with clipping in between) — so it is done with PIL here too:
        25 small host images per view pair, bit-identical to the reference (tests/test_orchestrator.py)."""
        import PIL.Image
        n = len(frames)
        if replace:
            frames[0], frames[-1] = image_o, image_o2
        def one(k):
            v = np.clip(np.asarray(frames[k]) * 255.0, 0, 255)       # in the frame's own dtype, as the reference
            # diffused frames reach the reference as PIL images made by `(f * 255).round()` (tensor2vid / numpy_to_pil);
            # only the two replaced end frames are truncated, `(image_o * 255).astype(np.uint8)` (diffusionGS.py:909-911)
            u8 = v.astype(np.uint8) if (replace and k in (0, n - 1)) else np.rint(v).astype(np.uint8)
            im = PIL.Image.fromarray(u8)
            if (im.height, im.width) != (self.gs_height, self.gs_width):
                im = im.resize((self.gs_width, self.gs_height))
            return torch.from_numpy(np.array(im)).permute(2, 0, 1) / 255.0

        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(8) as ex:                            # PIL's resize releases the GIL: the frames in parallel
            return list(ex.map(one, range(n)))

    def _finish_forward_warp(self, interpolated_poses, image1, image2, depth1, depth2, pseudo_images, replace):
        """`--interp_type forward_warp` (diffusionGS.py:814-815 -> warp_images, :1512).  In the reference this branch
        cannot complete: both accepted diffusion types contain 'Prob', whose fusion block reads `aux[...]`, a name only
        the backward-warp branch defines (:822 -> NameError).  Here the forward splat's own hard hole masks and masked
        condition images go to the pipeline directly (the soft reprojection confidence the fusion needs does not exist
        for a splat) — an extension, documented as such."""
        Hd, Wd = self.diffusion_height, self.diffusion_width
        image_o, image_o2, masks, cond_image = O.warp_images(
            self.diffusion_intrinsics, interpolated_poses, _resize_linear(image1, Hd, Wd), _resize_linear(image2, Hd, Wd),
            _resize_nearest(depth1, Hd, Wd), _resize_nearest(depth2, Hd, Wd), h=Hd // 8, w=Wd // 8)
        masks = masks.float()
        cond_image = [torch.from_numpy(np.ascontiguousarray(c)).permute(2, 0, 1) for c in cond_image]
        lambda_ts = O.search_hypers_v2(masks, None, type="double_end", diffusion_steps=self.num_inference_steps)
        frames = self.svd_render(image_o, image_o2, masks, cond_image, None, lambda_ts, num_frames=len(interpolated_poses))
        return self._frames_to_gs(frames, image_o, image_o2, replace), interpolated_poses, pseudo_images

    def densify_views(self, cycle_num, down_sample_rate=1, densify_type="interpolate", num_views_for_pcd_densification=4):
        """diffusionGS.py:179-343.  View densification per input-view pair (HOT LOOP B), the key-frame / input-frame
        bookkeeping (:221-224,268-294) and, for `num_views_for_pcd_densification > 1`, the point-cloud densification:
        `densify_pcds` on the key frames, then the cloud filter (`syn3r_amd.pcd`: stride `n // 100000`, statistical outlier
        removal k = 20 / 3 sigma on the device) and `dense_views/dense_views_cyc{c}.ply` (:302-336).
        With `args.pixel_confidence` (EXTENSION, off by default) `self.dense_confidence_maps` becomes a list parallel to the
        returned `dense_views` - a [H,W] confidence map for a diffused inner frame, None for an input view - that follows the same
        bookkeeping (`down_sample_rate` picks, `frames[:-1]`, the open chain's last view), and the pair's `.pt` cache gets a third
        key `confidence_maps` (a cache without it loads as all None).  Without the flag nothing is kept and no key is added."""
        dense_views, dense_poses, key_frame_mask, input_flags = [], [], [], []
        dense_maps = [] if _pixel_confidence(self) else None
        os.makedirs(os.path.join(self.save_dir, "dense_views"), exist_ok=True)
        for i in range(self.num_input_views):
            saving_path = os.path.join(self.save_dir, "dense_views" f"interpolated_dense_views_cyc{cycle_num}_view{i}.pt")
            if os.path.exists(saving_path):
                data = torch.load(saving_path, weights_only=False)
                frames, poses = data["views"], data["poses"]
                cmaps = data.get("confidence_maps") or [None] * len(frames)
            else:
                if densify_type == "interpolate_loop0_gs":
                    if i == self.num_input_views - 1:
                        break
                    frames, poses, _ = self._interpolate_between_gs_v3(i, (i + 1) % self.num_input_views, replace=True,
                                                                       perturb_interp_poses=True)
                elif densify_type == "interpolate_gs_v2":
                    frames, poses, _ = self._interpolate_between_gs_v3(i, (i + 1) % self.num_input_views, replace=True)
                else:
                    raise NotImplementedError(f"{densify_type} not supported")
                cmaps = getattr(self, "_pair_confidence_maps", None) or [None] * len(frames)
                if down_sample_rate < 1:
                    idx = np.linspace(0, len(frames) - 1, int(len(frames) * down_sample_rate), dtype=int)
                    frames, poses, cmaps = [frames[k] for k in idx], [poses[k] for k in idx], [cmaps[k] for k in idx]
            input_flags.extend([True] + [False] * (len(frames) - 2))           # a pair's first frame is an input view
            dense_views.extend(frames[:-1])
            dense_poses.extend(poses[:-1])
            if dense_maps is not None:
                assert len(cmaps) == len(frames)
                dense_maps.extend(cmaps[:-1])
            key_frame_mask.extend(list(O.key_frame_template(poses, len(frames), num_views_for_pcd_densification,
                                                            bool(self.fps_keyframe_sampling))))
            if densify_type == "interpolate_loop0_gs" and i == self.num_input_views - 2:
                input_flags.append(True)                                       # the open chain's last input view
                dense_views.append(frames[-1])
                dense_poses.append(poses[-1])
                key_frame_mask.append(True)
                if dense_maps is not None:
                    dense_maps.append(cmaps[-1])
            assert len(dense_views) == len(dense_poses) == len(key_frame_mask) == len(input_flags)
            assert dense_maps is None or len(dense_maps) == len(dense_views)
            if _pixel_confidence(self):
                torch.save({"views": frames, "poses": poses,
                            "confidence_maps": [None if m is None else m.detach().cpu() for m in cmaps]}, saving_path)
            else:
                torch.save({"views": frames, "poses": poses}, saving_path)
        self.dense_confidence_maps = dense_maps
        dense_pcds = None
        if num_views_for_pcd_densification > 1:
            key = np.nonzero(key_frame_mask)[0]
            trimesh_scene = self.densify_pcds([dense_views[k] for k in key], [dense_poses[k] for k in key],
                                              key_frame_mask=[True] * len(key), input_flags=[input_flags[k] for k in key],
                                              win_samples=-1)
            cloud = trimesh_scene.geometry["geometry_0"]
            from . import pcd as P
            dense_pcds = P.filter_dense_cloud(cloud.vertices, cloud.colors, self.device)        # :314-334
            P.write_point_cloud(os.path.join(self.save_dir, "dense_views", f"dense_views_cyc{cycle_num}.ply"), dense_pcds)
        return dense_views, dense_poses, dense_pcds

    def densify_pcds(self, diffused_frames, interpolated_poses, key_frame_mask=None, input_flags=None, win_samples=-1):
        """diffusionGS.py:347-435.  Every candidate frame is rendered from the Gaussians and compared with its diffused
        frame by the trainer's correspondence mask (`gsTrainer.generate_corresp_mask(..., dist_thresh=3, desc_only=False)`:
        the flow network is an attribute of the trainer, the cycle test is `syn3r_flow_cycle_mask`); frames whose mask
        mean exceeds 0.3 — and every input view — go to dust3r (`self.dust3r`, the trainer's attribute as in the
        reference :51) with camera-to-world poses, intrinsics scaled to a 512-wide image and the complete pair graph of
        the kept key frames.  Returns dust3r's trimesh scene."""
        assert len(diffused_frames) == len(interpolated_poses)
        if key_frame_mask is not None:
            assert len(diffused_frames) == len(key_frame_mask)
        if self.dust3r is None:
            raise RuntimeError("densify_pcds needs gsTrainer.dust3r (the reference's trainer attribute, diffusionGS.py:51): "
                               "an object with to(device) / run(frames, c2w_poses=, intrinsics=, preset_pairs=)")
        if isinstance(diffused_frames[0], torch.Tensor):
            diffused_frames = [im.permute([1, 2, 0]).cpu().numpy() * 255 for im in diffused_frames]
        num_frames = len(diffused_frames)
        kept_frames, kept_c2w, kept_K, kept_key_inds = [], [], [], []
        for i in range(num_frames):
            _, image, _, _ = self.render_GS(pose=interpolated_poses[i], return_alpha=True)
            masks, _ = self.gsTrainer.generate_corresp_mask(
                gs_renderings=[torch.from_numpy(np.ascontiguousarray(image))],
                svd_outputs=[torch.from_numpy(np.ascontiguousarray(diffused_frames[i].transpose([2, 0, 1])))],
                dist_thresh=3, desc_only=False)
            share = float(masks[0][0].mean())
            if (i == 0 or i == num_frames - 1) and share < 0.2:
                print("Warning: Weird phenomenon, the first or last frame is not good, please check the input images")
            if share > 0.3 or (input_flags is not None and input_flags[i]):
                if key_frame_mask is not None and key_frame_mask[i]:
                    kept_key_inds.append(len(kept_frames))
                kept_frames.append(diffused_frames[i])
                kept_c2w.append(np.linalg.inv(interpolated_poses[i]))
                K = self.gs_intrinsics.copy()
                K[:2] = K[:2] * 512 / self.gs_width
                kept_K.append(K)
        self.dust3r.to("cuda")
        key_frames = [kept_frames[k] for k in kept_key_inds]
        if hasattr(self.dust3r, "make_pairs"):
            pairs = self.dust3r.make_pairs(key_frames, scene_graph="complete", global_image_inds=kept_key_inds)
        else:
            pairs = O.complete_pair_graph(kept_key_inds)
        _, trimesh_scene = self.dust3r.run(kept_frames, c2w_poses=kept_c2w, intrinsics=kept_K, preset_pairs=pairs)
        self.dust3r.to("cpu")
        return trimesh_scene

    def refine_GS(self, dense_views, dense_poses, intrinsics, cam_confidence=0.01, gs_start_iter=0,
                  disable_densification=False, load_iteration=None, pseudo_cam_sampling_rate=1, load_ckpt=True, confidence_maps=None):
        """diffusionGS.py:1608-1643: reload the latest refined (else the initial) checkpoint, append the dense views to
        the training cameras, finetune, restore the original cameras.  `confidence_maps` (EXTENSION; `run` passes
        `self.dense_confidence_maps` when `args.pixel_confidence` is set): per-pixel maps parallel to `dense_views`, handed to
        `update_cameras`."""
        import glob
        tr = self.gsTrainer
        model_path = getattr(tr.scene, "model_path", None)
        if load_ckpt and model_path:
            refine_ckpts = glob.glob(f"{model_path}/refine_*_chkpnt*.pth")
            if len(refine_ckpts) > 0:
                refine_ckpts = sorted(refine_ckpts, key=lambda x: int(os.path.basename(x).split("_")[1]))
                tr.load_checkpoint(checkpoint=refine_ckpts[-1])                       # the latest refined GS
            else:
                checkpoint_path = None
                if tr.checkpoint_iterations:
                    checkpoint_path = os.path.join(model_path, "chkpnt" + str(tr.checkpoint_iterations[-1]) + ".pth")
                if checkpoint_path is None or not os.path.exists(checkpoint_path):
                    checkpoint_path = os.path.join(model_path, "chkpnt_latest.pth")
                tr.load_checkpoint(checkpoint=checkpoint_path)                        # the initial GS
        # the reference deep-copies scene.train_cameras (:1627); the camera objects are not replaced by a finetune (pose refinement, when on, moves them in place: kept), so
        # copying the lists is enough to restore them (:1641)
        self.original_GS_train_cameras_bak = {k: list(v) for k, v in tr.scene.train_cameras.items()}
        if confidence_maps is not None:
            tr.update_cameras(dense_views, dense_poses, intrinsics, cam_confidences=cam_confidence, append=True,
                              load_iteration=load_iteration, confidence_maps=confidence_maps)
        else:
            tr.update_cameras(dense_views, dense_poses, intrinsics, cam_confidences=cam_confidence, append=True,
                              load_iteration=load_iteration)
        tr.reset_optimizers()
        tr.reset_gs()
        tr.finetune(0, self.refine_epoch, disable_densification=disable_densification,
                    pseudo_cam_sampling_rate=pseudo_cam_sampling_rate)
        if hasattr(tr, "flush_pose_updates"):
            tr.flush_pose_updates()                      # (pose refinement: what is pending belongs to the cameras of this finetune)
        tr.scene.train_cameras = self.original_GS_train_cameras_bak                   # restore the original GS cameras
        self.refine_epoch += 1

    def run(self, refine_cycles=1):
        """diffusionGS.py:1668-1697."""
        self.init_GS()
        for i in range(refine_cycles):
            dense_views, dense_poses, dense_pcds = self.densify_views(
                cycle_num=i, down_sample_rate=1, densify_type=self.densify_type,
                num_views_for_pcd_densification=self.args.num_views_for_pcd_densification)
            if dense_pcds is not None:                                                # :1683-1687
                self.gsTrainer.reset_gaussians_from_pcd(dense_pcds, append_to_old_gaussians=(i != 0))
            self.gsTrainer.opt.use_lpips_loss = True                                  # :1690
            self.refine_GS(dense_views=dense_views, dense_poses=dense_poses, intrinsics=self.gs_intrinsics,
                           cam_confidence=self.cam_confidence, load_iteration=None,
                           pseudo_cam_sampling_rate=self.pseudo_cam_sampling_rate, load_ckpt=(i > 0),
                           **({"confidence_maps": self.dense_confidence_maps} if _pixel_confidence(self) else {}))
            self.gsTrainer.opt.use_lpips_loss = False                                 # :1697
