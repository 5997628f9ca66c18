"""Fused trainer-loop operators on the HIP library, re-exported from one module per family: `photo` (image
losses), `depth`, `reproj` (multi-view reprojection), `exposure`, `mcmc`, `cloud` (neighbour search, unpooling, 3D filter), `adam`.  No CPU fallback: `Syn3rError`
without the extension."""
from .adam import FusedAdam
from .cloud import camera_table, compute_filter_3D, knn3_graph, knn3_mean_dist2, proximity_unpool
from .depth import (depth_correlation_local_loss, depth_correlation_local_loss_step, depth_correlation_local_records,
                    depth_correlation_loss, depth_correlation_loss_step, depth_edge_weights, depth_smoothness_loss,
                    depth_smoothness_loss_step)
from .exposure import exposure_apply, exposure_apply_step, exposure_backward_step
from .mcmc import mcmc_noise, mcmc_reg_step, mcmc_relocate, mcmc_sample, mcmc_weights
from .reproj import photo_reprojection_loss, photo_reprojection_loss_step, photo_reprojection_records
from .photo import _photo_entries, image_metrics, l1_loss, l1_loss_step, photometric_loss, photometric_loss_step
