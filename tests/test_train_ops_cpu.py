"""`syn3r_amd.gs.train_ops` is a package of one module per operator family; every caller imports from its root."""

PUBLIC = ["FusedAdam", "camera_table", "compute_filter_3D", "depth_correlation_local_loss", "depth_correlation_local_loss_step",
          "depth_correlation_local_records", "depth_correlation_loss", "depth_correlation_loss_step", "depth_edge_weights",
          "depth_smoothness_loss", "depth_smoothness_loss_step", "exposure_apply", "exposure_apply_step", "exposure_backward_step",
          "image_metrics", "knn3_graph", "knn3_mean_dist2", "l1_loss", "l1_loss_step", "mcmc_noise", "mcmc_reg_step", "mcmc_relocate",
          "mcmc_sample", "mcmc_weights", "photometric_loss", "photometric_loss_step", "proximity_unpool"]


def test_package_root_exports_every_public_name():
    """the 27 names the single-file module defined without a leading underscore"""
    from syn3r_amd.gs import train_ops
    missing = [name for name in PUBLIC if not callable(getattr(train_ops, name, None))]
    assert not missing, missing
