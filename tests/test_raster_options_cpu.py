"""`GaussianRasterizer` refuses an output buffer that requires grad before it touches any tensor (no device needed)."""
import pytest
import torch


@pytest.mark.parametrize("name", ["means2D_abs", "camera_grad"])
def test_a_buffer_that_requires_grad_is_refused(name):
    from syn3r_amd.raster import GaussianRasterizationSettings, GaussianRasterizer
    z = torch.zeros(3)
    st = GaussianRasterizationSettings(4, 4, 1.0, 1.0, z, 1.0, torch.zeros(4, 4), torch.zeros(4, 4), 0, z)
    n = 5
    t = torch.zeros((n, 2) if name == "means2D_abs" else (35,), requires_grad=True)
    with pytest.raises(ValueError, match=f"GaussianRasterizer: {name} is a buffer the backward fills, not a tensor that requires grad"):
        GaussianRasterizer(st)(torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n), shs=torch.zeros(n, 1, 3), scales=torch.zeros(n, 3),
                               rotations=torch.zeros(n, 4), **{name: t})
