"""SHA-256 digests of the rasteriser's results on the test scenes (developer tool): are two builds of the library the same bits?

    python tools/raster_digest.py > digest.txt          (in each tree; the two files must be the same text)

Only `rasterize_forward` / `rasterize_backward` are used.  For the three scenes of tests/raster_aa_ref.SHAPES (without the Gaussians
tests/raster_f3d_ref.scene leaves out) x {activated, raw} x {plain, antialias} x {no filter, the scene's filter}: one digest of
colour, depth, alpha and radii, and one of every gradient tensor with the upstream gradients restricted to one 16 x 8 half-tile at a
time (all half-tiles, in order).  With one live half-tile the blend backward's float atomics add in an order that cannot matter
(tests/test_raster_aa_gpu.py's module docstring), so the gradients are the same bits in every launch of one binary."""
import hashlib
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import raster_aa_ref as A  # noqa: E402
import raster_f3d_ref as F  # noqa: E402
from syn3r_amd.raster import GaussianRasterizationSettings, rasterize_backward, rasterize_forward  # noqa: E402

dev = torch.device("cuda", 0)


def add(h, *tensors):
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())


for shape in A.SHAPES:
    sc, deg = F.scene(shape), shape[4]
    H, W = sc["H"], sc["W"]
    f = lambda t: t.to(dev, torch.float32).contiguous()
    gen = torch.Generator(device="cpu").manual_seed(29)
    gc, gd, ga = (torch.randn(c, H, W, generator=gen).to(dev) for c in (3, 1, 1))
    for raw in (False, True):
        p = F.raw_params(sc) if raw else sc
        for aa in (False, True):
            st = GaussianRasterizationSettings(H, W, sc["tfx"], sc["tfy"], f(sc["bg"]), 1.0, f(sc["view"]), f(sc["proj"]), deg,
                                               f(sc["campos"]), False, False, aa)
            for filt in (None, sc["f"]):
                with torch.no_grad():
                    color, radii, depth, alpha, state = rasterize_forward(
                        f(sc["m"]), f(sc["sh"]), f(p["o"]), f(p["s"]), f(p["q"]), f(sc["cf"]) if sc["cf"] is not None else None, st,
                        raw_params=raw, filter_3D=f(filt) if filt is not None else None)
                    fwd, bwd = hashlib.sha256(), hashlib.sha256()
                    add(fwd, color, depth, alpha, radii)
                    for y0 in range(0, H, 8):
                        for x0 in range(0, W, 16):
                            m = torch.zeros(1, H, W, device=dev)
                            m[:, y0:y0 + 8, x0:x0 + 16] = 1.0
                            add(bwd, *[g for g in rasterize_backward(state, gc * m, gd * m, ga * m) if g is not None])
                print(f"N{sc['N']}_{H}x{W} {'raw' if raw else 'activated':<9} {'antialias' if aa else 'plain':<9} "
                      f"{'filter' if filt is not None else 'nofilter':<8} visible {int((radii > 0).sum()):4d}  fwd {fwd.hexdigest()}  "
                      f"bwd {bwd.hexdigest()}")
