"""Which kernels of the library three `GSTrainer.train_step` calls launch, and how often, per step route and option set: the table
tests/test_trainer_launches_gpu.py holds a change of the trainer's HOST code against.  Public names only (`measure.synthetic_scene`,
`OptimizationParams`, `train_step`, `_lib.kernel_trace`), so the same file runs on the commit before such a change and on the one
after.  A plain module: no fixtures, nothing collected.

    python tests/trainer_launches.py > tests/data/trainer_launches.json

records every configuration TWICE (fresh trainers) and writes the table; a kernel whose count differs between the two recordings is
data dependent: it is left out of that configuration's table and named under "left_out".  The committed table is recorded on the
PARENT of the commit that is tested, never on the tree under test."""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

TABLE = Path(__file__).resolve().parent / "data" / "trainer_launches.json"
N, H, W, VIEWS = 300, 33, 50, 2              # the smallest scene of the suite with edge tiles and culled Gaussians
WARMUP, STEPS = 2, 3
ALL_ON = dict(antialiasing=True, filter_3d=True, densify_abs_grad=True, pose_opt=True, pose_opt_interval=2, depth_weight=0.05,
              lambda_dssim=0.2)
# name -> (OptimizationParams fields, camera extras (depth_image and confidence_map), density control)
OPTIONS = {"off": ({}, False, False), "all_on": (ALL_ON, True, False), "l1": (dict(lambda_dssim=0.0), False, False),
           "density": (dict(densify_until_iter=1000, densification_interval=1000), False, True)}
CONFIGS = [(route, name) for route in ("explicit", "autograd") for name in OPTIONS]


def key(route: str, name: str) -> str:
    return f"{route}/{name}"


def launches(dev, route: str, name: str) -> dict:
    """{kernel name: calls} over STEPS train_step calls (cameras in turn) after WARMUP of them, on a fresh trainer"""
    from syn3r_amd import _lib as L
    from syn3r_amd import measure
    from syn3r_amd.gs import OptimizationParams
    fields, extras, density = OPTIONS[name]
    tr = measure.synthetic_scene(dev, N, H, W, VIEWS, 10, None)
    tr.opt = OptimizationParams(iterations=10, **fields)
    tr.densify = density
    cams = tr.scene.getTrainCameras()
    if extras:
        gen = torch.Generator().manual_seed(7)
        for cam in cams:
            cam.depth_image = (0.5 + 4.0 * torch.rand(H, W, generator=gen)).to(dev)
            cam.confidence_map = torch.rand(H, W, generator=gen)
    for k in range(WARMUP):
        tr.train_step(cams[k % VIEWS], explicit=route == "explicit")
    torch.cuda.synchronize(dev)
    with L.kernel_trace() as trace:
        for k in range(WARMUP, WARMUP + STEPS):
            tr.train_step(cams[k % VIEWS], explicit=route == "explicit")
        torch.cuda.synchronize(dev)
    return {kernel: int(calls) for kernel, (calls, _) in sorted(trace.result.items())}


def expected() -> dict:
    return json.loads(TABLE.read_text())


def main():
    dev = torch.device("cuda", 0)
    first = {key(*c): launches(dev, *c) for c in CONFIGS}
    second = {key(*c): launches(dev, *c) for c in CONFIGS}
    table, left_out = {}, {}
    for k in first:
        unstable = sorted(n for n in set(first[k]) | set(second[k]) if first[k].get(n) != second[k].get(n))
        table[k] = {n: c for n, c in first[k].items() if n not in unstable}
        if unstable:
            left_out[k] = unstable
    print(json.dumps({"comment": f"{{kernel: calls}} over {STEPS} train_step calls after {WARMUP}, {N} Gaussians, {H} x {W}, {VIEWS} cameras; "
                                 "recorded twice by tests/trainer_launches.py on the parent commit, kernels whose count differed between "
                                 "the two recordings (data dependent) under left_out", "left_out": left_out, "launches": table},
                     indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
