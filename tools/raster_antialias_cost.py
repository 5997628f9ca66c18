"""What `GaussianRasterizationSettings.antialiasing` costs on the bench scene (developer tool; profiles/r10/raster_antialias.txt).

    python tools/raster_antialias_cost.py [--iters 200] [--rounds 3]     raster fwd+bwd iteration and full trainer iteration, filter
                                                                          off / on alternating, host clock around a synchronised loop
    rocprofv3 --kernel-trace --stats -d DIR -o aa -- python tools/raster_antialias_cost.py --profile 20
                                                                          20 iterations of each mode and nothing else: the kernel
                                                                          names carry the template arguments (k_preprocess<true> is
                                                                          the filter's instance, k_preprocess_bwd<true, true> too)

The library launches both instances of each kernel under the one trace name (`k_preprocess`, `k_preprocess_bwd`: bench.py's per-kernel
tables are keyed by it), so those tables cannot tell the filter on from off; only the profiler's own kernel names, as above, can.
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch  # noqa: E402

import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--profile", type=int, default=0, metavar="N", help="only N iterations per mode, no timing (run under rocprofv3)")
mine = ap.parse_args()
sys.argv = sys.argv[:1]
args = bench.parse()

from syn3r_amd import raster  # noqa: E402
from syn3r_amd.raster import GaussianRasterizer  # noqa: E402

dev = torch.device("cuda", 0)
loop = bench.RasterLoop(args, dev)
base = loop.rast.raster_settings
rast = {aa: GaussianRasterizer(base._replace(antialiasing=aa)) for aa in (False, True)}


def run(aa, n):
    loop.rast = rast[aa]
    for _ in range(n):
        loop.iteration()
    torch.cuda.synchronize()


if mine.profile:
    for aa in (False, True):
        run(aa, mine.profile)
    raster.flush_pair_checks()
    print("ok")
    sys.exit(0)

for aa in (False, True):
    run(aa, 10)
print(f"scene: {args.gaussians} Gaussians, {args.height}x{args.width}; {mine.iters} iterations per timing, {mine.rounds} rounds, off / on alternating")
for r in range(mine.rounds):
    row = []
    for aa in (False, True):
        t0 = time.perf_counter()
        run(aa, mine.iters)
        row.append((time.perf_counter() - t0) / mine.iters * 1e3)
    print(f"round {r}: raster fwd+bwd iteration  off {row[0]:.4f} ms   on {row[1]:.4f} ms   on/off {row[1] / row[0]:.4f}")
for r in range(mine.rounds):
    row = []
    for aa in (False, True):
        loop.rast = rast[aa]
        row.append(loop.full_iteration_rate(50))
    print(f"round {r}: full trainer iteration    off {row[0]:.1f} /s   on {row[1]:.1f} /s   on/off {row[1] / row[0]:.4f}")
raster.flush_pair_checks()
