#!/usr/bin/env python
"""Times the fused nearest-neighbour scale initialisation (csrc/knn.hip through gsplat_amd.knn_scale_init) against its torch
composition (knn_scale_init_torch: what a user without the kernels would run; nothing on the parent commit runs at all) and
writes profiles/knn_init.json.

Clouds: `clustered` (tests/_knn_cases.py: half a blob of sigma 0.05, a quarter a blob of sigma 1, a quarter uniform in a 20-unit
box, 8 outliers at sigma 500, 8 duplicates) and `garden` (the means of tests/golden/garden_scene.npz, repeated on a 4-unit
lattice of copies until N points are there). Per cloud and size: alternating windows of fused and torch, each window the median
of `--iters` calls between device events after a warm-up call; at the sizes of --fused-only the torch form is one timed chunk of
1024 rows times N / 1024, marked as an extrapolation. Recorded per size: the window times, the grid, the number of rows that took
the all-points scan, the largest cell population (recomputed here from the grid the kernel reports) and, with
--kernel-resources FILE (JSON written from the compiler's resource remarks at build time), the kernels' VGPRs, LDS and scratch.

usage: python tools/knn_bench.py [--iters 3] [--windows 3] [--out profiles/knn_init.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _knn_cases as kc  # noqa: E402
from gsplat_amd import init_utils as iu  # noqa: E402

DEV = "cuda"


def garden(N):
    m = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "garden_scene.npz"))["means"].astype(np.float32))
    copies = -(-N // m.shape[0])
    side = int(np.ceil(np.sqrt(copies)))
    parts = [m + torch.tensor([4.0 * (c % side), 4.0 * (c // side), 0.0]) for c in range(copies)]
    return torch.cat(parts)[:N].contiguous()


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def largest_cell(x, st):
    lo = torch.tensor(st["box_min"], device=x.device)
    h = torch.tensor(st["cell_size"], device=x.device)
    dims = torch.tensor(st["dims"], device=x.device)
    c = torch.where(h > 0, (x - lo) / h.clamp_min(1e-30), torch.zeros_like(x)).floor().clamp_min(0).long()
    c = torch.minimum(c, dims - 1)
    flat = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    return int(torch.bincount(flat).max())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--both", type=int, nargs="*", default=[50_000, 200_000])
    p.add_argument("--fused-only", type=int, nargs="*", default=[1_000_000, 2_800_000, 6_000_000])
    p.add_argument("--clouds", nargs="*", default=["clustered", "garden"])
    p.add_argument("--kernel-resources", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_init.json"))
    args = p.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "ring_cap": iu.RING_CAP, "k": 3, "sizes": []}
    if args.kernel_resources:
        with open(args.kernel_resources) as f:
            result["kernels"] = json.load(f)
    for cloud in args.clouds:
        for N in list(args.both) + list(args.fused_only):
            x = (kc.clustered(N) if cloud == "clustered" else garden(N)).to(DEV)
            entry = {"cloud": cloud, "N": N, "fused_ms": [], "torch_ms": []}
            with torch.no_grad():
                for _ in range(args.windows):
                    entry["fused_ms"].append(timed(lambda: iu.knn_scale_init(x, 3), args.iters))
                    if N in args.both:
                        entry["torch_ms"].append(timed(lambda: iu.knn_scale_init_torch(x, 3), args.iters))
                st = iu.knn_last_stats()
                entry.update({"grid": st["dims"], "deferred": st["deferred"], "largest_cell": largest_cell(x, st)})
                if N in args.both:
                    entry["ratio"] = [t / u for t, u in zip(entry["torch_ms"], entry["fused_ms"])]
                    entry["fused_wins_every_window"] = all(t > u for t, u in zip(entry["torch_ms"], entry["fused_ms"]))
                    a, b = iu.knn_scale_init(x, 3), iu.knn_scale_init_torch(x, 3)
                    entry["max_abs_diff_fused_vs_torch"] = float((a - b).abs().max())
                else:
                    one = timed(lambda: _one_chunk(x), args.iters)
                    entry["torch_one_chunk_of_1024_ms"] = one
                    entry["torch_ms_extrapolated"] = one * N / 1024.0
                    entry["note"] = "torch_ms_extrapolated = one timed chunk x N / 1024: an extrapolation, not a measurement"
            result["sizes"].append(entry)
            print(json.dumps(entry), flush=True)
            with open(args.out, "w") as fh:  # after every size: a run that is cut short leaves what it measured
                json.dump(result, fh, indent=1)
            del x
            torch.cuda.empty_cache()
    print("wrote", args.out)
    lost = [(e["cloud"], e["N"]) for e in result["sizes"] if e.get("fused_wins_every_window") is False]
    if lost:
        raise SystemExit(f"the fused form lost a window to the torch composition at {lost}")


def _one_chunk(x):
    """The work knn_torch does for one chunk of 1024 query rows against all N points."""
    d = [x[:1024, a:a + 1] - x[:, a][None, :] for a in range(3)]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return torch.topk(d2, 4, dim=-1, largest=False, sorted=True)


if __name__ == "__main__":
    main()
