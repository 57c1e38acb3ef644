#!/usr/bin/env python
"""Times the native grid sort of PngCompression (csrc/plas.hip through gsplat_amd.compression.sort) against the torch composition
that defines it (plas_blur_torch + plas_step_torch on the same device) and writes profiles/plas_sort.json.

Two grids: `--side` x `--side` x 14 (default 1000) with synthetic correlated features made on the device from a seed (smooth
functions of three uniform coordinates plus noise, min-max normalised), and `--garden-side` squared (default 334) with the garden
fixture's real points and colours (tests/_plas_cases.py: fixture_splats). Alternating windows, each the median of `--iters` calls
between device events after a warm-up call, at the large grid, of
  blur        gsx_plas_blur and plas_blur_torch at a large, a middle and the smallest radius
  step        gsx_plas_step and plas_step_torch (one step each on a copy of the same grid, without the host read)
and, on a host clock around a synchronise, the whole plas_sort at both grids, its step count and the host reads it made per step
(counted by wrapping Tensor.tolist / item / cpu for the run). The torch composition is run whole at the garden grid; at the large
grid one torch step (blur + step + host read) is timed per radius of the schedule and multiplied by the number of steps the fused
run took at that radius: an extrapolation, stated as such - the full torch run is not made unless --torch-whole is given. At the
garden grid also the summed bytes of the six PNGs under the Morton layout and under the native sort. With --kernel-resources FILE
(tools/plas_resources.py) the kernels' registers, LDS and occupancy are copied in.

usage: python tools/plas_bench.py [--iters 5] [--windows 3] [--out profiles/plas_sort.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gsplat_amd.compression import PngCompression  # noqa: E402
from gsplat_amd.compression import sort as S  # noqa: E402
from gsplat_amd.compression.png_compression import log_transform  # noqa: E402

DEV = "cuda"


def clock_state():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln or "Performance Level" in ln][:6]
    except Exception as e:  # the tool is optional
        return [f"unavailable: {e}"]


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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def synthetic_features(side, channels=14, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = side * side
    pos = torch.rand(n, 3, generator=g, device=DEV)
    mix = torch.randn(3, channels, generator=g, device=DEV) * 3.0
    feats = torch.sin(pos @ mix) + 0.1 * torch.randn(n, channels, generator=g, device=DEV)
    feats[:, :3] = pos
    lo, hi = feats.amin(0), feats.amax(0)
    return ((feats - lo) / (hi - lo)).contiguous()


class HostReads:
    """Counts Tensor.tolist / item / cpu calls while active."""

    def __enter__(self):
        self.count, self._saved = 0, {}
        for name in ("tolist", "item", "cpu"):
            orig = getattr(torch.Tensor, name)
            self._saved[name] = orig

            def counted(t, *a, _orig=orig, **k):
                self.count += int(t.is_cuda)
                return _orig(t, *a, **k)

            setattr(torch.Tensor, name, counted)
        return self

    def __exit__(self, *exc):
        for name, orig in self._saved.items():
            setattr(torch.Tensor, name, orig)
        return False


def steps_per_radius(H, W, feats, seed):
    """[(r, b, steps)] of the fused run: the loop of plas_sort with the steps counted per radius."""
    grid = feats.clone().reshape(H, W, -1)
    index = torch.arange(H * W, dtype=torch.int32, device=feats.device).reshape(H, W)
    t, out = 0, []
    for r, b in S._plas_schedule(H, W, 0.9):
        n = 0
        for _ in range(64):
            imp, tot = S._step_fused(grid, S._blur_fused(grid, r), index, b, seed, t).tolist()
            t, n = t + 1, n + 1
            if not imp > 1e-4 * tot:
                break
        out.append((r, b, n))
    return out


def measure_large(side, args, result):
    feats = synthetic_features(side)
    assert S._plas_fused_ok(feats)
    H = W = side
    grid = feats.reshape(H, W, -1)
    index32 = torch.arange(H * W, dtype=torch.int32, device=DEV).reshape(H, W)
    index64 = index32.long()
    radii = {"large": side // 2 - 1, "middle": max(1, side // 16), "smallest": 1}
    entry = {"side": side, "channels": feats.shape[1], "blur_ms": {}, "step_ms": {"fused": [], "torch": []}}
    target = S._blur_fused(grid, radii["middle"])
    b = 64
    for name, r in radii.items():
        entry["blur_ms"][name] = {"r": r, "fused": [], "torch": []}
    for _ in range(args.windows):
        for name, r in radii.items():
            entry["blur_ms"][name]["fused"].append(timed(lambda: S._blur_fused(grid, r), args.iters))
            entry["blur_ms"][name]["torch"].append(timed(lambda: S.plas_blur_torch(grid, r), max(1, args.iters // 2)))
        entry["step_ms"]["fused"].append(timed(lambda: S._step_fused(grid.clone(), target, index32.clone(), b, 0, 1), args.iters))
        entry["step_ms"]["torch"].append(timed(lambda: S._step_values(grid.clone(), target, index64.clone(), b, 0, 1), args.iters))
    copy_ms = timed(lambda: (grid.clone(), index32.clone()), args.iters)
    entry["step_ms"]["note"] = f"both include a copy of the grid and the index ({copy_ms:.3f} ms for the float32 / int32 pair)"
    with HostReads() as reads:
        entry["plas_sort_s"] = [wall(lambda: S.plas_sort(feats, H, W, seed=0))[0]]
    entry["steps"] = S.last_steps
    entry["host_reads_per_step"] = reads.count / max(1, S.last_steps)
    entry["plas_sort_s"].append(wall(lambda: S.plas_sort(feats, H, W, seed=0))[0])
    if args.torch_whole:
        entry["plas_sort_torch_s"] = [wall(lambda: S.plas_sort_torch(feats, H, W, seed=0))[0]]
    else:
        per_radius = steps_per_radius(H, W, feats, 0)
        g, ix = grid.clone(), index64.clone()
        total, t = 0.0, 0
        for r, b, n in per_radius:
            S.plas_step_torch(g, S.plas_blur_torch(g, r), ix, b, 0, t)  # warm
            total += n * wall(lambda: S.plas_step_torch(g, S.plas_blur_torch(g, r), ix, b, 0, t + 1))[0]
            t += n
        entry["plas_sort_torch_s_extrapolated"] = total
        entry["note"] = ("plas_sort_torch_s_extrapolated = one timed torch step (blur + step + host read) per radius of the schedule x "
                         "the steps the fused run took at that radius: an extrapolation, not a measurement of the full run")
    torch_s = entry.get("plas_sort_torch_s", [entry.get("plas_sort_torch_s_extrapolated")])[0]
    entry["ratio_torch_over_fused"] = torch_s / max(entry["plas_sort_s"])
    result["large"] = entry
    print(json.dumps(entry), flush=True)


def measure_garden(side, args, result):
    import _plas_cases as pc

    sp = pc.fixture_splats(side)
    pre = dict(sp, means=log_transform(sp["means"]), quats=torch.nn.functional.normalize(sp["quats"], dim=-1))
    feats_cpu = S._sort_features(pre)
    shuffle = torch.randperm(side * side, generator=torch.Generator().manual_seed(0))
    feats = feats_cpu[shuffle].to(DEV).contiguous()
    assert S._plas_fused_ok(feats)
    entry = {"side": side, "channels": feats.shape[1], "plas_sort_s": [], "plas_sort_torch_s": []}
    S.plas_sort(feats, side, side, seed=0)  # warm
    for _ in range(args.whole):
        s, order = wall(lambda: S.plas_sort(feats, side, side, seed=0))
        entry["plas_sort_s"].append(s)
        entry["steps"] = S.last_steps
        s, order_torch = wall(lambda: S.plas_sort_torch(feats, side, side, seed=0))
        entry["plas_sort_torch_s"].append(s)
    entry["ratio_torch_over_fused"] = [t / f for t, f in zip(entry["plas_sort_torch_s"], entry["plas_sort_s"])]
    orders = {"morton": pc.morton_order(pre["means"]), "native": shuffle[order.cpu()], "torch_composition": shuffle[order_torch.cpu()]}
    entry["roughness"] = {k: pc.roughness(feats_cpu, o, side, side) for k, o in orders.items()}
    entry["roughness"]["unsorted"] = pc.roughness(feats_cpu, torch.arange(side * side), side, side)
    entry["png_bytes"] = {}
    for name, o in orders.items():
        with tempfile.TemporaryDirectory() as tmp:
            PngCompression(use_sort=False, verbose=False).compress(tmp, {k: v[o] for k, v in sp.items()})
            entry["png_bytes"][name] = pc.png_bytes(tmp)
    result["garden"] = entry
    print(json.dumps(entry), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=5)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--side", type=int, default=1000)
    p.add_argument("--garden-side", type=int, default=334)
    p.add_argument("--whole", type=int, default=2)
    p.add_argument("--torch-whole", action="store_true", help="run the torch composition whole at the large grid too")
    p.add_argument("--kernel-resources", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "plas_sort.json"))
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plas_bench: needs a ROCm GPU; nothing is measured without one")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "windows": args.windows, "clock_state": clock_state()}
    if args.kernel_resources:
        with open(args.kernel_resources) as f:
            result["kernels"] = json.load(f)
    with torch.no_grad():
        for fn, side in ((measure_garden, args.garden_side), (measure_large, args.side)):
            fn(side, args, result)
            with open(args.out, "w") as fh:  # after every grid: a run that is cut short leaves what it measured
                json.dump(result, fh, indent=1)
    result["clock_state_after"] = clock_state()
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)
    if min(result["garden"]["ratio_torch_over_fused"]) <= 1.0 or result["large"]["ratio_torch_over_fused"] <= 1.0:
        raise SystemExit("the fused sort was not faster than the torch composition")


if __name__ == "__main__":
    main()
