#!/usr/bin/env python
"""Times the fused HexPlane field (csrc/hexplane.hip) against its torch composition, which is what a user without the kernels
would run, and writes profiles/hexplane.json.

The default field ([64, 64, 64, 25], scales 1 and 2, 32 channels, bounds 1.6) at 200 000, 1 000 000 and 2 800 000 points drawn
uniformly inside the box, t in [-1, 1]. Per size: `--windows` alternating windows of fused and `hexplane_torch`, forward and
forward + backward (cotangent on the features; xyzt and every plane take a gradient), each window the median of `--iters` calls
between device events after a warm-up. Recorded: the times, the ratio torch / fused per window and whether the fused form won
every window (it is reported, not required). Then, outside the windows, a few fused calls with an event pair around every C
entry point: gsx_hexplane_pack (one launch per scale), _fwd, _bwd (the zeroing of the gradient arena and the kernel) and _unpack,
and from the backward's time the rate of its float atomics, computed from the shapes: scales x 6 planes x 4 corners x 128 B per
point, against the 1.3 TB/s chip-wide figure.

`--ab-lib <libgsplat_amd_NAME.so>`: the layout A/B. NAME is a build of the library with -DGSX_HEXPLANE_CHANNEL_MAJOR=1
(tools/mkvariant.sh chmajor hexplane -DGSX_HEXPLANE_CHANNEL_MAJOR=1): its arena keeps the parameters' [32][cells] layout, so its
sampling kernels read and add the way kernels working on the parameters in place would; what reading in place saves is the pack
and unpack time, which is recorded beside. The entry-point times of both libraries are taken in fresh child processes, started in
turn, `--ab-rounds` each.

`--grid-lib BLOCKS=<libgsplat_amd_NAME.so>` (repeatable): the backward-grid A/B. NAME is a build with
-DGSX_HEXPLANE_BWD_BLOCKS=BLOCKS (the persistent backward grid; the product's is 2048 workgroups of four waves); measured the same
way, the default library standing for 2048.

`--entry-times` is what such a child runs: the entry-point times alone, printed as one JSON line.

usage: python tools/hexplane_bench.py [--iters 10] [--windows 5] [--ab-lib PATH] [--grid-lib BLOCKS=PATH ...]
       [--out profiles/hexplane.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (200_000, 1_000_000, 2_800_000)
DEV = "cuda"
ENTRIES = ("gsx_hexplane_pack", "gsx_hexplane_fwd", "gsx_hexplane_bwd", "gsx_hexplane_unpack")
ATOMIC_RATE_GB_S = 1300.0  # the chip-wide rate of shaped global float atomic adds


def setup(N, seed=0):
    import torch

    from gsplat_amd import hexplane as hp

    torch.manual_seed(seed)
    field = hp.HexPlaneField().to(DEV)
    g = torch.Generator().manual_seed(seed)
    xyzt = torch.rand(N, 4, generator=g) * 2.0 - 1.0
    xyzt[:, :3] *= field.bounds
    w = torch.randn(N, field.feat_dim, generator=g).to(DEV)
    return field, xyzt.to(DEV).requires_grad_(True), w


def timed(fn, iters):
    import torch

    fn()
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


def entry_times(sizes, calls=7):
    """{N: {entry point: median ms per forward + backward}} (pack and unpack: the sum over the scales)."""
    import torch

    from gsplat_amd import _cabi

    out = {}
    for N in sizes:
        field, xyzt, w = setup(N)

        def step():
            xyzt.grad = None
            field.zero_grad(set_to_none=True)
            (field(xyzt) * w).sum().backward()

        step()
        step()
        torch.cuda.synchronize()
        per_call = {k: [] for k in ENTRIES}
        for _ in range(calls):
            _cabi.profile_begin(only=ENTRIES)
            step()
            for k, v in _cabi.profile_end().items():
                per_call[k].append(sum(v))
        out[str(N)] = {k: statistics.median(v) for k, v in per_call.items()}
        del field, xyzt, w
        torch.cuda.empty_cache()
    return out


def child_entry_times(lib):
    env = dict(os.environ)
    if lib:
        env["GSPLAT_AMD_LIB"] = os.path.abspath(lib)
    else:
        env.pop("GSPLAT_AMD_LIB", None)
        env.pop("GSPLAT_AMD_TORCH_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--entry-times"], env=env, capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"entry-time child failed ({lib or 'default library'}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def grid_ab(runs):
    """{blocks: [backward ms per run]} per size, from the children's entry-point times."""
    return {"how": "gsx_hexplane_bwd (ms, median of 7 forward + backward calls) of builds with -DGSX_HEXPLANE_BWD_BLOCKS=<blocks>, "
                   "fresh processes started in turn; 2048 is the default library",
            "sizes": {str(N): {tag: [r[str(N)]["gsx_hexplane_bwd"] for r in rr] for tag, rr in runs.items()} for N in SIZES}}


def layout_ab(runs):
    res = {"how": "entry-point times (ms, median of 7 forward + backward calls) of the default library and of a build with "
                  "-DGSX_HEXPLANE_CHANNEL_MAJOR=1, fresh processes started in turn; per size the runs in order",
           "sizes": {}}
    for N in SIZES:
        e = {}
        for tag, rr in runs.items():
            e[tag] = {k: [r[str(N)][k] for r in rr] for k in ENTRIES}
        last, major = e["channel_last"], e["channel_major"]
        # in place = the channel-major sampling kernels without pack and unpack; the product = everything of channel-last
        e["in_place_ms"] = min(major["gsx_hexplane_fwd"]) + min(major["gsx_hexplane_bwd"])
        e["channel_last_with_pack_and_unpack_ms"] = sum(min(last[k]) for k in ENTRIES)
        e["channel_last_is_faster"] = e["channel_last_with_pack_and_unpack_ms"] < e["in_place_ms"]
        res["sizes"][str(N)] = e
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=10)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "hexplane.json"))
    p.add_argument("--ab-lib", default=None)
    p.add_argument("--ab-rounds", type=int, default=2)
    p.add_argument("--grid-lib", action="append", default=[], metavar="BLOCKS=PATH")
    p.add_argument("--entry-times", action="store_true")
    args = p.parse_args()
    if args.entry_times:
        print(json.dumps(entry_times(SIZES)), flush=True)
        return
    # the children first: this process has no GPU state yet
    libs = {"channel_last": None}
    if args.ab_lib:
        libs["channel_major"] = args.ab_lib
    libs.update(dict(g.split("=", 1) for g in args.grid_lib))
    runs = {tag: [] for tag in libs}
    if len(libs) > 1:
        for _ in range(args.ab_rounds):
            for tag, lib in libs.items():
                runs[tag].append(child_entry_times(lib))
    ab = layout_ab({k: runs[k] for k in ("channel_last", "channel_major")}) if args.ab_lib else None
    grid = grid_ab({("2048" if k == "channel_last" else k): v for k, v in runs.items() if k != "channel_major"}) if args.grid_lib else None

    import torch

    from gsplat_amd import hexplane as hp

    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "windows": args.windows,
              "field": {"resolution": [64, 64, 64, 25], "multires": [1, 2], "channels": 32, "bounds": 1.6}, "sizes": []}
    for N in SIZES:
        field, xyzt, w = setup(N)

        def fwd(fn):
            with torch.no_grad():
                fn(field, xyzt)

        def both(fn):
            xyzt.grad = None
            field.zero_grad(set_to_none=True)
            (fn(field, xyzt) * w).sum().backward()

        rows = {"fused_fwd": [], "torch_fwd": [], "fused_fwd_bwd": [], "torch_fwd_bwd": []}
        for _ in range(args.windows):
            rows["fused_fwd"].append(timed(lambda: fwd(hp.hexplane), args.iters))
            rows["torch_fwd"].append(timed(lambda: fwd(hp.hexplane_torch), args.iters))
            rows["fused_fwd_bwd"].append(timed(lambda: both(hp.hexplane), args.iters))
            rows["torch_fwd_bwd"].append(timed(lambda: both(hp.hexplane_torch), args.iters))
        entry = {"N": N, "ms": rows,
                 "ratio_fwd": [t / u for t, u in zip(rows["torch_fwd"], rows["fused_fwd"])],
                 "ratio_fwd_bwd": [t / u for t, u in zip(rows["torch_fwd_bwd"], rows["fused_fwd_bwd"])]}
        entry["fused_wins_every_window"] = all(r > 1.0 for r in entry["ratio_fwd"] + entry["ratio_fwd_bwd"])
        del field, xyzt, w
        torch.cuda.empty_cache()
        result["sizes"].append(entry)
        print(json.dumps(entry), flush=True)
    per_entry = entry_times(SIZES)
    for entry in result["sizes"]:
        ms = per_entry[str(entry["N"])]
        atomic_bytes = entry["N"] * 2 * 6 * 4 * 128
        entry["entry_ms"] = ms
        entry["atomic_bytes"] = atomic_bytes
        entry["atomic_gb_per_s"] = atomic_bytes / ms["gsx_hexplane_bwd"] / 1e6
        entry["atomic_share_of_1300_gb_per_s"] = entry["atomic_gb_per_s"] / ATOMIC_RATE_GB_S
        entry["fwd_features_gb_per_s"] = entry["N"] * 64 * 4 / ms["gsx_hexplane_fwd"] / 1e6
    result["lost_at"] = [e["N"] for e in result["sizes"] if not e["fused_wins_every_window"]]
    result["layout_ab"] = ab if ab is not None else "not measured in this run"
    result["backward_grid_ab"] = grid if grid is not None else "not measured in this run"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)
    print(json.dumps({k: v for k, v in result.items() if k != "sizes"})[:3000])


if __name__ == "__main__":
    main()
