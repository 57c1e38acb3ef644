#!/usr/bin/env python
"""Times the L1 K-means kernels of PngCompression's SH codebook (csrc/kmeans.hip through gsplat_amd.compression) against the
torch composition they replace (kmeans_l1_torch: chunked torch.cdist(p=1).argmin + index_add_) and writes profiles/kmeans.json.

Per D (45 = the SH bands of degree 3, 24 = degree 2) at N rows and K centroids: standard-normal rows scaled by 0.1, generated on
the device from a seed; the centroids are K distinct rows, as kmeans_l1 draws them. Alternating windows, each the median of
`--iters` calls between device events after a warm-up call, of
  assign        one fused assignment pass (gsx_kmeans_assign_l1) over all N rows
  torch_assign  the torch composition's assignment over the first `--torch-rows` rows in kmeans_l1_torch's own chunks
                (max_chunk_elems // (K D) rows per cdist call), scaled by N / torch_rows: an extrapolation, stated as such -
                the full torch pass is not run
  update        key building + torch.sort + gsx_kmeans_update on the labels of the assignment, and on all-zero labels (all rows
                in one cluster: the longest chain of additions the update can meet)
and, once warm, `--whole` runs of the whole kmeans_l1 (10 iterations + the final labelling) on a host clock around a
synchronise. Recorded besides: the ratio of the assignment pass to the arithmetic floor of 0.15 s the kernel was planned against
(N K D terms, a subtract and an add each, 16 lanes per clock per SIMD, 1024 SIMDs, 2.4 GHz; scaled with D), whether the fused
labels of the first `--check-rows` rows equal the sequential float32 composition bit for bit, how many of the torch subset's
labels agree (cdist adds in another order), and, with --kernel-resources FILE (written by tools/kmeans_resources.py from the
compiler's resource remarks where hipcc is), the kernels' VGPRs, LDS and occupancy.

usage: python tools/kmeans_bench.py [--iters 3] [--windows 3] [--out profiles/kmeans.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gsplat_amd.compression import png_compression as C  # noqa: E402

DEV = "cuda"
FLOOR_S_AT_1M_64K_45 = 0.15


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


def sequential_f32(x, c):
    """The definition of the fused result: one float32 accumulator per pair, ascending d, then the lowest minimal index."""
    acc = torch.zeros((x.shape[0], c.shape[0]), dtype=torch.float32, device=x.device)
    for d in range(x.shape[1]):
        acc = acc + (x[:, d, None] - c[None, :, d]).abs()
    best = acc.min(dim=1).values
    cols = torch.arange(c.shape[0], device=x.device).expand_as(acc)
    return torch.where(acc == best[:, None], cols, torch.full_like(cols, c.shape[0])).min(dim=1).values, best


def torch_assign(x, centroids, max_chunk_elems=1 << 27):
    """The assignment loop of kmeans_l1_torch with the chunk the FULL problem would get."""
    k, d = centroids.shape
    chunk = max(1, max_chunk_elems // max(1, k * d))
    labels = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for lo in range(0, x.shape[0], chunk):
        labels[lo:lo + chunk] = torch.cdist(x[lo:lo + chunk], centroids, p=1).argmin(dim=1)
    return labels


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=3)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--clusters", type=int, default=65536)
    p.add_argument("--dims", type=int, nargs="*", default=[45, 24])
    p.add_argument("--torch-rows", type=int, default=4096)
    p.add_argument("--check-rows", type=int, default=256)
    p.add_argument("--whole", type=int, default=2)
    p.add_argument("--kernel-resources", default=None)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans.json"))
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_bench: needs a ROCm GPU; nothing is measured without one")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    N, K = args.rows, args.clusters
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "N": N, "K": K, "torch_rows": args.torch_rows,
              "note": "torch_assign_ms_extrapolated = the torch composition's assignment timed on torch_rows rows x N / torch_rows: "
                      "an extrapolation, not a measurement of the full pass", "dims": []}
    if args.kernel_resources:
        with open(args.kernel_resources) as f:
            result["kernels"] = json.load(f)
    for D in args.dims:
        g = torch.Generator(device=DEV).manual_seed(1000 + D)
        x = torch.randn(N, D, generator=g, device=DEV) * 0.1
        cents = x[torch.randperm(N, generator=torch.Generator().manual_seed(0))[:K].to(DEV)].clone()
        assert C._kmeans_fused_ok(x)
        sub = x[:args.torch_rows].contiguous()
        entry = {"D": D, "assign_ms": [], "torch_assign_subset_ms": [], "torch_assign_ms_extrapolated": [], "update_ms": [],
                 "update_all_rows_in_one_cluster_ms": [], "kmeans_l1_10_iterations_s": []}
        with torch.no_grad():
            labels = C._assign_fused(x, cents, False)[0]
            one = torch.zeros_like(labels)
            for _ in range(args.windows):
                entry["assign_ms"].append(timed(lambda: C._assign_fused(x, cents, False), args.iters))
                t = timed(lambda: torch_assign(sub, cents), args.iters)
                entry["torch_assign_subset_ms"].append(t)
                entry["torch_assign_ms_extrapolated"].append(t * N / args.torch_rows)
                entry["update_ms"].append(timed(lambda: C._update_fused(x, labels, cents), args.iters))
                entry["update_all_rows_in_one_cluster_ms"].append(timed(lambda: C._update_fused(x, one, cents), args.iters))
            entry["ratio_torch_over_fused"] = [t / u for t, u in zip(entry["torch_assign_ms_extrapolated"], entry["assign_ms"])]
            entry["fused_wins_every_window"] = all(r > 1.0 for r in entry["ratio_torch_over_fused"])
            floor_ms = FLOOR_S_AT_1M_64K_45 * 1e3 * (N / 1e6) * (K / 65536) * (D / 45)
            entry["arithmetic_floor_ms"] = floor_ms
            entry["assign_over_floor"] = [t / floor_ms for t in entry["assign_ms"]]
            # results at the timed size
            seq_labels, seq_best = sequential_f32(x[:args.check_rows], cents)
            fl, fb = C._assign_fused(x[:args.check_rows].contiguous(), cents, True)
            entry["bit_equal_to_sequential_composition"] = bool(torch.equal(fl.long(), seq_labels) and torch.equal(fb, seq_best))
            entry["labels_agreeing_with_torch_cdist"] = float((torch_assign(sub, cents) == labels[:args.torch_rows]).float().mean())
            for _ in range(args.whole):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = C.kmeans_l1(x, K)
                torch.cuda.synchronize()
                entry["kmeans_l1_10_iterations_s"].append(time.perf_counter() - t0)
                del out
        result["dims"].append(entry)
        print(json.dumps(entry), flush=True)
        with open(args.out, "w") as fh:  # after every D: a run that is cut short leaves what it measured
            json.dump(result, fh, indent=1)
        del x, cents, sub, labels, one
        torch.cuda.empty_cache()
    print("wrote", args.out)
    lost = [e["D"] for e in result["dims"] if not e["fused_wins_every_window"]]
    if lost:
        raise SystemExit(f"the fused assignment lost a window to the torch composition at D = {lost}")
    if not all(e["bit_equal_to_sequential_composition"] for e in result["dims"]):
        raise SystemExit("the fused assignment differs from the sequential float32 composition")


if __name__ == "__main__":
    main()
