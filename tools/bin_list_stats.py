#!/usr/bin/env python
"""CPU only: the tile lists of the benchmark's scene as the binned intersection's sort kernel sees them (csrc/isect_binned.hip,
bin_sort_kernel): list lengths, how many lie just over 512, and how many of the 4 x 2-tile bins need a second batch under the
arena rules that were considered - the table of profiles/r13_split_lists.md.

Projection, isect_tiles and isect_offset_encode are the oracle's, on bench.make_workload. The rules restate the kernel's greedy
cut: a bin's eight lists in tile order (x fastest), a new batch whenever the next region does not fit what is left.

    python tools/bin_list_stats.py [--scene 1000000:0 --scene 1000000:1 --scene 900000:0 --scene 1100000:0]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from oracle import oracle as O  # noqa: E402

BW, BH = 4, 2


def pow2(n, floor=64):
    p = floor
    while p < n:
        p <<= 1
    return p


def words_pow2(n):
    """Every list padded to a power of two >= 64 (the kernel before the split)."""
    return pow2(n) if n > 0 else 0


def words_split(n, tail_round):
    """H < n <= H + H / 4 with H >= 256: H + the tail rounded by `tail_round`; else the power of two."""
    if n <= 0:
        return 0
    P = pow2(n)
    H = P >> 1
    if H >= 256 and n - H <= H // 4:
        return H + tail_round(n - H)
    return P


RULES = {  # name: (words of a list, arena words)
    "pow2 @4096 (before)": (words_pow2, 4096),
    "split, tail -> pow2 >= 64 @4096": (lambda n: words_split(n, pow2), 4096),
    "split, tail -> pow2 >= 64 @4352": (lambda n: words_split(n, pow2), 4352),
    "split, tail -> 64 @4352": (lambda n: words_split(n, lambda t: (t + 63) & ~63), 4352),
    "split, tail -> 8 @4352 (the kernel)": (lambda n: words_split(n, lambda t: (t + 7) & ~7), 4352),
}


def batches(lengths, words, arena):
    """Batches of one bin under the greedy cut (lists longer than the arena go to the work-list sort and take none)."""
    batch, used = 1, 0
    for n in lengths:
        w = words(int(n))
        if w == 0 or w > arena:
            continue
        if used + w > arena:
            batch, used = batch + 1, 0
        used += w
    return batch


def scene_lists(n_gaussians, seed):
    sc, W, H = bench.make_workload(n_gaussians, "cpu", seed=seed)
    with torch.no_grad():
        radii, means2d, depths, conics, _ = (t[0] if t is not None else None for t in O.fully_fused_projection(
            sc["means"][None], None, sc["quats"][None], sc["scales"][None], sc["viewmats"][None], sc["Ks"][None], W, H,
            opacities=sc["opacities"][None]))
    tw, th = (W + bench.TILE - 1) // bench.TILE, (H + bench.TILE - 1) // bench.TILE
    _, ids, _ = O.isect_tiles(means2d, radii, depths, bench.TILE, tw, th, conics=conics, opacities=sc["opacities"][None])
    off = O.isect_offset_encode(ids, 1, tw, th).numpy().reshape(-1)
    return np.diff(np.concatenate([off, [ids.numel()]])).reshape(th, tw), tw, th


def stats(n_gaussians, seed):
    lens, tw, th = scene_lists(n_gaussians, seed)
    flat = lens.reshape(-1)
    bins = []
    for by in range((th + BH - 1) // BH):
        for bx in range((tw + BW - 1) // BW):
            bins.append(lens[by * BH:(by + 1) * BH, bx * BW:(bx + 1) * BW].reshape(-1))
    row = {"gaussians": n_gaussians, "seed": seed, "lists": int(flat.size), "bins": len(bins),
           "mean": round(float(flat.mean()), 1), "std": round(float(flat.std()), 1), "min": int(flat.min()), "max": int(flat.max()),
           "lists_513_1024": int(((flat > 512) & (flat <= 1024)).sum()), "lists_513_640": int(((flat > 512) & (flat <= 640)).sum()),
           "longest_tail_over_512": int(max(0, flat[flat <= 1024].max() - 512)), "rules": {}}
    for name, (words, arena) in RULES.items():
        need = [int(sum(words(int(n)) for n in b)) for b in bins]
        row["rules"][name] = {"bins_with_2nd_batch": sum(batches(b, words, arena) > 1 for b in bins), "max_bin_words": max(need)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", action="append", default=None, metavar="GAUSSIANS:SEED")
    args = ap.parse_args()
    O.set_threads(min(os.cpu_count() or 1, 32))
    scenes = args.scene or ["1000000:0", "1000000:1", "900000:0", "1100000:0"]
    for s in scenes:
        n, seed = (int(v) for v in s.split(":"))
        print(json.dumps(stats(n, seed)), flush=True)


if __name__ == "__main__":
    main()
