#!/usr/bin/env python
"""Writes tests/golden/color_correct_ref.npz: color_correct_quadratic and color_correct_affine as the REFERENCE's
gsplat/color_correct.py evaluates them on the CPU, for every case of tests/_color_correct_cases.py.
tests/test_color_correct.py and tests/test_gpu_color_correct.py read it and run without a reference checkout.
TEST INFRASTRUCTURE; needs a checkout of the reference (only that one file of it is loaded).

Keys. in/{input}/img, /ref: the float32 inputs (inputs up to SMALL pixels); in/{input}/sum: the float64 sums of img and of ref
(the large input, which is rebuilt from in/nat-37x53). q/{case}/out64: the reference's quadratic output evaluated in float64,
q/{case}/e32: max |its float32 output - out64|. a/{input}/out64, /e32: the same for the affine form. The large input keeps
every STRIDE-th element of each output.

The reference is used on float32 images, where torch rounds the Python scalars eps and 1 - eps to float32 before it compares.
Its float64 evaluation is given exactly those two thresholds (a float whose `1 - eps` returns float32(1 - eps)), so that out64
is the exact-arithmetic value of what the float32 evaluation computes; the "thresholds" input, with values placed exactly on
both, confirms that float32 includes them: its e32 stays at rounding level only if both evaluations select the same rows.

Every input must keep the guard band of _color_correct_cases (no value within GUARD of a threshold at any iteration unless
exactly on it, every scaled pivot above MIN_PIVOT); `--search` prints seeds for which it holds.

usage: GSPLAT_REFERENCE_PATH=<reference checkout> python tools/pin_color_correct_against_reference.py [--search]"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class Float32Eps(float):
    """eps as torch applies it to a float32 tensor: float32(eps), and `1 - eps` gives float32(1 - eps)."""

    def __new__(cls, eps):
        return super().__new__(cls, float(np.float32(eps)))

    def __init__(self, eps):
        self.one_minus = float(np.float32(1.0 - eps))

    def __rsub__(self, other):
        assert other == 1
        return self.one_minus


def load_reference():
    if not os.environ.get("GSPLAT_REFERENCE_PATH"):
        raise SystemExit("set GSPLAT_REFERENCE_PATH to a checkout of the reference (its gsplat/color_correct.py is loaded)")
    path = os.path.join(os.environ["GSPLAT_REFERENCE_PATH"], "gsplat", "color_correct.py")
    spec = importlib.util.spec_from_file_location("reference_color_correct", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    return ref


def guard_cases(cc, key):
    """(num_iters, eps) pairs under which input `key` has to keep its guard band."""
    return sorted({(c.num_iters, c.eps) for c in cc.cases() if c.input == key and c.num_iters})


def search(cc):
    table = cc.inputs_table()
    for key, inp in table.items():
        if inp.kind == "tiled":
            continue
        for seed in range(1, 400):
            img, ref = cc.build(inp._replace(seed=seed))
            if all(cc.holds(img, ref, it, eps) for it, eps in guard_cases(cc, key)):
                print(f'"{key}": {seed},', flush=True)
                break
        else:
            raise SystemExit(f"no seed below 400 keeps the guard band for {key}")


def main():
    import _color_correct_cases as cc
    from gsplat_amd import color_correct as ours

    if "--search" in sys.argv:
        return search(cc)
    ref = load_reference()
    table = cc.inputs_table()
    out, arrays = {}, {}
    for key, inp in table.items():
        img, rf = cc.build(inp, arrays.get("nat-37x53"))
        arrays[key] = (img, rf)
        n = img.size // 3
        sat = lambda a: float(((a <= 0) | (a >= 1)).mean())
        for it, eps in guard_cases(cc, key):
            gap, pivot = cc.guard_report(img, rf, it, eps)
            print(f"{key}: {n} pixels, saturated img {sat(img):.3f} ref {sat(rf):.3f}, iters {it} eps {eps:.5f}: closest {gap:.2e}, "
                  f"pivot {pivot:.2e}")
            assert gap > cc.GUARD and pivot > cc.MIN_PIVOT, (key, it, eps, gap, pivot)
        if n <= cc.SMALL:
            out[f"in/{key}/img"], out[f"in/{key}/ref"] = img, rf
        else:
            out[f"in/{key}/sum"] = np.array([img.astype(np.float64).sum(), rf.astype(np.float64).sum()])

    def keep(t, n):
        t = t.detach().numpy()
        return t if n <= cc.SMALL else np.ascontiguousarray(t.reshape(-1)[::cc.STRIDE])

    def pin(name, fn, ours_fn, img, rf):
        x32, r32 = torch.from_numpy(img), torch.from_numpy(rf)
        o64, o32 = fn(x32.double(), r32.double()), fn(x32, r32)
        assert o64.dtype == torch.float64 and o32.dtype == torch.float32 and o64.shape == x32.shape
        e32 = float((o32.double() - o64).abs().max())
        mine64, mine32 = ours_fn(x32.double(), r32.double()), ours_fn(x32, r32)
        e_mine64, e_mine32 = float((mine64 - o64).abs().max()), float((mine32.double() - o64).abs().max())
        print(f"{name}: e32 {e32:.3e}; our torch composition: float64 {e_mine64:.1e}, float32 {e_mine32:.3e}")
        assert e_mine64 <= 1e-12, name
        n = img.size // 3
        out[f"{name}/out64"], out[f"{name}/e32"] = keep(o64, n), np.float64(e32)

    for case in cc.cases():
        img, rf = arrays[case.input]
        eps = Float32Eps(case.eps)
        pin(f"q/{case.name}", lambda a, b: ref.color_correct_quadratic(a, b, num_iters=case.num_iters, eps=eps),
            lambda a, b: ours.color_correct_quadratic_torch(a, b, case.num_iters, case.eps), img, rf)
    for key in table:
        pin(f"a/{key}", ref.color_correct_affine, ours.color_correct_affine_torch, *arrays[key])

    np.savez_compressed(cc.FIXTURE, **out)
    size = os.path.getsize(cc.FIXTURE)
    assert size < (1 << 20), size
    print("COLOUR CORRECTION PINNED ->", cc.FIXTURE, size, "bytes,", len(cc.cases()), "quadratic and", len(table), "affine cases")


if __name__ == "__main__":
    main()
