#!/usr/bin/env python
"""Writes tests/golden/knn_init_ref.npz: the nearest-neighbour scale initialisation as the REFERENCE evaluates it on the CPU,
for tests/test_knn_init.py and tests/test_gpu_knn_init.py, which run without a reference checkout. TEST INFRASTRUCTURE; needs a
checkout of the reference (gsplat/init_utils.py, loaded as a file: the package itself is not imported) and scikit-learn, which
is what the trainer's `knn` (examples/utils.py:156) calls.

Per case of tests/_knn_cases.py PINNED (N <= 4099):
  {name}_x             the float32 input
  {name}_scale32/64    the reference's knn_scale_init(x, 3), evaluated in float32 and in float64 (from the same float32 input)
  {name}_sk_dist       NearestNeighbors(n_neighbors=min(4, N)).fit(x).kneighbors(x) distances, float64
  {name}_spread_scale  max |scale32 - scale64|: the reference's own float32 spread (its cdist takes the |a|^2 + |b|^2 - 2 a.b form)
  {name}_err_scale     max |direct float32 brute force - scale64| in log-scale  } the tolerance of the tests is 4 x these + 1 ulp;
  {name}_err_dist      max relative difference of its distances to _sk_dist     } the brute force is written HERE, coordinate
                                                                                  differences in torch, not the code under test
Checks gsplat_amd's torch composition against the same rule on the way.

usage: GSPLAT_REFERENCE_PATH=<reference checkout> python tools/pin_knn_against_reference.py"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if not os.environ.get("GSPLAT_REFERENCE_PATH"):
    raise SystemExit("set GSPLAT_REFERENCE_PATH to a checkout of the reference (gsplat/init_utils.py)")


def load_reference():
    path = os.path.join(os.environ["GSPLAT_REFERENCE_PATH"], "gsplat", "init_utils.py")
    spec = importlib.util.spec_from_file_location("reference_init_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def direct_float32(x, K):
    """All-pairs float32 distances from coordinate differences, K smallest per row."""
    d = x[:, None, :] - x[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return torch.topk(d2, K, dim=-1, largest=False, sorted=True).values.sqrt()


def main():
    from sklearn.neighbors import NearestNeighbors

    import _knn_cases as kc
    from gsplat_amd import init_utils as ours

    ref = load_reference()
    out = {}
    for name, gen in kc.PINNED.items():
        x = gen()
        assert x.dtype == torch.float32 and x.shape[0] <= 4099
        N = x.shape[0]
        K = min(4, N)
        s32 = ref.knn_scale_init(x, 3)
        s64 = ref.knn_scale_init(x.double(), 3)
        x64 = x.double().numpy()
        sk = NearestNeighbors(n_neighbors=K).fit(x64).kneighbors(x64)[0]
        d32 = direct_float32(x, K)
        mine = kc.scale_of(d32[:, 1:]).double()
        err_scale = float((mine - s64).abs().max())
        skt = torch.from_numpy(sk)
        nz = skt > 0
        assert bool((d32.double()[~nz] == 0).all()), name
        err_dist = float(((d32.double() - skt).abs()[nz] / skt[nz]).max()) if bool(nz.any()) else 0.0
        spread = float((s32.double() - s64).abs().max())
        # scikit-learn's float64 distances and the reference's float64 log-scale state the same thing
        agree = float((kc.scale_of(skt[:, 1:]) - s64).abs().max())
        assert agree <= 1e-9, (name, agree)
        out.update({f"{name}_x": x.numpy(), f"{name}_scale32": s32.numpy(), f"{name}_scale64": s64.numpy(),
                    f"{name}_sk_dist": sk, f"{name}_spread_scale": np.float64(spread), f"{name}_err_scale": np.float64(err_scale),
                    f"{name}_err_dist": np.float64(err_dist)})
        print(f"{name}: N {N}  err_scale {err_scale:.3e}  err_dist {err_dist:.3e}  reference's float32 spread {spread:.3e}")
    path = os.path.join(ROOT, "tests", "golden", "knn_init_ref.npz")
    np.savez_compressed(path, **out)
    kc.golden.cache_clear()
    for name in kc.PINNED:  # our torch composition under the rule the tests apply
        x = kc.points(name)
        kc.check_scale(name, ours.knn_scale_init_torch(x, 3), "torch")
        kc.check_dist(name, ours.knn_torch(x, min(4, x.shape[0])), "torch")
    size = os.path.getsize(path)
    assert size < 1_000_000, size
    print("KNN PINNED ->", path, size, "bytes")


if __name__ == "__main__":
    main()
