"""Point clouds for the nearest-neighbour initialisation (gsplat_amd/init_utils.py), shared by
tools/pin_knn_against_reference.py, tests/test_knn_init.py and tests/test_gpu_knn_init.py, and the comparison rule against
tests/golden/knn_init_ref.npz. Every generator is seeded and runs on the CPU; N is the smallest size that reaches its path."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_init_ref.npz")
ULP = 2.0 ** -23  # one float32 ulp, relative
EPS = 1e-7  # knn_scale_init's default clamp


def four():
    return torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.5, 0.5, 3.0]])


def identical():
    return torch.tensor([[0.25, -1.5, 3.0]]).repeat(257, 1)


def collinear():
    g = torch.Generator().manual_seed(11)
    t = torch.rand(300, 1, generator=g) * 10.0 - 5.0
    return (torch.tensor([[1.0, 0.0, 0.0]]) * t + torch.tensor([[0.0, 2.0, -1.0]])).contiguous()  # along x: y and z constant


def coplanar():
    g = torch.Generator().manual_seed(12)
    uv = torch.rand(1000, 2, generator=g) * 4.0
    return torch.stack([uv[:, 0], torch.full((1000,), 0.5), uv[:, 1]], dim=-1).contiguous()  # y constant


def lattice():
    r = torch.arange(16, dtype=torch.float32)
    return torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()


def clustered(N=4099, seed=3):
    """Half a blob of sigma 0.05, a quarter a blob of sigma 1, a quarter (the rest) uniform in a 20-unit box, 8 outliers at
    sigma 500 and 8 exact duplicates of earlier points; shuffled."""
    g = torch.Generator().manual_seed(seed)
    n_a, n_b = N // 2, N // 4
    n_c = N - n_a - n_b - 16
    a = torch.randn(n_a, 3, generator=g) * 0.05 + torch.tensor([1.0, -2.0, 0.5])
    b = torch.randn(n_b, 3, generator=g) * 1.0 + torch.tensor([-4.0, 3.0, 2.0])
    c = torch.rand(n_c, 3, generator=g) * 20.0 - 10.0
    out = torch.randn(8, 3, generator=g) * 500.0
    body = torch.cat([a, b, c, out])
    dup = body[torch.randint(0, body.shape[0], (8,), generator=g)]
    x = torch.cat([body, dup])
    return x[torch.randperm(N, generator=g)].contiguous()


def uniform(N=20_000, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, 3, generator=g).contiguous()


PINNED = {"four": four, "identical": identical, "collinear": collinear, "coplanar": coplanar, "lattice": lattice,
          "clustered": clustered}


def brute_force(x, K, dtype=torch.float64, chunk=1024):
    """K smallest distances per row (ascending) and their indices, from coordinate differences in `dtype` on x's device: the
    yardstick where no fixture exists. Not the code under test."""
    x = x.to(dtype)
    ds, ids = [], []
    for s in range(0, x.shape[0], chunk):
        d = x[s:s + chunk, None, :] - x[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        v, i = torch.topk(d2, K, dim=-1, largest=False, sorted=True)
        ds.append(v.sqrt())
        ids.append(i)
    return torch.cat(ds), torch.cat(ids)


def scale_of(dist, eps=EPS):
    """knn_scale_init's value from the distances to the k nearest OTHER points."""
    return dist.pow(2).mean(dim=-1).sqrt().clamp_min(eps).log()


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def points(name):
    return torch.from_numpy(golden()[name + "_x"].copy())


def check_scale(name, got, who):
    """|got - float64 reference| <= 4 x (direct float32 brute force's own distance from float64) + one float32 ulp of the largest
    magnitude; and within the reference's own float32-float64 spread (+ the same ulp): drop-in parity."""
    z = golden()
    ref = torch.from_numpy(z[name + "_scale64"])
    err, spread = float(z[name + "_err_scale"]), float(z[name + "_spread_scale"])
    # one float32 ulp of a log-scale: of its own magnitude, and never below the ulp of the distance it is the log of (a relative
    # step of 2^-23 in a distance is an absolute step of 2^-23 in its log)
    ulp = ULP * max(1.0, float(ref.abs().max()))
    d = float((got.detach().cpu().double() - ref).abs().max())
    print(f"{who} {name} log-scale: diff {d:.3e} tol {4 * err + ulp:.3e} (err {err:.3e}); reference's own spread {spread:.3e}")
    assert d <= 4 * err + ulp, (name, d, 4 * err + ulp)
    assert d <= spread + ulp, (name, d, spread)


def check_dist(name, got, who):
    """Relative difference of the K = 4 distances against scikit-learn's float64 kneighbors <= 4 x the direct float32 brute
    force's + one ulp; a zero distance must be exactly zero."""
    z = golden()
    ref = torch.from_numpy(z[name + "_sk_dist"])
    err = float(z[name + "_err_dist"])
    got = got.detach().cpu().double()
    assert got.shape == ref.shape
    zero = ref == 0
    assert bool((got[zero] == 0).all()), name
    rel = float(((got - ref).abs()[~zero] / ref[~zero]).max()) if bool((~zero).any()) else 0.0
    print(f"{who} {name} distances: rel diff {rel:.3e} tol {4 * err + ULP:.3e} (err {err:.3e})")
    assert rel <= 4 * err + ULP, (name, rel, 4 * err + ULP)
