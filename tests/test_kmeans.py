"""CPU: the dispatch and the definition behind the L1 K-means of PngCompression (gsplat_amd/compression/png_compression.py,
csrc/kmeans.hip). Off the GPU nothing changes (kmeans_l1 is kmeans_l1_torch); the fused predicate is what it says; the
sequential float32 composition that defines the kernels' result stays inside the float64 tolerance the GPU file applies; and the
torch form of kmeans_assign_l1 is that composition."""
import pytest
import torch

import _kmeans_cases as kc
import gsplat_amd.compression as compression
from gsplat_amd.compression import png_compression as C


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_kmeans_l1_is_the_torch_composition(dtype):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(700, 11, generator=g).to(dtype)
    for k, iters in ((16, 10), (900, 3)):  # K < N and K clipped to N
        a, b = C.kmeans_l1(x, k, n_iters=iters, seed=2), C.kmeans_l1_torch(x, k, n_iters=iters, seed=2)
        assert a[0].dtype == dtype and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert compression.kmeans_l1 is C.kmeans_l1 and compression.kmeans_assign_l1 is C.kmeans_assign_l1
    assert {"PngCompression", "kmeans_l1", "kmeans_assign_l1"} <= set(compression.__all__)


def test_fused_predicate():
    assert not C._kmeans_fused_ok(torch.zeros(10, 45))
    assert not C._kmeans_fused_ok(torch.zeros(10, 45, dtype=torch.float64))
    assert not C._kmeans_fused_ok(torch.zeros(10, 129))
    assert not C._kmeans_fused_ok(torch.zeros(10, 45, device="meta"))
    ok = C._kmeans_fused_config_ok
    assert ok("cuda", torch.float32, (10, 45)) and ok("cuda", torch.float32, (0, 1)) and ok("cuda", torch.float32, (10, 128))
    for dev in ("cpu", "meta", "xla"):
        assert not ok(dev, torch.float32, (10, 45))
    for dt in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
        assert not ok("cuda", dt, (10, 45))
    for shape in ((10, 129), (10, 0), (10,), (10, 3, 15), (2 ** 31 - 1, 4)):
        assert not ok("cuda", torch.float32, shape)


@pytest.mark.parametrize("d", kc.DS)
def test_the_definition_stays_inside_the_float64_tolerance(d):
    """For every shape of the GPU file: the centroid the sequential float32 composition picks is, in float64, within
    2 (D + 1) 2^-24 dist of the float64 minimum (kc.tolerance)."""
    worst = 0.0
    for n, k, dd in kc.ASSIGN_CASES:
        if dd != d:
            continue
        x, c = kc.assign_case(n, k, d)
        labels, best = kc.sequential_f32(x, c)
        assert bool(((labels >= 0) & (labels < k)).all())
        excess, chosen = kc.excess_over_f64_minimum(x, c, labels)
        tol = kc.tolerance(d, chosen)
        assert bool((excess <= tol).all()), (n, k, d, float((excess - tol).max()))
        assert bool(((best.double() - chosen).abs() <= 0.5 * tol).all())  # the float32 value itself: (D + 1) u dist
        worst = max(worst, float((excess / tol.clamp_min(1e-300)).max()))
    print(f"D = {d}: largest excess over the float64 minimum = {worst:.3f} of the tolerance")


def test_assign_on_cpu_is_the_float64_argmin_with_wide_margins():
    g = torch.Generator().manual_seed(11)
    c = torch.randn(37, 45, generator=g) * 10
    truth = torch.randint(0, 37, (500,), generator=g)
    x = c[truth] + 0.01 * torch.randn(500, 45, generator=g)
    labels, best = C.kmeans_assign_l1(x, c, return_distance=True)
    d64 = kc.distances_f64(x, c)
    assert labels.dtype == torch.int64 and best.dtype == torch.float32
    assert torch.equal(labels, d64.argmin(dim=1)) and torch.equal(labels, truth)
    assert torch.equal(C.kmeans_assign_l1(x, c), labels)
    seq_labels, seq_best = kc.sequential_f32(x, c)
    assert torch.equal(labels, seq_labels) and torch.equal(best, seq_best)
    # float64 rows take the same path in their own precision
    l64, b64 = C.kmeans_assign_l1(x.double(), c.double(), return_distance=True)
    assert torch.equal(l64, labels) and b64.dtype == torch.float64 and float((b64 - d64.min(dim=1).values).abs().max()) < 1e-12
    # ties go to the lowest index; a row with a non-finite coordinate gets a label in range
    cc = torch.cat([c, c])
    assert torch.equal(C.kmeans_assign_l1(x, cc), labels)
    y = x.clone()
    y[3, 7], y[9, 0] = float("nan"), float("inf")
    ly = C.kmeans_assign_l1(y, c)
    keep = torch.ones(500, dtype=torch.bool)
    keep[[3, 9]] = False
    assert bool(((ly >= 0) & (ly < 37)).all()) and torch.equal(ly[keep], labels[keep])
    with pytest.raises(ValueError):
        C.kmeans_assign_l1(x, c[:, :44])
