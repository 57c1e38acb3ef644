"""CPU: the torch path of gsplat_amd/init_utils.py (knn, knn_scale_init on CPU tensors) against tests/golden/knn_init_ref.npz -
the reference's knn_scale_init in float64 and scikit-learn's kneighbors (tools/pin_knn_against_reference.py) - and the error
cases. Tolerance: 4 x the stored distance of a direct float32 brute force from float64, plus one float32 ulp."""
import pytest
import torch

import gsplat_amd
import _knn_cases as kc
from gsplat_amd import init_utils as iu


@pytest.mark.parametrize("name", list(kc.PINNED))
def test_generators_reproduce_the_pinned_inputs(name):
    assert torch.equal(kc.PINNED[name](), kc.points(name))


@pytest.mark.parametrize("name", list(kc.PINNED))
def test_torch_path_matches_reference(name):
    x = kc.points(name)
    K = min(4, x.shape[0])
    dist, idx = gsplat_amd.knn(x, K, return_indices=True)
    assert dist.shape == (x.shape[0], K) and idx.shape == dist.shape and idx.dtype == torch.int64
    assert bool((dist[:, 0] == 0).all()) and bool((dist[:, 1:] >= dist[:, :-1]).all())
    kc.check_dist(name, dist, "torch")
    kc.check_scale(name, gsplat_amd.knn_scale_init(x, 3), "torch")
    kc.check_scale(name, iu.knn_scale_init_torch(x, 3, chunk_size=100), "torch chunk 100")


def test_lattice_and_identical_points_are_exact():
    x = kc.points("lattice")
    assert bool((gsplat_amd.knn_scale_init(x, 3) == 0).all())
    assert torch.equal(gsplat_amd.knn(x, 4), torch.tensor([0.0, 1.0, 1.0, 1.0]).expand(4096, 4))
    x = kc.points("identical")
    assert bool((gsplat_amd.knn(x, 4) == 0).all())
    assert torch.equal(gsplat_amd.knn_scale_init(x, 3), torch.tensor(kc.EPS).log().expand(257))


def test_float64_and_large_k_take_the_torch_path():
    x = kc.points("coplanar")
    d64, ref = gsplat_amd.knn(x.double(), 17), kc.brute_force(x, 17)[0]
    assert d64.dtype == torch.float64 and float((d64 - ref).abs().max()) <= 1e-12
    s = gsplat_amd.knn_scale_init(x, k=16)  # K = 17 > 16
    assert float((s.double() - kc.scale_of(ref[:, 1:])).abs().max()) <= 1e-5


def test_indices_name_the_reported_neighbours():
    x = kc.points("clustered")
    dist, idx = gsplat_amd.knn(x, 4, return_indices=True)
    assert bool(((idx >= 0) & (idx < x.shape[0])).all())
    assert all(len(set(r)) == 4 for r in idx.tolist())
    again = (x.double()[idx] - x.double()[:, None, :]).norm(dim=-1)
    assert float((again - dist.double()).abs().max()) <= 4 * kc.ULP * float(dist.max())


def test_non_finite_points_are_left_out():
    x = kc.points("clustered")
    y = torch.cat([x, torch.tensor([[float("nan"), 0.0, 0.0], [1.0, float("-inf"), 2.0]])])
    a, (b, ib) = gsplat_amd.knn(x, 4), gsplat_amd.knn(y, 4, return_indices=True)
    assert torch.equal(a, b[:-2]) and bool(b[-2:].isnan().all()) and bool((ib[-2:] == -1).all())
    assert bool((ib[:-2] < x.shape[0]).all())
    s = gsplat_amd.knn_scale_init(y, 3)
    assert torch.equal(s[:-2], gsplat_amd.knn_scale_init(x, 3)) and bool(s[-2:].isnan().all())


def test_gradient_flows_through_the_torch_path():
    x = kc.points("coplanar")[:200].clone().requires_grad_(True)
    gsplat_amd.knn_scale_init(x, 3).sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0


def test_error_cases():
    x = kc.four()
    assert gsplat_amd.knn(x, 4).shape == (4, 4) and gsplat_amd.knn_scale_init(x, 3).shape == (4,)
    with pytest.raises(ValueError):
        gsplat_amd.knn(x, 5)
    with pytest.raises(ValueError, match=r"need at least k\+1=5 points, got 4"):
        gsplat_amd.knn_scale_init(x, 4)
    with pytest.raises(ValueError):
        gsplat_amd.knn(x, 0)
    with pytest.raises(ValueError):
        gsplat_amd.knn(torch.zeros(5, 2), 2)


def test_public_names():
    assert gsplat_amd.init_utils is iu and gsplat_amd.knn is iu.knn and gsplat_amd.knn_scale_init is iu.knn_scale_init
    assert {"init_utils", "knn", "knn_scale_init"} <= set(dir(gsplat_amd))
