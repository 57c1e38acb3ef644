"""GPU: the nearest-neighbour kernels (csrc/knn.hip) behind gsplat_amd.knn / knn_scale_init, against
tests/golden/knn_init_ref.npz (the reference's float64 knn_scale_init and scikit-learn's kneighbors) and, where no fixture
exists, a float64 brute force. Tolerance (tests/_knn_cases.py): 4 x the stored distance of a direct float32 brute force from
float64 plus one float32 ulp, and within the reference's own float32-float64 spread. The search is exact, so everything that
does not involve float64 is compared bit for bit."""
import functools

import pytest
import torch

import gsplat_amd
import _knn_cases as kc
from gsplat_amd import init_utils as iu

pytestmark = pytest.mark.gpu
DEV = "cuda"


def fused(x, K, return_indices=False, ring_cap=iu.RING_CAP):
    assert iu._fused_ok(x, K), "the fused kernels were not taken"
    return iu._knn_fused(x, K, return_indices, ring_cap)


def check_rows(x, dist, idx):
    """Ascending, column 0 zero, indices distinct and in range, and the float64 distance to x[idx] is the one returned (ties
    are not compared index for index)."""
    N, K = dist.shape
    assert bool((dist[:, 0] == 0).all()) and bool((dist[:, 1:] >= dist[:, :-1]).all())
    assert idx.dtype == torch.int64 and bool(((idx >= 0) & (idx < N)).all())
    s = idx.sort(dim=-1).values
    assert bool((s[:, 1:] != s[:, :-1]).all()), "an index twice in a row"
    xd = x.double()
    again = (xd[idx] - xd[:, None, :]).norm(dim=-1)
    rel = float(((again - dist.double()).abs() / again.clamp_min(1e-300)).max())
    print(f"distance to x[idx] against the returned one: rel {rel:.3e}")
    assert rel <= 4 * kc.ULP  # (dx dx + dy dy) + dz dz and a square root in float32: under three roundings


@pytest.mark.parametrize("name", list(kc.PINNED))
def test_fused_matches_reference(name):
    x = kc.points(name).to(DEV)
    K = min(4, x.shape[0])
    dist, idx = fused(x, K, True)
    check_rows(x, dist, idx)
    kc.check_dist(name, dist, "fused")
    s = gsplat_amd.knn_scale_init(x, 3)
    kc.check_scale(name, s, "fused")
    # knn_scale_init is the same backend's knn: to 1 ulp (the same tensor operations on the same distances)
    mine = kc.scale_of(gsplat_amd.knn(x, 4)[:, 1:])
    assert float((s - mine).abs().max()) <= kc.ULP * max(1.0, float(mine.abs().max()))


def test_lattice_and_identical_points_are_exact():
    x = kc.points("lattice").to(DEV)
    assert bool((gsplat_amd.knn_scale_init(x, 3) == 0).all())
    assert torch.equal(fused(x, 4), torch.tensor([0.0, 1.0, 1.0, 1.0], device=DEV).expand(4096, 4))
    x = kc.points("identical").to(DEV)
    assert bool((fused(x, 4) == 0).all())
    assert iu.knn_last_stats()["dims"] == [1, 1, 1]
    assert torch.equal(gsplat_amd.knn_scale_init(x, 3), torch.tensor(kc.EPS, device=DEV).log().expand(257))


def test_degenerate_boxes_get_one_cell_along_the_flat_axes():
    fused(kc.points("collinear").to(DEV), 4)
    assert iu.knn_last_stats()["dims"][1:] == [1, 1] and iu.knn_last_stats()["dims"][0] > 1
    fused(kc.points("coplanar").to(DEV), 4)
    d = iu.knn_last_stats()["dims"]
    assert d[1] == 1 and d[0] > 1 and d[2] > 1


def test_error_cases_on_the_device():
    x = kc.four().to(DEV)
    assert torch.equal(fused(x, 4)[:, 0], torch.zeros(4, device=DEV))
    with pytest.raises(ValueError):
        gsplat_amd.knn(x, 5)
    with pytest.raises(ValueError):
        gsplat_amd.knn_scale_init(x, 4)


def test_every_path_gives_the_same_bits_on_the_clustered_cloud():
    """ring_cap 0 sends every query whose own cell does not settle it to the all-points scan, the default walks rings: the
    outputs are the same bits, and so are those of a second call. The tight blob, half the cloud, falls into a cell or two."""
    x = kc.points("clustered").to(DEV)
    a, ia = fused(x, 4, True)
    st = iu.knn_last_stats()
    b, ib = fused(x, 4, True)
    assert torch.equal(a, b) and torch.equal(ia, ib), "two calls differ"
    c, ic = fused(x, 4, True, ring_cap=0)
    n_def = iu.knn_last_stats()["deferred"]
    print(f"grid {st['dims']}, deferred at the default ring cap {st['deferred']}, at ring cap 0 {n_def}")
    assert n_def > 0, "the all-points scan was not reached"
    assert torch.equal(a, c)
    check_rows(x, c, ic)
    d = fused(x, 4, False, ring_cap=1)
    assert torch.equal(a, d) and iu.knn_last_stats()["deferred"] > 0


def test_permuting_the_rows_permutes_the_output():
    x = kc.points("clustered").to(DEV)
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(9)).to(DEV)
    for K in (4, 7):
        assert torch.equal(fused(x, K)[perm], fused(x[perm].contiguous(), K))
    assert torch.equal(gsplat_amd.knn_scale_init(x, 3)[perm], gsplat_amd.knn_scale_init(x[perm].contiguous(), 3))


def test_non_finite_points_are_left_out():
    x = kc.points("clustered")
    y = torch.cat([x[:100], torch.tensor([[float("nan"), 0.0, 0.0]]), x[100:], torch.tensor([[1.0, float("-inf"), 2.0]]),
                   torch.tensor([[float("inf"), 0.0, 0.0]])]).to(DEV)
    keep = torch.tensor([i for i in range(y.shape[0]) if i not in (100, y.shape[0] - 2, y.shape[0] - 1)], device=DEV)
    a = fused(x.to(DEV), 4)
    b, ib = fused(y, 4, True)
    assert torch.equal(a, b[keep]), "a finite row changed"
    for r in (100, y.shape[0] - 2, y.shape[0] - 1):
        assert bool(b[r].isnan().all()) and bool((ib[r] == -1).all())
        assert not bool((ib[keep] == r).any()), "a non-finite point is somebody's neighbour"
    s = gsplat_amd.knn_scale_init(y, 3)
    assert torch.equal(s[keep], gsplat_amd.knn_scale_init(x.to(DEV), 3)) and bool(s[100].isnan())


@functools.lru_cache(maxsize=None)
def uniform_reference():
    """The 16 smallest float64 distances of every row of the uniform cube, on the CPU, once."""
    x = kc.uniform()
    return x, kc.brute_force(x, 16)[0]


@pytest.mark.parametrize("K", [1, 4, 16])
def test_uniform_cube_against_float64_brute_force(K):
    """N = 20 000: a 20 x 20 x 20 grid, the multi-ring walk; K = 16 fills the register best-list. The bound: the float32 distance of two
    float32 points from coordinate differences is within 3 roundings of the float64 one (each difference is one rounding of an
    exact value, the sum of squares adds under two more, the root halves the relative error and adds one), so 4 ulp."""
    x, ref = uniform_reference()
    xg = x.to(DEV)
    dist, idx = fused(xg, K, True)
    check_rows(xg, dist, idx)
    st = iu.knn_last_stats()
    print(f"grid {st['dims']}, deferred {st['deferred']}")
    r = ref[:, :K]
    rel = float(((dist.cpu().double() - r).abs()[:, 1:] / r[:, 1:]).max()) if K > 1 else 0.0
    print(f"K {K}: rel diff against float64 {rel:.3e}")
    assert rel <= 4 * kc.ULP
    assert torch.equal(dist, fused(xg, K)), "two calls differ"


def test_nothing_is_read_back():
    x = kc.points("clustered").to(DEV)
    ref = gsplat_amd.knn_scale_init(x, 3)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        s = gsplat_amd.knn_scale_init(x, 3)
        d, i = gsplat_amd.knn(x, 4, return_indices=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(s, ref) and d.shape == i.shape


def test_dispatch():
    x = kc.points("coplanar").to(DEV)
    assert iu._fused_ok(x, 16) and not iu._fused_ok(x, 17) and not iu._fused_ok(x.double(), 4)
    assert not iu._fused_ok(x.clone().requires_grad_(True), 4)
    with torch.no_grad():
        assert iu._fused_ok(x.clone().requires_grad_(True), 4)
    # the torch path on the device agrees with the kernels to the ulp rule
    a, b = gsplat_amd.knn(x, 4), iu.knn_torch(x, 4)
    assert float((a - b).abs().max()) <= 2 * kc.ULP * float(a.max())
    assert gsplat_amd.knn(x, 17).shape == (1000, 17)
