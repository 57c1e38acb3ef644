"""GPU: the ops whose Python bodies hand several `.contiguous()` temporaries to one C-ABI call give the same bits for strided
inputs as for contiguous ones. Each tensor input is replaced by torch.stack((t, t), -1)[..., 0] - same values and shape at
stride 2 - so that every `.contiguous()` in the body makes a copy; N = 1024 rows are copies of the size the caching allocator
hands out again at once, which is what a call that dropped them before the launch would trip over. One 64 x 64 image, tile
size 16, tile lists from intersect_tile on a _util.make_scene scene. With two devices: inputs on the device that is not
current give the bits of the current one, and inputs on both are refused."""
import pytest
import torch

from _util import make_scene

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, W, H, TS = 1024, 64, 64, 16
GLOBAL_SHUTTER = 4  # RollingShutterType.GLOBAL


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd

    return gsplat_amd


@pytest.fixture(scope="module")
def scene(G):
    """One camera: the scene, its projection and its sorted tile lists."""
    sc, _, _ = make_scene(N=N, C=1, width=W, height=H, seed=3)
    s = {k: v.to(DEV) for k, v in sc.items()}
    rad, m2, d, con, _ = G.fully_fused_projection(s["means"], None, s["quats"], s["scales"], s["viewmats"], s["Ks"], W, H,
                                                  opacities=s["opacities"])
    op = s["opacities"][None].contiguous()
    tw, th = W // TS, H // TS
    _, ids, fl = G.isect_tiles(m2, rad, d, TS, tw, th, conics=con, opacities=op)
    # make_scene spreads the means over 1.3 x the image each way: (1 / 1.3)^2 = 59 % of them are in view, each in >= 1 tile
    assert fl.numel() >= N // 2, "the lists are too short to say anything"
    s.update(means2d=m2, conics=con, opac=op, offsets=G.isect_offset_encode(ids, 1, tw, th), flatten_ids=fl)
    return s


def _strided(t):
    """Same values, same shape, stride 2."""
    v = torch.stack((t, t), -1)[..., 0]
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


def _both(name, *args, keep=()):
    """The op's body on `args` as they are and with every tensor among them strided (positions in `keep` excepted: an output
    updated in place, cloned per run). Returns the two lists of tensor results."""
    from gsplat_amd import _ops

    body = _ops.impl(name)
    runs = []
    for swap in (False, True):
        a = [x.clone() if i in keep else _strided(x) if swap and isinstance(x, torch.Tensor) else x for i, x in enumerate(args)]
        out = body(*a)
        out = [a[i] for i in keep] if keep else ([out] if isinstance(out, torch.Tensor) else list(out))
        runs.append([t for t in out if t is not None])
    torch.cuda.synchronize()
    return runs


def _assert_same(runs, name):
    plain, strided = runs
    assert len(plain) == len(strided) and len(plain) > 0
    for k, (p, s) in enumerate(zip(plain, strided)):
        assert p.shape == s.shape and p.numel() > 0, (name, k, p.shape, s.shape)
        assert torch.equal(p, s), f"{name}: output {k} differs on {int((p != s).sum())} of {p.numel()} elements"


def test_query_rasterizers(scene):
    q = (scene["means2d"], scene["conics"], scene["opac"], scene["offsets"], scene["flatten_ids"], W, H, TS)
    runs = _both("rasterize_num_contributing_gaussians", *q)
    _assert_same(runs, "num_contributing")
    counts = runs[0][0]
    assert int(counts.max()) > 1
    _assert_same(_both("rasterize_contributing_gaussian_ids", *q, counts), "contributing_ids")


def test_rasterize_to_indices(scene):
    T0 = torch.ones(1, H, W, device=DEV)
    runs = _both("rasterize_to_indices_3dgs", 0, 10 ** 6, T0, scene["means2d"], scene["conics"], scene["opac"], W, H, TS,
                 scene["offsets"], scene["flatten_ids"])
    _assert_same(runs, "rasterize_to_indices_3dgs")


def test_mcmc_perturb_positions(scene):
    g = torch.Generator().manual_seed(4)
    noise = torch.randn(N, 3, generator=g).to(DEV)
    # the op takes log scales and opacity logits; densities around its threshold t = 0.005 give every row a visible step
    logits = torch.logit(scene["opacities"] * 0.02)
    runs = _both("mcmc_perturb_positions", scene["means"], scene["quats"], scene["scales"].log(), logits, noise, 0.5,
                 keep=(0,))  # positions: updated in place, must be contiguous
    _assert_same(runs, "mcmc_perturb_positions")
    assert bool((runs[0][0] != scene["means"]).any(-1).all()), "a row was not perturbed: the inputs say nothing"


def test_projection_ewa_simple_bwd(G, scene):
    g = torch.Generator().manual_seed(5)
    covars, _ = G.quat_scale_to_covar_preci(scene["quats"], scene["scales"], compute_preci=False, triu=False)
    v_m2, v_c2 = torch.randn(1, N, 2, generator=g).to(DEV), torch.randn(1, N, 2, 2, generator=g).to(DEV)
    # camera 0 of make_scene sits at the origin: the world-space means are its camera-space means
    runs = _both("projection_ewa_simple_bwd", scene["means"][None], covars[None], scene["Ks"], W, H, 0, v_m2, v_c2)
    _assert_same(runs, "projection_ewa_simple_bwd")


def test_quat_scale_to_covar_preci_bwd(scene):
    g = torch.Generator().manual_seed(6)
    v_cov, v_pre = torch.randn(N, 3, 3, generator=g).to(DEV), torch.randn(N, 3, 3, generator=g).to(DEV)
    runs = _both("quat_scale_to_covar_preci_bwd", scene["quats"], scene["scales"], False, v_cov, v_pre)
    _assert_same(runs, "quat_scale_to_covar_preci_bwd")


def test_projection_ut_pinhole_global_shutter(scene):
    runs = _both("projection_ut_3dgs_fused", scene["means"], scene["quats"], scene["scales"], scene["opacities"],
                 scene["viewmats"], None, scene["Ks"], W, H, 0.3, 0.01, 1e10, 0.0, True, 0, True, None, GLOBAL_SHUTTER, None,
                 None, None, None, None, None)
    _assert_same(runs, "projection_ut_3dgs_fused")
    assert len(runs[0]) == 5 and int((runs[0][0] > 0).all(-1).sum()) > N // 4  # radii: the scene is in view


def test_launch_follows_the_tensors_device(G):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    from gsplat_amd import _cabi, _ops

    sc, _, _ = make_scene(N=N, C=1, width=W, height=H, seed=3)
    body = _ops.impl("quat_scale_to_covar_preci")
    torch.cuda.set_device(0)
    on0 = body(sc["quats"].to("cuda:0"), sc["scales"].to("cuda:0"), True, True, False)
    on1 = body(sc["quats"].to("cuda:1"), sc["scales"].to("cuda:1"), True, True, False)
    assert torch.cuda.current_device() == 0
    for a, b in zip(on0, on1):
        assert b.device == torch.device("cuda", 1) and torch.equal(a.cpu(), b.cpu())
    with pytest.raises(_cabi.GsplatAmdError, match="cuda:0.*cuda:1|cuda:1.*cuda:0"):
        body(sc["quats"].to("cuda:0"), sc["scales"].to("cuda:1"), True, True, False)
