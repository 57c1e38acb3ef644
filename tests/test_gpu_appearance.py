"""GPU: the fused appearance kernels (csrc/appearance.hip) against tests/golden/appearance_ref.npz and against the torch
composition. Tolerance as in tests/test_appearance.py: 4 x the yardstick's own float32-vs-float64 spread plus one float32 ulp
of its largest magnitude, for every output including the summed weight and bias gradients. At N = 100 003, where no fixture
exists, the yardstick is the torch composition: its float64 run is the truth and its own float32 run gives the spread."""
import pytest
import torch

import gsplat_amd as gs
from _appearance_cases import OUTPUTS, PARAMS, amax, case_names, check_case, make_module, run_case
from _util import make_scene
from gsplat_amd import appearance as ap
from gsplat_amd.appearance import _FusedAppearance

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAU = 1e-4


def fused(m, f, ids, d, deg):
    before = _FusedAppearance.calls
    out = m(f, ids, d, deg)
    assert _FusedAppearance.calls == before + 1, "the fused kernels were not taken"
    return out


@pytest.mark.parametrize("name", case_names())
def test_fused_matches_reference(name):
    check_case(name, run_case(name, fused, device=DEV))


def drop_near_kinks(m, f, ids, d, deg):
    """Indices of the Gaussians none of whose float64 hidden pre-activations, in any camera, lies within TAU of zero."""
    m64 = make_module("m16", DEV, torch.float64)
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    pre = []
    hooks = [m64.color_head[i].register_forward_hook(lambda _m, _i, o: pre.append(o.detach().clone())) for i in (0, 2)]
    ap.appearance_torch(m64, f.double(), ids, d.double(), deg)
    for h in hooks:
        h.remove()
    near = torch.zeros(f.shape[0], dtype=torch.bool, device=f.device)
    for z in pre:
        near |= (z.abs() < TAU).any(dim=-1).any(dim=0)
    share = float(near.float().mean())
    print(f"near-kink share {share:.3%}")
    assert share <= 0.10
    return torch.nonzero(~near).flatten()


def all_outputs(fn, f, ids, d, w, deg, dtype):
    m = make_module("m16", DEV, dtype)
    f = f.to(dtype).clone().requires_grad_(True)
    d = d.to(dtype).clone().requires_grad_(True)
    colors = fn(m, f, ids, d, deg)
    (colors * w.to(dtype)).sum().backward()
    out = {"colors": colors.detach(), "v_features": f.grad, "v_dirs": d.grad, "v_embeds": m.embeds.weight.grad}
    for p in PARAMS:
        out["v_" + p] = m.color_head.get_parameter(p).grad
    return out


def test_fused_matches_float64_composition_large():
    """N = 100 003 (after dropping), C = 2: 782 row tiles of 128 over a persistent grid, the last one partial."""
    g = torch.Generator().manual_seed(7)
    N, C, deg = 100_003, 2, 3
    drawn = N + N // 8
    m = make_module("m16", DEV)
    f = (torch.randint(-32, 33, (drawn, 32), generator=g).float() / 32.0).to(DEV)
    d = (torch.randn(C, drawn, 3, generator=g) * 2.0).to(DEV)
    w = (torch.randint(-4, 5, (C, drawn, 3), generator=g).float() / 4.0).to(DEV)
    ids = torch.tensor([2, 1], device=DEV)
    keep = drop_near_kinks(m, f, ids, d, deg)
    assert keep.numel() >= N
    keep = keep[:N]
    f, d, w = f[keep].contiguous(), d[:, keep].contiguous(), w[:, keep].contiguous()
    r64 = all_outputs(ap.appearance_torch, f, ids, d, w, deg, torch.float64)
    r32 = all_outputs(ap.appearance_torch, f, ids, d, w, deg, torch.float32)
    got = all_outputs(fused, f, ids, d, w, deg, torch.float32)
    bad = []
    for k in OUTPUTS:
        err = amax(r32[k].double() - r64[k])
        diff, tol = amax(got[k].double() - r64[k]), 4 * err + 1.2e-7 * amax(r64[k])
        print(f"large {k}: fused-vs-f64 {diff:.3e} tol {tol:.3e} (float32 composition's own {err:.3e})")
        if not diff <= tol:
            bad.append((k, diff, tol))
    assert not bad, bad


def test_two_runs_are_bit_equal():
    a, b = run_case("d", fused, device=DEV), run_case("d", fused, device=DEV)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k


def test_no_device_read():
    m = make_module("m16", DEV)
    f = torch.randn(300, 32, device=DEV, requires_grad=True)
    d = torch.randn(2, 300, 3, device=DEV, requires_grad=True)
    ids = torch.ones(2, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fused(m, f, ids, d, 3).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert f.grad is not None and d.grad is not None


def test_strided_inputs_match_contiguous_copies():
    g = torch.Generator().manual_seed(3)
    wide = torch.randn(150, 40, generator=g).to(DEV)
    one = torch.randn(1, 150, 3, generator=g).to(DEV)
    ids = torch.tensor([0, 3], device=DEV)
    res = []
    for f0, d0 in ((wide[:, 5:37], one.expand(2, -1, -1)), (wide[:, 5:37].contiguous(), one.expand(2, -1, -1).contiguous())):
        m = make_module("m16", DEV)
        f, d = f0.detach().requires_grad_(True), d0.detach().requires_grad_(True)
        c = fused(m, f, ids, d, 3)
        c.square().sum().backward()
        res.append([c.detach(), f.grad, d.grad, m.embeds.weight.grad] + [p.grad for p in m.color_head.parameters()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_dirs_without_grad():
    g = torch.Generator().manual_seed(4)
    f0, d0 = torch.randn(200, 32, generator=g).to(DEV), torch.randn(2, 200, 3, generator=g).to(DEV)
    ids = torch.tensor([1, 2], device=DEV)
    res = []
    for want in (True, False):
        m = make_module("m16", DEV)
        f, d = f0.clone().requires_grad_(True), d0.clone().requires_grad_(want)
        fused(m, f, ids, d, 3).square().sum().backward()
        assert (d.grad is not None) == want
        res.append([f.grad, m.embeds.weight.grad] + [p.grad for p in m.color_head.parameters()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_fallback_configuration_on_gpu_matches_cpu():
    torch.manual_seed(5)
    m = ap.AppearanceOptModule(3, 32, embed_dim=16, sh_degree=3, mlp_width=32, mlp_depth=2)
    f, d, ids = torch.randn(100, 32), torch.randn(2, 100, 3), torch.tensor([2, 0])
    want = m(f, ids, d, 2)
    before = _FusedAppearance.calls
    got = m.to(DEV)(f.to(DEV), ids.to(DEV), d.to(DEV), 2)
    assert _FusedAppearance.calls == before
    assert float((got.cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_training_step_end_to_end():
    """colors = sigmoid(app(features, ids, means - camera centres, degree) + base) -> rasterization -> photometric loss."""
    sc, W, H = make_scene(N=3000, C=2, width=64, height=64, seed=2, device=DEV)
    g = torch.Generator().manual_seed(6)
    target = torch.rand(2, 3, H, W, generator=g).to(DEV)
    c2w = torch.linalg.inv(sc["viewmats"])
    ids = torch.tensor([1, 3], device=DEV)
    grads = {}
    for detach in (False, True):
        m = make_module("m16", DEV)
        means = sc["means"].clone().requires_grad_(True)
        features = (torch.randn(3000, 32, generator=torch.Generator().manual_seed(8)) * 0.5).to(DEV).requires_grad_(True)
        base = sc["colors"].clone().requires_grad_(True)
        dirs = means[None] - c2w[:, None, :3, 3]
        colors = torch.sigmoid(fused(m, features, ids, dirs.detach() if detach else dirs, 3) + base)
        rc, _ra, _meta = gs.rasterization(means, sc["quats"], sc["scales"], sc["opacities"], colors, sc["viewmats"], sc["Ks"], W, H,
                                          sh_degree=None)
        gs.photometric_loss(rc.permute(0, 3, 1, 2), target).backward()
        grads[detach] = means.grad
        if not detach:
            for name, t in [("features", features), ("means", means), ("embeds", m.embeds.weight)] + list(m.color_head.named_parameters()):
                assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0, name
    assert float((grads[False] - grads[True]).abs().max()) > 0, "no gradient reaches means through v_dirs"
