"""GPU: the fused HexPlane kernels (csrc/hexplane.hip) against tests/golden/hexplane_ref.npz and against the torch composition.
Tolerance as in tests/test_hexplane.py: 4 x the yardstick's own float32-vs-float64 spread plus one float32 ulp of its largest
magnitude, for every output including the plane gradients. Where no fixture exists the yardstick is the torch composition: its
float64 run is the truth and its own float32 run gives the spread."""
import pytest
import torch

import gsplat_amd as gs
from _deformation_cases import compare
from _deformation_cases import make_module as make_deform
from _hexplane_cases import (all_outputs, case_inputs, case_names, check, check_case, golden, grid_keys, make_field, near_kink,
                             outputs, run_case)
from _util import make_scene
from gsplat_amd import hexplane as hp
from gsplat_amd.deformation import _FusedDeform
from gsplat_amd.hexplane import HexPlaneField, _FusedHexPlane

pytestmark = pytest.mark.gpu
DEV = "cuda"


def fused(field, xyzt):
    before = _FusedHexPlane.calls
    out = field(xyzt)
    assert _FusedHexPlane.calls == before + 1, "the fused kernels were not taken"
    return out


def draw(n, bounds, seed):
    """The pin tool's distribution: per axis three quarters inside the box, the rest up to 1.5 x bounds outside on either side;
    t in [-1.5, 1.5]."""
    g = torch.Generator().manual_seed(seed)
    inside = torch.rand(n, 4, generator=g) < 0.75
    u = torch.rand(n, 4, generator=g) * 2.0 - 1.0
    far = (1.0 + 0.5 * torch.rand(n, 4, generator=g)) * torch.where(torch.rand(n, 4, generator=g) < 0.5, -1.0, 1.0)
    xyzt = torch.where(inside, u, far) * bounds
    xyzt[:, 3] = torch.rand(n, generator=g) * 3.0 - 1.5
    return xyzt.contiguous().to(DEV)


def fixture_rule(tag, a, b, keys, name):
    """|a - b| under the rule, with case `name`'s reference as the magnitude and its spread as err."""
    z = golden()
    bad = [check(tag, a[k], b[k], float(z[f"{name}_err_{k}"]), k) for k in keys]
    assert not any(bad), (tag, [x for x in bad if x])


@pytest.mark.parametrize("name", case_names())
def test_fused_matches_reference(name):
    check_case(name, run_case(name, fused, device=DEV))


def test_default_field_matches_float64_composition():
    """The default field ([64, 64, 64, 25], scales 1 and 2, bounds 1.6), planes seeded uniform(-1, 1), N = 20 011 after dropping
    the rows next to a kink: 626 forward workgroups, 2.4 passes of the backward's grid of 8192 waves, the last pass partial."""
    N = 20_011
    g = torch.Generator().manual_seed(17)
    f32 = HexPlaneField()
    with torch.no_grad():
        for p in f32.grids.parameters():
            p.copy_(torch.rand(p.shape, generator=g) * 2.0 - 1.0)
    f32 = f32.to(DEV)
    f64 = HexPlaneField().to(DEV).double()
    f64.load_state_dict({k: v.double() for k, v in f32.state_dict().items()}, strict=True)
    xyzt = draw(N + N // 8, f32.bounds, seed=18)
    near = near_kink(f32, xyzt)
    share = float(near.float().mean())
    print(f"near-kink share {share:.3%}")
    assert share <= 0.05
    keep = torch.nonzero(~near).flatten()
    assert keep.numel() >= N
    xyzt = xyzt[keep[:N]].contiguous()
    w = (torch.randint(-4, 5, (N, 64), generator=g).float() / 4.0).to(DEV)
    r64 = all_outputs(hp.hexplane_torch, f64, xyzt.double(), w.double())
    r32 = all_outputs(hp.hexplane_torch, f32, xyzt, w)
    r32 = {k: v.clone() for k, v in r32.items()}
    got = all_outputs(fused, f32, xyzt, w)
    compare("default field", got, r32, r64, keys=outputs(f32))


def test_run_to_run():
    """features and v_xyzt are bit-equal; the plane gradients are sums of float atomics and stay within the rule."""
    a, b = run_case("h", fused, device=DEV), run_case("h", fused, device=DEV)
    assert torch.equal(a["features"], b["features"]) and torch.equal(a["v_xyzt"], b["v_xyzt"])
    fixture_rule("run to run", a, b, [k for k in a if k.startswith("v_grids.")], name="h")


def test_no_device_read():
    field = make_field("m2", DEV)
    xyzt, w = case_inputs("k", DEV)
    x = xyzt.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        (fused(field, x) * w).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert x.grad is not None and all(p.grad is not None for p in field.grids.parameters())


def test_strided_and_offset_inputs_match_contiguous_copies():
    """xyzt a column slice of a wider tensor (rows 36 bytes apart, the slice 8 bytes in), and a contiguous tensor 4 bytes off a
    16-byte boundary."""
    xyzt, w = case_inputs("g", DEV)
    N = xyzt.shape[0]
    wide = torch.zeros(N, 9, device=DEV)
    wide[:, 2:6] = xyzt
    view = wide[:, 2:6]
    odd = torch.empty(N * 4 + 1, device=DEV)[1:].view(N, 4).copy_(xyzt)
    assert not view.is_contiguous() and odd.is_contiguous() and odd.data_ptr() % 16 == 4
    res = [all_outputs(fused, make_field("m2", DEV), x, w) for x in (xyzt, view, odd)]
    for other in res[1:]:
        assert torch.equal(other["features"], res[0]["features"]) and torch.equal(other["v_xyzt"], res[0]["v_xyzt"])
        fixture_rule("strided", other, res[0], grid_keys(make_field("m2")), name="g")


def test_xyzt_without_grad():
    xyzt, w = case_inputs("h", DEV)
    with_grad = all_outputs(fused, make_field("m2", DEV), xyzt, w)
    field = make_field("m2", DEV)
    (fused(field, xyzt) * w).sum().backward()
    assert xyzt.grad is None and not xyzt.requires_grad
    without = {"v_grids." + k: p.grad for k, p in field.grids.named_parameters()}
    fixture_rule("xyzt without grad", without, with_grad, list(without), name="h")


def test_frozen_planes():
    xyzt, w = case_inputs("h", DEV)
    want = all_outputs(fused, make_field("m2", DEV), xyzt, w)
    field = make_field("m2", DEV).requires_grad_(False)
    got = all_outputs(fused, field, xyzt, w)
    assert all(p.grad is None for p in field.parameters())
    assert torch.equal(got["v_xyzt"], want["v_xyzt"]) and torch.equal(got["features"], want["features"])
    # some planes frozen: the others still get theirs
    field = make_field("m2", DEV)
    field.grids[0][2].requires_grad_(False)
    field.grids[1][0].requires_grad_(False)
    got = all_outputs(fused, field, xyzt, w)
    assert got["v_grids.0.2"] is None and got["v_grids.1.0"] is None
    fixture_rule("some frozen", got, want, [k for k in grid_keys(field) if got[k] is not None], name="h")
    assert sum(got[k] is not None for k in grid_keys(field)) == 10


def test_fresh_module_time_planes_get_gradients():
    got = run_case("j", fused, device=DEV)
    for s in range(2):
        for p in (2, 4, 5):
            assert float(got[f"v_grids.{s}.{p}"].abs().max()) > 0


def test_points_outside_the_box():
    """x, y, z beyond the box on either side, t inside: the features are those of the clamped point, bit for bit, v_xyzt is zero
    along x, y, z and not along t."""
    field = make_field("m2", DEV)  # bounds 1.0: the normalised border is exactly -1 / 1
    g = torch.Generator().manual_seed(5)
    N = 300
    sign = torch.where(torch.rand(N, 3, generator=g) < 0.5, -1.0, 1.0)
    xyz = sign * (1.01 + torch.rand(N, 3, generator=g) * 10.0)
    xyz[:4] = sign[:4] * torch.tensor([1e10, 3e38, 1.0000001, 2.0])[:, None]
    t = torch.rand(N, 1, generator=g) * 1.8 - 0.9
    w = torch.randn(N, 64, generator=g).to(DEV)
    outside, border = torch.cat([xyz, t], dim=1).to(DEV), torch.cat([sign, t], dim=1).to(DEV)
    keep = ~near_kink(field, outside)  # t next to a grid line: v_xyzt jumps there
    assert int(keep.sum()) >= N - N // 20
    outside, border, w = outside[keep], border[keep], w[keep]
    got, at_border = all_outputs(fused, field, outside, w), all_outputs(fused, field, border, w)
    assert bool(torch.isfinite(got["features"]).all()) and torch.equal(got["features"], at_border["features"])
    assert float(got["v_xyzt"][:, :3].abs().max()) == 0.0 and float(got["v_xyzt"][:, 3].abs().min()) > 0.0
    # and they are the composition's border values
    r32 = all_outputs(hp.hexplane_torch, field, outside, w)
    r32 = {k: v.clone() for k, v in r32.items()}
    r64 = all_outputs(hp.hexplane_torch, make_field("m2", DEV, torch.float64), outside.double(), w.double())
    compare("outside", got, r32, r64, keys=outputs(field))


@pytest.mark.parametrize("kind", ["channels16", "float64", "five_scales", "resolution1"])
def test_fallback_configuration_on_gpu_matches_cpu(kind):
    cfg = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32, "resolution": [5, 6, 7, 4]}
    multires, dtype = (1, 2), torch.float32
    if kind == "channels16":
        cfg["output_coordinate_dim"] = 16
    elif kind == "float64":
        dtype = torch.float64
    elif kind == "five_scales":
        multires = (1, 2, 3, 4, 5)
    else:
        cfg["resolution"] = [5, 1, 7, 4]
    torch.manual_seed(3)
    field = HexPlaneField(bounds=1.0, planes_config=cfg, multires=multires).to(dtype)
    with torch.no_grad():
        for p in field.grids.parameters():
            p.uniform_(-1.0, 1.0)
    xyzt = draw(100, 1.0, seed=4).cpu().to(dtype)
    want = field(xyzt)
    before = _FusedHexPlane.calls
    got = field.to(DEV)(xyzt.to(DEV))
    assert _FusedHexPlane.calls == before
    assert got.shape == want.shape == (100, field.feat_dim)
    assert float((got.detach().cpu() - want.detach()).abs().max()) <= 1e-5 * float(want.detach().abs().max())


def test_training_step_end_to_end():
    """HexPlaneField -> fused DeformNetwork -> packed rasterization with an expected-depth channel -> photometric loss plus the
    field's regularisers: every plane, the means and every network parameter get a finite, non-zero gradient."""
    sc, W, H = make_scene(N=3000, C=2, width=64, height=64, seed=2, device=DEV)
    target = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(6)).to(DEV)
    torch.manual_seed(8)
    cfg = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32, "resolution": [8, 8, 8, 4]}
    means = sc["means"].clone().requires_grad_(True)
    bounds = float(means.detach().abs().max()) * 1.05
    field = HexPlaneField(bounds=bounds, planes_config=cfg, multires=(1, 2)).to(DEV)
    with torch.no_grad():
        for p in field.temporal_planes():  # off their initial value: time_l1 has no gradient at exactly one
            p.add_(torch.rand_like(p) * 0.2 - 0.1)
    net = make_deform("d3", DEV)
    g = torch.Generator().manual_seed(10)
    with torch.no_grad():
        for head in (net.pos_head, net.quat_head, net.opacity_head):
            for p in head.parameters():
                p.copy_(((torch.rand(p.shape, generator=g) * 2.0 - 1.0) * 0.125).to(DEV))
    t = torch.full((means.shape[0], 1), 0.3, device=DEV)
    features = fused(field, torch.cat([means, t], dim=1))
    before = _FusedDeform.calls
    means_new, quats_new, opac_new = net(means, sc["quats"], sc["opacities"][:, None], t, features)
    assert _FusedDeform.calls == before + 1
    rc, _ra, _meta = gs.rasterization(means_new, quats_new, sc["scales"], opac_new[:, 0].clamp(0.01, 0.99), sc["colors"],
                                      sc["viewmats"], sc["Ks"], W, H, sh_degree=None, packed=True, render_mode="RGB+ED")
    assert rc.shape == (2, H, W, 4)
    loss = gs.photometric_loss(rc[..., :3].permute(0, 3, 1, 2).contiguous(), target) + 1e-3 * gs.hexplane_regularization(field)
    loss.backward()
    named = [("means", means)] + [("field." + k, p) for k, p in field.grids.named_parameters()] + list(net.named_parameters())
    assert len(named) == 1 + 12 + 12
    for name, p in named:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
