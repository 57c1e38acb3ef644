"""CPU: HexPlaneField's surface and its torch composition against tests/golden/hexplane_ref.npz (the reference on the CPU,
tools/pin_hexplane_against_reference.py), and the three regularisers. Tolerance: 4 x the reference's own float32-vs-float64 spread
plus one float32 ulp of its largest magnitude, for every output."""
import itertools

import pytest
import torch

import gsplat_amd as gs
from _hexplane_cases import (case_names, check, check_case, config, golden, make_field, run_case, state_dict)
from gsplat_amd import hexplane as hp
from gsplat_amd.hexplane import HexPlaneField, _FusedHexPlane

PAIRS = list(itertools.combinations(range(4), 2))


def test_exported_from_the_package():
    assert gs.HexPlaneField is HexPlaneField and gs.hexplane is hp and gs.hexplane_torch is hp.hexplane_torch
    for name in ("plane_smoothness", "time_smoothness", "time_l1", "hexplane_regularization"):
        assert getattr(gs, name) is getattr(hp, name)


def test_default_constructor():
    f = HexPlaneField()
    assert f.bounds == 1.6 and f.concat_features is True and f.feat_dim == 64 and f.multires == [1, 2]
    assert f.grid_config == {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32,
                             "resolution": [64, 64, 64, 25]}
    assert isinstance(f.aabb, torch.nn.Parameter) and not f.aabb.requires_grad and f.aabb.dtype == torch.float32
    assert torch.equal(f.aabb.detach(), torch.tensor([[1.6] * 3, [-1.6] * 3]))
    assert isinstance(f.grids, torch.nn.ModuleList) and len(f.grids) == 2
    for factor, planes in zip((1, 2), f.grids):
        assert isinstance(planes, torch.nn.ParameterList) and len(planes) == 6
        reso = [64 * factor] * 3 + [25]
        for p, (a, b) in zip(planes, PAIRS):
            assert tuple(p.shape) == (1, 32, reso[b], reso[a]) and p.requires_grad
    assert [tuple(p.shape) for p in f.spatial_planes()] == [(1, 32, 64, 64)] * 3 + [(1, 32, 128, 128)] * 3
    assert [tuple(p.shape) for p in f.temporal_planes()] == [(1, 32, 25, 64)] * 3 + [(1, 32, 25, 128)] * 3
    assert f.spatial_planes()[1] is f.grids[0][1] and f.temporal_planes()[4] is f.grids[1][4]


def test_custom_constructor():
    cfg = {"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 8, "resolution": [5, 6, 7, 4]}
    f = HexPlaneField(bounds=2.0, planes_config=cfg, multires=(1, 3, 2))
    assert f.bounds == 2.0 and f.feat_dim == 24 and f.multires == [1, 3, 2] and f.grid_config == cfg
    assert torch.equal(f.aabb.detach(), torch.tensor([[2.0] * 3, [-2.0] * 3]))
    for factor, planes in zip((1, 3, 2), f.grids):
        reso = [5 * factor, 6 * factor, 7 * factor, 4]  # a scale multiplies the spatial resolutions only
        assert [tuple(p.shape) for p in planes] == [(1, 8, reso[b], reso[a]) for a, b in PAIRS]
    assert f(torch.zeros(3, 4)).shape == (3, 24)


def test_constructor_errors():
    with pytest.raises(ValueError, match=r"_init_grid_param: in_dim=4 != len\(reso\)=3\."):
        HexPlaneField(planes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 4,
                                     "resolution": [4, 4, 4]})
    with pytest.raises(ValueError, match=r"_init_grid_param: grid_nd=5 > in_dim=4\."):
        HexPlaneField(planes_config={"grid_dimensions": 5, "input_coordinate_dim": 4, "output_coordinate_dim": 4,
                                     "resolution": [4, 4, 4, 4]})


def test_initialisation_rule():
    torch.manual_seed(0)
    f = HexPlaneField()
    for planes in f.grids:
        for p, pair in zip(planes, PAIRS):
            p = p.detach()
            if 3 in pair:
                assert bool((p == 1.0).all())
            else:
                assert float(p.min()) >= 0.1 and float(p.max()) <= 0.5 and float(p.std()) > 0.05
                assert abs(float(p.mean()) - 0.3) < 0.01


def test_state_dict_keys_and_strict_load():
    f = HexPlaneField()
    assert list(f.state_dict()) == ["aabb"] + [f"grids.{s}.{p}" for s in range(2) for p in range(6)]
    for fname, multires in config()["multires"].items():
        sd = state_dict(fname)
        assert sorted(sd) == sorted(["aabb"] + [f"grids.{s}.{p}" for s in range(len(multires)) for p in range(6)])
        m = make_field(fname)  # load_state_dict(strict=True) of the reference's state dict
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd[k]), k


@pytest.mark.parametrize("name", case_names())
def test_composition_matches_reference(name):
    check_case(name, run_case(name, hp.hexplane_torch))


def test_module_call_on_cpu_takes_the_torch_route():
    before = _FusedHexPlane.calls
    got = run_case("f", lambda field, x: field(x))
    assert _FusedHexPlane.calls == before
    check_case("f", got)


def test_last_dim_must_be_four():
    f = make_field("m1")
    for fn in (f, lambda x: hp.hexplane(f, x), lambda x: hp.hexplane_torch(f, x)):
        with pytest.raises(ValueError, match=r"HexPlaneField\.forward: xyzt last dim must be 4, got shape \(5, 3\)\."):
            fn(torch.zeros(5, 3))


def test_leading_shape_is_flattened():
    f = make_field("m2")
    x = torch.from_numpy(golden()["g_xyzt"])[:30]
    flat = f(x)
    assert flat.shape == (30, 64)
    assert torch.equal(f(x.view(2, 3, 5, 4)), flat) and torch.equal(f(x.view(1, 30, 4)), flat)
    assert torch.equal(f(x[0]), flat[:1])
    empty = f(torch.zeros(0, 4))
    assert empty.shape == (0, 64) and empty.dtype == torch.float32
    assert f(torch.zeros(2, 0, 4)).shape == (0, 64)


def test_regularisers_match_reference():
    z = golden()
    f = make_field("m2")
    got = {"plane_smoothness": hp.plane_smoothness(f.spatial_planes()), "time_smoothness": hp.time_smoothness(f.temporal_planes()),
           "time_l1": hp.time_l1(f.temporal_planes())}
    total = hp.hexplane_regularization(f, *[float(v) for v in z["reg_lambdas"]])
    total.backward()
    got["total"] = total
    for k, p in f.grids.named_parameters():
        got["v_grids." + k] = p.grad
    assert len(got) == 4 + 12
    bad = [check("reg", v.detach(), torch.from_numpy(z["reg_" + k]), float(z["reg_err_" + k]), k) for k, v in got.items()]
    assert not any(bad), [b for b in bad if b]
    # the default weights are one each
    want = got["plane_smoothness"] + got["time_smoothness"] + got["time_l1"]
    assert abs(float(hp.hexplane_regularization(f)) - float(want)) <= 1e-6 * float(want)


def test_regulariser_edges():
    g = torch.Generator().manual_seed(1)
    tall, short = torch.rand(1, 4, 5, 3, generator=g), torch.rand(1, 4, 2, 3, generator=g)
    for fn in (hp.plane_smoothness, hp.time_smoothness):
        d2 = tall[..., 2:, :] - 2.0 * tall[..., 1:-1, :] + tall[..., :-2, :]
        assert abs(float(fn([tall])) - float(d2.pow(2).mean())) <= 1e-6
        assert torch.equal(fn([tall, short]), fn([tall]))  # H < 3 contributes nothing
        only_short = fn([short.double()])
        assert only_short.shape == () and float(only_short) == 0.0 and only_short.dtype == torch.float64
        with pytest.raises(ValueError, match=r"Expected 4D plane tensors \(B, C, H, W\); got 3D shape \(4, 5, 3\)\."):
            fn([tall[0]])
    assert abs(float(hp.time_l1([tall, short])) - float((1 - tall).abs().mean() + (1 - short).abs().mean())) <= 1e-6
    for fn in (hp.plane_smoothness, hp.time_smoothness, hp.time_l1):
        zero = fn([])
        assert zero.shape == () and float(zero) == 0.0 and zero.dtype == torch.float32


def test_symbols_are_declared():
    from gsplat_amd import _cabi

    for name in ("gsx_hexplane_scale_cells", "gsx_hexplane_pack", "gsx_hexplane_unpack", "gsx_hexplane_fwd", "gsx_hexplane_bwd"):
        assert name in _cabi.exported_symbols()
    assert _cabi.query("gsx_hexplane_scale_cells", 5, 6, 7, 4) == 5 * 6 + 5 * 7 + 5 * 4 + 6 * 7 + 6 * 4 + 7 * 4
    assert _cabi.query("gsx_hexplane_scale_cells", 5, 1, 7, 4) == 0 and _cabi.query("gsx_hexplane_scale_cells", 5, 6, 2049, 4) == 0
