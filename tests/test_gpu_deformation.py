"""GPU: the fused deformation kernels (csrc/deformation.hip) against tests/golden/deformation_ref.npz and against the torch
composition. Tolerance as in tests/test_deformation.py: 4 x the yardstick's own float32-vs-float64 spread plus one float32 ulp
of its largest magnitude, for every output including the summed weight and bias gradients. Where no fixture exists the yardstick
is the torch composition: its float64 run is the truth and its own float32 run gives the spread."""
import pytest
import torch

import gsplat_amd as gs
from _deformation_cases import (INPUTS, NEW, OUTPUTS, PARAMS, TAU, TRUNK, all_outputs, call_module, case_names, check_case, compare,
                                make_module, run_case)
from _util import make_scene
from gsplat_amd import deformation as df
from gsplat_amd.deformation import _FusedDeform

pytestmark = pytest.mark.gpu
DEV = "cuda"


def fused(m, means, quats, opacities, x):
    before = _FusedDeform.calls
    out = m(means, quats, opacities, None, x)
    assert _FusedDeform.calls == before + 1, "the fused kernels were not taken"
    return out


def draw(N, seed, spare=0):
    """(means, quats, opacities, plane_features), (w_means, w_quats, w_opac) on the GPU, the fixture's value sets."""
    g = torch.Generator().manual_seed(seed)
    n = N + spare
    inputs = [(torch.randint(-32, 33, (n, d), generator=g).float() / 32.0).to(DEV) for d in (3, 4, 1, 64)]
    weights = [(torch.randint(-4, 5, (n, d), generator=g).float() / 4.0).to(DEV) for d in (3, 4, 1)]
    return inputs, weights


def randomize_heads(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for head in (m.pos_head, m.quat_head, m.opacity_head):
            for p in head.parameters():
                p.copy_(((torch.rand(p.shape, generator=g) * 2.0 - 1.0) * 0.125).to(p.device))
    return m


def three_runs(mname, inputs, weights):
    """(fused float32, composition float32, composition float64) on the same inputs."""
    r64 = all_outputs(df.deform_torch, make_module(mname, DEV, torch.float64), [t.double() for t in inputs],
                      [w.double() for w in weights])
    r32 = all_outputs(df.deform_torch, make_module(mname, DEV), inputs, weights)
    got = all_outputs(fused, make_module(mname, DEV), inputs, weights)
    return got, r32, r64


@pytest.mark.parametrize("name", case_names())
def test_fused_matches_reference(name):
    check_case(name, run_case(name, fused, device=DEV))


def test_fused_matches_float64_composition_large():
    """N = 100 003 (after dropping): 3126 row tiles over a persistent grid of 256 workgroups, the last tile partial."""
    N = 100_003
    inputs, weights = draw(N, seed=7, spare=N // 8)
    m64 = make_module("d3", DEV, torch.float64)
    pre = []
    hooks = [m64.trunk[i].register_forward_hook(lambda _m, _i, o: pre.append(o.detach())) for i in (0, 2, 4)]
    m64.trunk(inputs[3].double())
    for h in hooks:
        h.remove()
    near = torch.zeros(inputs[3].shape[0], dtype=torch.bool, device=DEV)
    for z in pre:
        near |= (z.abs() < TAU).any(dim=-1)
    share = float(near.float().mean())
    print(f"near-kink share {share:.3%}")
    assert share <= 0.05
    keep = torch.nonzero(~near).flatten()
    assert keep.numel() >= N
    keep = keep[:N]
    inputs, weights = [t[keep].contiguous() for t in inputs], [t[keep].contiguous() for t in weights]
    got, r32, r64 = three_runs("d3", inputs, weights)
    compare("large", got, r32, r64)


def test_two_runs_are_bit_equal():
    a, b = run_case("f", fused, device=DEV), run_case("f", fused, device=DEV)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k


def test_no_device_read():
    m = make_module("d3", DEV)
    inputs, weights = draw(300, seed=2)
    leaves = [t.requires_grad_(True) for t in inputs]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = fused(m, *leaves)
        sum((o * w).sum() for o, w in zip(outs, weights)).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.grad is not None for t in leaves) and all(p.grad is not None for p in m.parameters())


def test_strided_inputs_match_contiguous_copies():
    """plane_features a column slice of a wider tensor (rows 288 bytes apart, the slice 20 bytes in: not 16-byte aligned), means
    and quats slices of one [N, 8] buffer."""
    g = torch.Generator().manual_seed(3)
    N = 150
    wide = torch.randn(N, 72, generator=g).to(DEV)
    mq = torch.randn(N, 8, generator=g).to(DEV)
    opac = torch.randn(N, 1, generator=g).to(DEV)
    views = (mq[:, :3], mq[:, 4:], opac, wide[:, 5:69])
    assert not views[3].is_contiguous() and not views[0].is_contiguous() and not views[1].is_contiguous()
    odd = torch.empty(N * 64 + 1, device=DEV)[1:].view(N, 64).copy_(views[3])  # contiguous, but 4 bytes off a 16-byte boundary
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4
    res = []
    for inputs in (views, tuple(v.contiguous() for v in views), views[:3] + (odd,)):
        m = make_module("d3", DEV)
        leaves = [t.detach().requires_grad_(True) for t in inputs]
        outs = fused(m, *leaves)
        sum(o.square().sum() for o in outs).backward()
        res.append([o.detach() for o in outs] + [t.grad for t in leaves] + [p.grad for p in m.parameters()])
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert a.shape == b.shape and torch.equal(a, b)


def test_plane_features_without_grad():
    inputs, weights = draw(200, seed=4)
    res = []
    for want in (True, False):
        m = make_module("d3", DEV)
        leaves = [t.clone().requires_grad_(want or i < 3) for i, t in enumerate(inputs)]
        outs = fused(m, *leaves)
        sum((o * w).sum() for o, w in zip(outs, weights)).backward()
        assert (leaves[3].grad is not None) == want
        res.append([t.grad for t in leaves[:3]] + [p.grad for p in m.parameters()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("only", [0, 2])
def test_loss_on_one_output_only(only):
    """The other two cotangents reach the backward as None (null pointers to the kernel)."""
    inputs, weights = draw(333, seed=5 + only)

    def one(fn):
        return lambda m, *a: tuple(o if i == only else o.detach() for i, o in enumerate(fn(m, *a)))

    r64 = all_outputs(one(df.deform_torch), make_module("d3", DEV, torch.float64), [t.double() for t in inputs],
                      [w.double() for w in weights])
    r32 = all_outputs(one(df.deform_torch), make_module("d3", DEV), inputs, weights)
    got = all_outputs(one(fused), make_module("d3", DEV), inputs, weights)
    unused = ["v_" + INPUTS[i] for i in range(3) if i != only]
    for k in unused:
        assert got[k] is None and r32[k] is None, k
    compare(f"only {NEW[only]}", got, r32, r64, keys=[k for k in OUTPUTS if k not in unused])
    assert float(got["v_trunk.0.weight"].abs().max()) > 0


def test_zero_heads():
    """A fresh module: the outputs are the inputs, every trunk gradient is exactly zero, the head gradients are not."""
    inputs, weights = draw(500, seed=9)
    got, r32, r64 = three_runs("z3", inputs, weights)
    for k, t in zip(NEW, inputs[:3]):
        assert torch.equal(got[k], t), k
    for p in TRUNK:
        assert float(got["v_" + p].abs().max()) == 0.0, p
    assert float(got["v_plane_features"].abs().max()) == 0.0
    heads = ["v_" + p for p in PARAMS if p not in TRUNK]
    compare("zero heads", got, r32, r64, keys=heads)
    for k in heads:
        assert float(got[k].abs().max()) > 0, k


@pytest.mark.parametrize("kwargs,feature_dim,dtype", [({"hidden_dim": 32}, 64, torch.float32), ({"num_layers": 2}, 64, torch.float32),
                                                      ({}, 32, torch.float32), ({}, 64, torch.float64)])
def test_fallback_configuration_on_gpu_matches_cpu(kwargs, feature_dim, dtype):
    torch.manual_seed(5)
    m = randomize_heads(df.DeformNetwork(feature_dim, **kwargs), 6).to(dtype)
    inputs = [torch.randn(100, d, dtype=dtype) for d in (3, 4, 1, feature_dim)]
    want = call_module(m, *inputs)
    before = _FusedDeform.calls
    got = call_module(m.to(DEV), *[t.to(DEV) for t in inputs])
    assert _FusedDeform.calls == before
    for a, b in zip(got, want):
        assert float((a.detach().cpu() - b.detach()).abs().max()) <= 1e-5 * float(b.detach().abs().max())


def test_training_step_end_to_end():
    """plane features from a stand-in with parameters (a linear map of the means) -> fused deform -> packed rasterization with an
    expected-depth channel -> photometric loss."""
    sc, W, H = make_scene(N=3000, C=2, width=64, height=64, seed=2, device=DEV)
    target = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(6)).to(DEV)
    torch.manual_seed(8)
    field = torch.nn.Linear(3, 64).to(DEV)
    m = randomize_heads(make_module("d3", DEV), 10)
    means = sc["means"].clone().requires_grad_(True)
    means_new, quats_new, opac_new = fused(m, means, sc["quats"], sc["opacities"][:, None], field(means))
    rc, _ra, _meta = gs.rasterization(means_new, quats_new, sc["scales"], opac_new[:, 0].clamp(0.01, 0.99), sc["colors"],
                                      sc["viewmats"], sc["Ks"], W, H, sh_degree=None, packed=True, render_mode="RGB+ED")
    assert rc.shape == (2, H, W, 4)
    gs.photometric_loss(rc[..., :3].permute(0, 3, 1, 2).contiguous(), target).backward()
    for name, t in [("means", means)] + [("field." + k, p) for k, p in field.named_parameters()] + list(m.named_parameters()):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0, name
