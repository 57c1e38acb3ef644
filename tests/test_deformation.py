"""CPU: the deformation module (gsplat_amd/deformation.py) in its torch composition against tests/golden/deformation_ref.npz, the
reference's own DeformNetwork evaluated in float32 and float64, and DeformationTable against the reference's recorded masks
(tools/pin_deformation_against_reference.py). Tolerance: 4 x the reference's own float32-vs-float64 spread plus one float32 ulp
of its largest magnitude."""
import json

import pytest
import torch

import gsplat_amd
from _deformation_cases import call_module, case_names, check_case, golden, make_module, run_case, state_dict
from gsplat_amd import deformation as df
from gsplat_amd.deformation import _FusedDeform


@pytest.mark.parametrize("name", case_names())
def test_torch_composition_matches_reference(name):
    check_case(name, run_case(name, df.deform_torch))


@pytest.mark.parametrize("name", ["c", "g"])
def test_module_call_on_cpu_is_the_composition(name):
    """CPU tensors never reach the C-ABI."""
    before = _FusedDeform.calls
    a, b = run_case(name, call_module), run_case(name, df.deform_torch)
    assert _FusedDeform.calls == before
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_state_dict_is_the_references():
    sd = state_dict()
    assert set(sd) == {f"{m}.{p}" for m in ("trunk.0", "trunk.2", "trunk.4", "pos_head", "quat_head", "opacity_head")
                       for p in ("weight", "bias")}
    m = df.DeformNetwork(64)
    mine = m.state_dict()
    assert list(mine) == [k[len("d3_sd_"):] for k in golden() if k.startswith("d3_sd_")]  # same keys, same order
    for k, v in sd.items():
        assert tuple(mine[k].shape) == tuple(v.shape), k
    m.load_state_dict(sd, strict=True)
    back = make_module("d3").state_dict()
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    assert (m.feature_dim, m.hidden_dim, m.num_layers) == (64, 64, 3)


def test_exported_names():
    assert gsplat_amd.DeformNetwork is df.DeformNetwork
    assert gsplat_amd.DeformationTable is df.DeformationTable
    assert gsplat_amd.deformation is df
    assert {"DeformNetwork", "DeformationTable", "deformation"} <= set(dir(gsplat_amd))


@pytest.mark.parametrize("feature_dim,hidden_dim,num_layers", [(64, 64, 3), (10, 32, 1), (7, 16, 4)])
def test_zero_heads_return_the_inputs(feature_dim, hidden_dim, num_layers):
    torch.manual_seed(1)
    m = df.DeformNetwork(feature_dim, hidden_dim=hidden_dim, num_layers=num_layers)
    assert len(m.trunk) == 2 * num_layers
    for head in (m.pos_head, m.quat_head, m.opacity_head):
        assert float(head.weight.detach().abs().max()) == 0.0 and float(head.bias.detach().abs().max()) == 0.0
    means, quats, opac, x = torch.randn(37, 3), torch.randn(37, 4), torch.randn(37, 1), torch.randn(37, feature_dim)
    for got, want in zip(m(means, quats, opac, torch.zeros(37, 1), x), (means, quats, opac)):
        assert torch.equal(got, want)


def test_configuration_outside_the_fused_set_is_the_plain_mlp():
    torch.manual_seed(2)
    m = df.DeformNetwork(10, hidden_dim=32, num_layers=2)
    with torch.no_grad():
        for head in (m.pos_head, m.quat_head, m.opacity_head):
            for p in head.parameters():
                p.uniform_(-0.2, 0.2)
    means, quats, opac, x = torch.randn(21, 3), torch.randn(21, 4), torch.randn(21, 1), torch.randn(21, 10)
    h = torch.relu(torch.relu(x @ m.trunk[0].weight.t() + m.trunk[0].bias) @ m.trunk[2].weight.t() + m.trunk[2].bias)
    got = m(means, quats, opac, None, x)
    want = (means + h @ m.pos_head.weight.t() + m.pos_head.bias, quats + h @ m.quat_head.weight.t() + m.quat_head.bias,
            opac + h @ m.opacity_head.weight.t() + m.opacity_head.bias)
    for a, b in zip(got, want):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-6


def test_composition_is_twice_differentiable():
    m = make_module("d3", dtype=torch.float64)
    x = torch.randn(5, 64, dtype=torch.float64, requires_grad=True)
    means, quats, opac = (torch.randn(5, k, dtype=torch.float64) for k in (3, 4, 1))
    out = df.deform_torch(m, means, quats, opac, x)
    (gx,) = torch.autograd.grad(out[0].square().sum() + out[1].square().sum(), x, create_graph=True)
    gx.square().sum().backward()
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0


def test_constructor_errors():
    with pytest.raises(ValueError, match=r"num_layers must be >= 1, got 0\."):
        df.DeformNetwork(64, num_layers=0)
    with pytest.raises(ValueError, match=r"feature_dim must be >= 1, got 0\."):
        df.DeformNetwork(0)


def test_forward_errors():
    m = df.DeformNetwork(64)
    z = torch.zeros
    with pytest.raises(ValueError) as e:
        m(z(4, 3), z(5, 4), z(4, 1), None, z(4, 64))
    assert str(e.value) == "DeformNetwork: batch dim mismatch — means 4, quats 5, opacities 4, plane_features 4."
    with pytest.raises(ValueError):
        m(z(4, 3), z(4, 4), z(3, 1), None, z(4, 64))
    with pytest.raises(ValueError):
        m(z(4, 3), z(4, 4), z(4, 1), None, z(6, 64))
    with pytest.raises(ValueError) as e:
        m(z(4, 3), z(4, 4), z(4, 1), None, z(4, 32))
    assert str(e.value) == "DeformNetwork: plane_features last dim 32 != feature_dim 64."
    with pytest.raises(ValueError) as e:
        m(z(4, 3), z(4, 4, dtype=torch.float64), z(4, 1), None, z(4, 64))
    assert str(e.value) == ("DeformNetwork: dtype mismatch — means torch.float32, quats torch.float64, "
                            "opacities torch.float32, plane_features torch.float32.")
    with pytest.raises(ValueError):
        df.deform_torch(m, z(4, 3), z(4, 4), z(4, 1), z(4, 32))


def _table_args(kw):
    return {k: (torch.tensor(v, dtype=torch.bool) if k == "keep_mask" else torch.tensor(v) if isinstance(v, list) else v)
            for k, v in kw.items()}


def test_deformation_table_matches_the_reference_masks():
    """set_indices, prune, duplicate, then split with factors 1, 2 and 3, each on the table as the earlier steps left it."""
    z = golden()
    ops = json.loads(str(z["table_ops"]))
    assert [op for op, _ in ops] == ["set_indices", "set_indices", "prune", "duplicate", "split", "split", "split"]
    assert [kw["factor"] for op, kw in ops if op == "split"] == [1, 2, 3]
    t = df.DeformationTable(int(z["table_n"]))
    assert len(t) == int(z["table_n"]) and t.mask.dtype == torch.bool and not bool(t.mask.any())
    base = None
    for i, (op, kw) in enumerate(ops):
        if op == "split":
            t = df.DeformationTable(0)
            t.mask = base.clone()
        getattr(t, op)(**_table_args(kw))
        if op != "split":
            base = t.mask.clone()
        want = torch.from_numpy(z[f"table_mask_{i}"])
        assert t.mask.dtype == torch.bool and len(t) == want.numel() and torch.equal(t.mask, want), (i, op)


def test_deformation_table_split_defaults_to_two_children():
    a, b = df.DeformationTable(5), df.DeformationTable(5)
    for t in (a, b):
        t.set_indices(torch.tensor([0, 3]))
    a.split(torch.tensor([3, 1]))
    b.split(torch.tensor([3, 1]), factor=2)
    assert torch.equal(a.mask, b.mask) and a.mask.tolist() == [True, False, False, True, True, False, False]


def test_deformation_table_errors():
    with pytest.raises(ValueError, match=r"DeformationTable: num_gaussians must be >= 0, got -1\."):
        df.DeformationTable(-1)
    t = df.DeformationTable(4)
    with pytest.raises(ValueError) as e:
        t.prune(torch.ones(5, dtype=torch.bool))
    assert str(e.value) == "DeformationTable.prune: keep_mask shape (5,) != table shape (4,)."
    with pytest.raises(ValueError, match=r"DeformationTable.split: factor must be >= 1, got 0\."):
        t.split(torch.tensor([1]), factor=0)
    assert len(t) == 4
