"""CPU: the appearance module (gsplat_amd/appearance.py) in its torch composition against tests/golden/appearance_ref.npz, the
reference's own AppearanceOptModule evaluated in float32 and float64 (tools/pin_appearance_against_reference.py). Tolerance: 4 x
the reference's own float32-vs-float64 spread plus one float32 ulp of its largest magnitude."""
import pytest
import torch

import gsplat_amd
from _appearance_cases import case_names, check_case, golden, make_module, run_case, state_dict
from gsplat_amd import appearance as ap


@pytest.mark.parametrize("name", case_names())
def test_torch_composition_matches_reference(name):
    check_case(name, run_case(name, ap.appearance_torch))


@pytest.mark.parametrize("name", ["c", "e"])
def test_module_call_on_cpu_is_the_composition(name):
    a, b = run_case(name, lambda m, *args: m(*args)), run_case(name, ap.appearance_torch)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mname", ["m16", "m0"])
def test_state_dict_is_the_references(mname):
    sd = state_dict(mname)
    assert set(sd) == {"embeds.weight", "color_head.0.weight", "color_head.0.bias", "color_head.2.weight", "color_head.2.bias",
                       "color_head.4.weight", "color_head.4.bias"}
    E = sd["embeds.weight"].shape[1]
    m = ap.AppearanceOptModule(4, 32, embed_dim=E, sh_degree=3, mlp_width=64, mlp_depth=2)
    mine = m.state_dict()
    assert list(mine) == [k[len(mname) + 4:] for k in golden() if k.startswith(mname + "_sd_")]  # same keys, same order
    for k, v in sd.items():
        assert tuple(mine[k].shape) == tuple(v.shape), k
    m.load_state_dict(sd, strict=True)
    assert tuple(m.color_head[0].weight.shape) == (64, E + 32 + 16)
    back = make_module(mname).state_dict()
    for k, v in sd.items():
        assert torch.equal(back[k], v), k


def test_exported_names():
    assert gsplat_amd.AppearanceOptModule is gsplat_amd.appearance.AppearanceOptModule
    assert gsplat_amd.appearance is ap
    assert "AppearanceOptModule" in dir(gsplat_amd)


@pytest.mark.parametrize("width,depth,embed_dim,feature_dim,module_degree", [(32, 2, 16, 32, 3), (64, 3, 8, 10, 2)])
def test_configuration_outside_the_fused_set(width, depth, embed_dim, feature_dim, module_degree):
    """Runs, and equals a direct restatement with torch.nn.Sequential."""
    torch.manual_seed(3)
    m = ap.AppearanceOptModule(5, feature_dim, embed_dim=embed_dim, sh_degree=module_degree, mlp_width=width, mlp_depth=depth)
    N, C, deg = 37, 2, module_degree - 1
    f, d = torch.randn(N, feature_dim), torch.randn(C, N, 3)
    ids = torch.tensor([4, 1])
    got = m(f, ids, d, deg)
    layers, n_in = [], embed_dim + feature_dim + (module_degree + 1) ** 2
    for i in range(depth):
        layers += [torch.nn.Linear(n_in if i == 0 else width, width), torch.nn.ReLU()]
    layers.append(torch.nn.Linear(width, 3))
    seq = torch.nn.Sequential(*layers)
    seq.load_state_dict(m.color_head.state_dict())
    u = torch.nn.functional.normalize(d, dim=-1)
    bases = torch.zeros(C, N, (module_degree + 1) ** 2)
    bases[..., :(deg + 1) ** 2] = ap.sh_bases_torch(deg, u)
    x = torch.cat([m.embeds.weight[ids][:, None].expand(-1, N, -1), f[None].expand(C, -1, -1), bases], dim=-1)
    want = seq(x)
    assert got.shape == (C, N, 3)
    assert float((got - want).detach().abs().max()) <= 1e-6 * float(want.detach().abs().max())


def test_argument_checks():
    m = ap.AppearanceOptModule(2, 32)
    with pytest.raises(ValueError):
        m(torch.zeros(4, 32), None, torch.zeros(1, 5, 3), 3)
    with pytest.raises(ValueError):
        m(torch.zeros(4, 32), None, torch.zeros(1, 4, 3), 4)
