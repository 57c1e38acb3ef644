"""Training-step components around the rasterizer: fused selective Adam, MCMC relocation and
noise kernels against the CPU oracle, strategy edits (row bookkeeping of parameters / optimizer state / statistics), and
a short end-to-end fit (rasterization + SelectiveAdam + DefaultStrategy / MCMCStrategy) whose loss must go down."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd
    import gsplat_amd._ops  # noqa: F401  (defines torch.ops.gsplat.*; the package itself loads lazily)

    return gsplat_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


@pytest.mark.parametrize("shape", [(1000, 3), (777,), (500, 16, 3), (64, 4), (2000, 15, 3), (4096, 3), (8192,), (4100, 2), (1001, 45)])
@pytest.mark.parametrize("masked", [True, False])
def test_adam_matches_oracle(G, O, shape, masked):
    g = torch.Generator().manual_seed(1)
    p, gr = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    m, v = torch.randn(shape, generator=g) * 0.1, torch.rand(shape, generator=g) * 0.1
    valid = (torch.rand(shape[0], generator=g) > 0.4) if masked else None
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    pe, me, ve = O.adam_step(p, gr, m, v, valid, lr, b1, b2, eps)
    pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
    torch.ops.gsplat.adam(pd, gr.to(DEV), md, vd, None if valid is None else valid.to(DEV), lr, b1, b2, eps)
    torch.testing.assert_close(pd.cpu(), pe, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(md.cpu(), me, rtol=2e-5, atol=5e-7)
    torch.testing.assert_close(vd.cpu(), ve, rtol=2e-5, atol=5e-7)  # fma contraction on the device
    if masked:  # masked rows are bit-identical to the inputs
        assert torch.equal(pd.cpu()[~valid], p[~valid]) and torch.equal(md.cpu()[~valid], m[~valid])
        assert torch.equal(vd.cpu()[~valid], v[~valid])


def test_selective_adam_optimizer(G, O):
    torch.manual_seed(0)
    param = torch.nn.Parameter(torch.randn(300, 3, device=DEV))
    opt = G.SelectiveAdam([param], eps=1e-8, betas=(0.9, 0.999))
    vis = torch.rand(300, device=DEV) > 0.5
    ref_p, ref_m, ref_v = param.detach().cpu().clone(), torch.zeros(300, 3), torch.zeros(300, 3)
    for _ in range(3):
        opt.zero_grad()
        (param ** 2).sum().backward()
        ref_p, ref_m, ref_v = O.adam_step(ref_p, 2 * ref_p, ref_m, ref_v, vis.cpu(), opt.param_groups[0]["lr"], 0.9, 0.999,
                                          1e-8)
        opt.step(vis)
    torch.testing.assert_close(param.detach().cpu(), ref_p, rtol=1e-5, atol=1e-6)


def test_relocation_matches_oracle_restatement_unpinned_to_the_reference(G, O):
    """`compute_relocation` against the oracle's restatement of gsplat/relocation.py:25 + Relocation.cu (the published formula
    of "3D Gaussian Splatting as Markov Chain Monte Carlo", eq. 9). PARITY UNPINNED TO THE REFERENCE: its implementation is a CUDA
    op with no Python restatement and no golden vector in its tests (tests/test_strategy.py only checks shapes), so the oracle
    cannot be replayed against reference outputs here - this test pins the kernel to the formula, not to the reference's bits."""
    st = G.MCMCStrategy().initialize_state()
    binoms = st["binoms"]
    g = torch.Generator().manual_seed(2)
    n = 400
    opac = torch.rand(n, generator=g) * 0.98 + 0.01
    scales = torch.rand(n, 3, generator=g) * 0.1 + 0.01
    ratios = torch.randint(1, 12, (n,), generator=g)
    eo, es = O.relocation(opac, scales, ratios, binoms, min_opacity=0.005)
    no, ns = G.compute_relocation(opac.to(DEV), scales.to(DEV), ratios.to(DEV), binoms.to(DEV), min_opacity=0.005)
    torch.testing.assert_close(no.cpu(), eo, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(ns.cpu(), es, rtol=2e-3, atol=1e-6)  # alternating binomial sum in fp32
    # ratio 1 keeps the Gaussian (up to the opacity clamp)
    one = torch.ones(n, dtype=torch.long)
    no1, ns1 = G.compute_relocation(opac.to(DEV), scales.to(DEV), one.to(DEV), binoms.to(DEV), min_opacity=0.0)
    torch.testing.assert_close(no1.cpu(), opac, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(ns1.cpu(), scales, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("scaler,t,k", [(0.01, 0.005, 100.0), (1.0, 0.005, 100.0), (0.25, 0.25, 8.0)])
def test_mcmc_perturb_matches_oracle(G, O, scaler, t, k):
    """Mirrors the reference's tests/test_mcmc_perturb.py (inputs, tolerances)."""
    torch.manual_seed(42)
    n = 1024
    pos, quats, sl = torch.randn(n, 3), torch.randn(n, 4), torch.randn(n, 3)
    ol, noise = torch.randn(n), torch.randn(n, 3)
    exp = O.mcmc_perturb(pos, quats, sl, ol, noise, scaler, t, k)
    out = pos.to(DEV).clone()
    torch.ops.gsplat.mcmc_perturb_positions(out, quats.to(DEV), sl.to(DEV), ol.to(DEV), noise.to(DEV), scaler, t, k)
    torch.testing.assert_close(out.cpu(), exp, atol=1e-4 if scaler >= 1.0 else 1e-5, rtol=1e-3 if scaler >= 1.0 else 1e-4)
    assert not torch.equal(out.cpu(), pos)


def _make_params(n, seed=0, with_opt=True):
    g = torch.Generator().manual_seed(seed)
    raw = {
        "means": torch.randn(n, 3, generator=g),
        "scales": torch.log(torch.rand(n, 3, generator=g) * 0.05 + 0.01),
        "quats": torch.randn(n, 4, generator=g),
        "opacities": torch.logit(torch.rand(n, generator=g) * 0.9 + 0.05),
        "sh0": torch.rand(n, 1, 3, generator=g),
    }
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(v.to(DEV)) for k, v in raw.items()})
    opts = {k: torch.optim.Adam([{"params": params[k], "lr": 1e-3, "name": k}]) for k in params.keys()}
    for k in params.keys():  # create optimizer state
        params[k].grad = torch.ones_like(params[k])
        opts[k].step()
        params[k].grad = None
    return params, opts


def _check_consistency(params, opts, n):
    for k, p in params.items():
        assert p.shape[0] == n, (k, p.shape)
        st = opts[k].state[p]
        assert opts[k].param_groups[0]["params"][0] is p
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape


def test_strategy_ops_bookkeeping(G):
    from gsplat_amd.strategy import ops

    n = 50
    params, opts = _make_params(n)
    state = {"grad2d": torch.arange(n, device=DEV, dtype=torch.float32), "count": torch.ones(n, device=DEV)}
    mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    mask[[3, 7, 11]] = True
    means0 = params["means"].detach().clone()
    ops.duplicate(params, opts, state, mask)
    _check_consistency(params, opts, n + 3)
    assert torch.equal(params["means"][n:], means0[[3, 7, 11]])
    assert opts["means"].state[params["means"]]["exp_avg"][n:].abs().max() == 0  # fresh moments for the copies
    assert torch.equal(state["grad2d"][n:], torch.tensor([3.0, 7.0, 11.0], device=DEV))
    # split: the two selected rows are replaced by 2 samples each, unselected rows first
    n1 = n + 3
    mask = torch.zeros(n1, dtype=torch.bool, device=DEV)
    mask[[0, 5]] = True
    scales0 = params["scales"].detach().clone()
    ops.split(params, opts, state, mask, revised_opacity=True)
    _check_consistency(params, opts, n1 + 2)
    torch.testing.assert_close(torch.exp(params["scales"][-4:]), (torch.exp(scales0[[0, 5]]) / 1.6).repeat(2, 1))
    # remove
    n2 = n1 + 2
    mask = torch.zeros(n2, dtype=torch.bool, device=DEV)
    mask[:10] = True
    ops.remove(params, opts, state, mask)
    _check_consistency(params, opts, n2 - 10)
    assert state["count"].shape[0] == n2 - 10
    # reset_opa
    ops.reset_opa(params, opts, state, value=0.01)
    assert torch.sigmoid(params["opacities"]).max() <= 0.01 + 1e-6
    assert opts["opacities"].state[params["opacities"]]["exp_avg"].abs().max() == 0
    # MCMC edits
    binoms = G.MCMCStrategy().initialize_state()["binoms"].to(DEV)
    n3 = params["means"].shape[0]
    with torch.no_grad():
        params["opacities"].copy_(torch.logit(torch.rand(n3, device=DEV) * 0.8 + 0.1))
        params["opacities"][:5] = -10.0  # dead
    dead = torch.sigmoid(params["opacities"]) <= 0.005
    assert int(dead.sum()) == 5
    ops.relocate(params, opts, {}, dead, binoms, min_opacity=0.005)
    _check_consistency(params, opts, n3)
    assert (torch.sigmoid(params["opacities"]) > 0.004).all()  # the dead ones now sit on live Gaussians
    ops.sample_add(params, opts, {}, 7, binoms, min_opacity=0.005)
    _check_consistency(params, opts, n3 + 7)
    m_before = params["means"].detach().clone()
    ops.inject_noise_to_position(params, opts, {}, scaler=0.5)
    assert not torch.equal(params["means"].detach(), m_before)
    assert torch.isfinite(params["means"]).all()


def _target_scene(G, n=600, W=128, H=96, seed=3):
    g = torch.Generator().manual_seed(seed)
    means = torch.stack([(torch.rand(n, generator=g) - 0.5) * 2.0, (torch.rand(n, generator=g) - 0.5) * 1.5,
                         torch.rand(n, generator=g) * 2.0 + 3.0], -1)
    sc = dict(means=means, quats=torch.randn(n, 4, generator=g), scales=torch.log(torch.rand(n, 3, generator=g) * 0.08 + 0.03),
              opacities=torch.logit(torch.rand(n, generator=g) * 0.6 + 0.3), colors=torch.rand(n, 3, generator=g))
    viewmats = torch.eye(4)[None].to(DEV)
    Ks = torch.tensor([[[120.0, 0, W / 2], [0, 120.0, H / 2], [0, 0, 1]]], device=DEV)
    return {k: v.to(DEV) for k, v in sc.items()}, viewmats, Ks, W, H


def _render(G, p, viewmats, Ks, W, H, **kw):
    return G.rasterization(p["means"], p["quats"], torch.exp(p["scales"]), torch.sigmoid(p["opacities"]), p["colors"],
                           viewmats, Ks, W, H, **kw)


@pytest.mark.parametrize("which", ["default", "default_absgrad_packed", "mcmc"])
def test_short_fit_loss_decreases(G, which):
    """rasterization() + SelectiveAdam + a densification strategy fit a target image: the loss must drop by half and the
    strategy must have edited the Gaussian set without breaking the parameter / optimizer bookkeeping."""
    torch.manual_seed(0)
    tgt, viewmats, Ks, W, H = _target_scene(G)
    with torch.no_grad():
        target, _, _ = _render(G, tgt, viewmats, Ks, W, H)
    n0 = 300
    g = torch.Generator().manual_seed(9)
    init = dict(means=torch.stack([(torch.rand(n0, generator=g) - 0.5) * 2.0, (torch.rand(n0, generator=g) - 0.5) * 1.5,
                                   torch.rand(n0, generator=g) * 2.0 + 3.0], -1),
                quats=torch.randn(n0, 4, generator=g), scales=torch.log(torch.full((n0, 3), 0.06)),
                opacities=torch.logit(torch.full((n0,), 0.3)), colors=torch.rand(n0, 3, generator=g))
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(v.to(DEV)) for k, v in init.items()})
    lrs = dict(means=2e-2, quats=1e-2, scales=2e-2, opacities=5e-2, colors=5e-2)
    opts = {k: G.SelectiveAdam([{"params": params[k], "lr": lrs[k], "name": k}], eps=1e-15, betas=(0.9, 0.999))
            for k in params.keys()}
    packed = which == "default_absgrad_packed"
    absgrad = which == "default_absgrad_packed"
    if which == "mcmc":
        strategy = G.MCMCStrategy(cap_max=600, refine_start_iter=20, refine_every=20, noise_lr=5e3)
        state = strategy.initialize_state()
    else:
        strategy = G.DefaultStrategy(refine_start_iter=20, refine_every=20, reset_every=10_000, grow_grad2d=2e-5,
                                     absgrad=absgrad, prune_opa=0.01)
        state = strategy.initialize_state(scene_scale=1.0)
    strategy.check_sanity(params, opts)
    losses, sizes = [], set()
    for step in range(121):
        colors, alphas, info = _render(G, params, viewmats, Ks, W, H, packed=packed, absgrad=absgrad)
        loss = ((colors - target) ** 2).mean()
        if which != "mcmc":
            strategy.step_pre_backward(params, opts, state, step, info)
        loss.backward()
        losses.append(float(loss))
        vis = (info["radii"] > 0).all(-1).any(0) if not packed else torch.zeros(
            len(params["means"]), dtype=torch.bool, device=DEV).index_fill_(0, info["gaussian_ids"], True)
        for o in opts.values():
            o.step(vis)
            o.zero_grad(set_to_none=True)
        if which == "mcmc":
            strategy.step_post_backward(params, opts, state, step, info, lr=lrs["means"])
        else:
            strategy.step_post_backward(params, opts, state, step, info, packed=packed)
        sizes.add(len(params["means"]))
        _check_consistency(params, opts, len(params["means"]))
    assert all(math.isfinite(x) for x in losses)
    assert min(losses[-10:]) < 0.5 * losses[0], (losses[0], losses[-10:])
    assert len(sizes) > 1, "the strategy never changed the number of Gaussians"


def test_mcmc_relocation_keeps_the_dead_rows_own_moments(G):
    """MCMC relocation (reference gsplat/strategy/ops.py relocate: `v[sampled_idxs] = 0` and nothing else): a dead row takes
    the PARAMETERS of the live row it is teleported onto but keeps its own Adam moments; the sampled live rows restart from
    zero moments; untouched rows keep everything. The one-plan refinement must reproduce that."""
    torch.manual_seed(0)
    n = 64
    g = torch.Generator().manual_seed(3)
    raw = dict(means=torch.randn(n, 3, generator=g), scales=torch.log(torch.rand(n, 3, generator=g) * 0.05 + 0.001),
               quats=torch.randn(n, 4, generator=g), opacities=torch.logit(torch.rand(n, generator=g) * 0.9 + 0.05),
               sh0=torch.randn(n, 1, 3, generator=g))
    raw["opacities"][:10] = torch.logit(torch.tensor(0.001))  # 10 dead rows (min_opacity = 0.005)
    params = torch.nn.ParameterDict({k: torch.nn.Parameter(v.to(DEV)) for k, v in raw.items()})
    opts = {k: torch.optim.Adam([p], lr=1e-3) for k, p in params.items()}
    for k, p in params.items():
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
        opts[k].step()
        p.grad = None
    before = {k: {m: opts[k].state[params[k]][m].clone() for m in ("exp_avg", "exp_avg_sq")} for k in params.keys()}
    old_means = params["means"].detach().clone()
    strat = G.MCMCStrategy(cap_max=n, min_opacity=0.005)  # cap_max = n: no stage-2 growth, relocation only
    binoms = torch.zeros((51, 51), device=DEV)
    for i in range(51):
        for j in range(i + 1):
            binoms[i, j] = math.comb(i, j)
    n_dead, n_new = strat._refine(params, opts, binoms)
    assert n_dead == 10 and n_new == 0
    for k in params.keys():
        for m in ("exp_avg", "exp_avg_sq"):
            now = opts[k].state[params[k]][m]
            assert torch.equal(now[:10], before[k][m][:10]), f"{k}.{m}: a teleported row must keep its own moments"
            live = now[10:]
            zeroed = (live.reshape(len(live), -1) == 0).all(1)
            same = (live == before[k][m][10:]).reshape(len(live), -1).all(1)
            assert bool((zeroed | same).all()), f"{k}.{m}: live rows are either sampled sources (zeroed) or untouched"
            assert bool(zeroed.any()), "the sampled sources restart from zero moments"
    assert not torch.equal(params["means"][:10].detach(), old_means[:10])  # and the dead rows carry live parameters now


def test_default_strategy_statistics_dense_equals_gathered(G):
    """The densification statistics of dense rows (masked reductions over the camera axis, nothing leaves the device) against
    the gather-then-index_add form the reference uses (gsplat/strategy/default.py:210-262) - written out here with torch."""
    from _util import make_scene

    sc, W, H = make_scene(N=5000, C=3, width=160, height=96, seed=4)
    a = {k: v.to(DEV) for k, v in sc.items()}
    params = {k: a[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "colors")}
    strategy = G.DefaultStrategy(refine_scale2d_stop_iter=10**9, verbose=False)
    state = strategy.initialize_state(scene_scale=1.0)
    for _ in range(2):  # two accumulations: the running sums really accumulate
        rc, ra, info = G.rasterization(params["means"], params["quats"], params["scales"], params["opacities"], params["colors"],
                                       a["viewmats"], a["Ks"], W, H, packed=False)
        strategy.step_pre_backward(params, {}, state, 0, info)
        rc.square().sum().backward()
        strategy._accumulate(params, state, info, packed=False)
        grad = info["means2d"].grad.clone()
        for p in params.values():
            p.grad = None
    # the reference's form, for the last gradient twice (same render both times)
    half = grad.new_tensor([0.5 * W, 0.5 * H]) * 3
    sel = (info["radii"] > 0).all(dim=-1)
    gs_ids = torch.where(sel)[1]
    norms = (grad[sel] * half).norm(dim=-1)
    want_g = torch.zeros(5000, device=DEV).index_add_(0, gs_ids, norms) * 2
    want_c = torch.zeros(5000, device=DEV).index_add_(0, gs_ids, torch.ones_like(norms)) * 2
    want_r = torch.zeros(5000, device=DEV).scatter_reduce_(0, gs_ids, info["radii"][sel].amax(-1).float() / float(max(W, H)),
                                                           reduce="amax", include_self=True)
    torch.testing.assert_close(state["grad2d"], want_g, rtol=1e-5, atol=1e-7)
    assert torch.equal(state["count"], want_c)
    torch.testing.assert_close(state["radii"], want_r, rtol=0, atol=0)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("layout", ["contiguous", "rows"])
@pytest.mark.parametrize("absgrad", [False, True])
def test_default_strategy_accumulate_is_one_launch_with_the_tensor_op_sums(C, layout, absgrad):
    """gsx_strategy_accumulate (DefaultStrategy._accumulate on GPU tensors) against the tensor-op form the same method runs on
    CPU tensors: summed gradient norms, view counts, largest relative radius - with invisible rows that hold NaN gradients
    (never read for their value), a gradient that is a column view of wider rows, several cameras."""
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd as G

    n, W, H = 5000, 640, 360
    g = torch.Generator().manual_seed(7 * C + absgrad)
    grad = torch.randn(C, n, 2, generator=g) * 1e-4
    radii = torch.randint(0, 40, (C, n, 2), generator=g, dtype=torch.int32)
    radii[torch.rand(C, n, generator=g) < 0.3] = 0
    hidden = ~(radii > 0).all(-1)
    grad[hidden] = float("nan")  # a row that is not visible must not be read for its value
    strat = G.DefaultStrategy(refine_scale2d_stop_iter=100, absgrad=absgrad, verbose=False)
    params = {"means": torch.zeros(n, 3)}

    def run(dev):
        if layout == "rows" and dev != "cpu":
            wide = torch.full((C, n, 9), float("nan"), device=dev)
            wide[..., 3:5] = grad.to(dev)
            gt = wide[..., 3:5]
            assert not gt.is_contiguous()
        else:
            gt = grad.to(dev)
        m2 = torch.zeros(C, n, 2, device=dev, requires_grad=True)
        if absgrad:
            m2.absgrad = gt
        else:
            m2.grad = gt if gt.is_contiguous() else None
            if m2.grad is None:  # a strided .grad cannot be assigned to a contiguous leaf: hand the view over as the strategy reads it
                class _G:  # noqa: N801
                    pass
                holder = _G()
                holder.grad = gt
                m2 = holder
        state = strat.initialize_state()
        state["grad2d"] = torch.rand(n, generator=torch.Generator().manual_seed(1)).to(dev)
        state["count"] = torch.ones(n, device=dev)
        state["radii"] = torch.full((n,), 0.01, device=dev)
        info = {"width": W, "height": H, "n_cameras": C, "radii": radii.to(dev), "gaussian_ids": None, strat.key_for_gradient: m2}
        strat._accumulate({"means": params["means"].to(dev)}, state, info, packed=False)
        return {k: state[k].cpu() for k in ("grad2d", "count", "radii")}

    want, got = run("cpu"), run("cuda")
    assert torch.isfinite(got["grad2d"]).all()
    torch.testing.assert_close(got["grad2d"], want["grad2d"], rtol=2e-6, atol=1e-9)
    assert torch.equal(got["count"], want["count"])
    torch.testing.assert_close(got["radii"], want["radii"], rtol=1e-6, atol=0)
