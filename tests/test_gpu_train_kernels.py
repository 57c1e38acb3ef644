"""GPU: the five training-step kernels of csrc/optim.hip through their public entry points - torch.ops.gsplat.adam,
SelectiveAdam.step (three chained steps), compute_relocation, torch.ops.gsplat.mcmc_perturb_positions and
DefaultStrategy._accumulate - against the float64 references of tests/_train_cases.py, per element, under the bounds derived
there: both Adam kernels on both sides of a 256-lane block, every base pointer 4 bytes off a 16-byte boundary, every mask shape,
relocation over the whole ratio table and down to opacities below the clamp, the SGLD step at extreme logits, the statistics kernel
at every radii pattern, and the inputs its guard must hand to the tensor-op form. tests/test_train_cases.py checks references and
bounds without a GPU. Where a result is promised unchanged (rows Adam does not select, Gaussians never seen, positions under
a zero noise weight, a running radius that is not tracked) the comparison is bit-for-bit.

Largest error / bound observed on an MI355X (a correct float32 kernel stays below 1; the CPU float32 restatements reach 0.50):
Adam 0.497 (op, 257 x 4 on the scalar kernel; SelectiveAdam chains 0.487), relocation 0.069 opacity / 0.114 scale, SGLD perturb
0.465, statistics 0.381. No bound needed a correction. The relocation corners (printed, not asserted): ratio 1 returns the scales
finite and positive at both opacities; ratio 51 returns them finite and positive at opacity 1 - 2^-24 (new opacity 0.278, kappa
4.3e4) and finite and NEGATIVE, of size 1e-8, at opacity 1.0 (new opacity at the upper clamp, kappa 5e8). A logit of +30 zeroes
the noise weight only where expf(k (1 - t)) overflows (k = 100); at (0.25, 0.25, 8) that row is held to the bound like any other.
The whole file takes 3.2 s."""
import pytest
import torch

import _train_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd
    import gsplat_amd._ops  # noqa: F401  (defines torch.ops.gsplat.*)

    return gsplat_amd


# ---- Adam ------------------------------------------------------------------------------------------------------------------
def _adam_device(cs, case):
    """The case's tensors on the device, each aligned or 4 bytes off as the case says, and the mask in its layout."""
    tensors = [tc.place(cs[k], off, DEV) for k, off in zip("pgmv", case.misalign)]
    valid = cs["valid"]
    if valid is not None:
        valid = tc.strided_bool(valid, DEV) if case.mask.endswith("strided") else valid.to(DEV)
    return tensors, valid


@pytest.mark.parametrize("name", [c.name for c in tc.ADAM_CASES])
def test_adam_op_per_element(G, name):
    case, cs = tc.ADAM_BY_NAME[name], tc.adam_case(name)
    (p, g, m, v), valid = _adam_device(cs, case)
    vec4 = tc.adam_takes_vec4(cs["D"], [t.data_ptr() for t in (p, g, m, v)])
    assert vec4 == (cs["D"] % 4 == 0 and not any(case.misalign)), "the case is not in its intended regime"
    assert all((t.data_ptr() % 16 == 4) == bool(off) for t, off in zip((p, g, m, v), case.misalign) if t.numel())
    if case.mask.endswith("strided") and cs["n_rows"] > 1:
        assert not valid.is_contiguous()
    hyper = (cs["lr"], cs["b1"], cs["b2"], cs["eps"])
    torch.ops.gsplat.adam(p, g, m, v, valid, *hyper)
    assert tc.bits_equal(g, cs["g"]), "the gradient is an input"
    r = tc.adam_check(p, m, v, (cs["p"], cs["g"], cs["m"], cs["v"]), cs["valid"], cs["never"], hyper)
    print(f"adam {name} ({'vec4' if vec4 else 'scalar'}): error / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("name", [c.name for c in tc.ADAM_CASES if any(c.misalign)])
def test_adam_scalar_and_vector_kernels_agree_on_the_same_data(G, name):
    """The same data 4 bytes off takes the scalar kernel; both kernels evaluate one expression per element, so each result must
    lie within its bound of the other's float64 reference - and rows that are not selected stay bit-identical in both."""
    case, cs = tc.ADAM_BY_NAME[name], tc.adam_case(name)
    hyper = (cs["lr"], cs["b1"], cs["b2"], cs["eps"])
    results = []
    for c in (case, case._replace(misalign=tc.ADAM_MISALIGN[0])):
        (p, g, m, v), valid = _adam_device(cs, c)
        torch.ops.gsplat.adam(p, g, m, v, valid, *hyper)
        results.append((p.cpu(), m.cpu(), v.cpu()))
    refs = tc.adam_ref(cs["p"], cs["g"], cs["m"], cs["v"], cs["valid"], *hyper)
    sel = tc._row_select(cs["valid"], cs["p"])
    for a, b, tol in zip(results[0], results[1], refs[3:]):
        assert tc.ratio(a[sel], b[sel].double(), 2.0 * tol[sel]) <= 1.0
        assert tc.bits_equal(a[~sel], b[~sel])


@pytest.mark.parametrize("shape,h", tc.ADAM_CHAINS)
def test_selective_adam_three_chained_steps(G, shape, h):
    """SelectiveAdam.step with carried state: each step against the float64 step from the kernel's own float32 state before it."""
    lr, b1, b2, eps = tc.ADAM_HYPER[h]
    n_rows, _ = tc.adam_rows_width(shape)
    p0, _, _, _, _ = tc.adam_values(shape, 300 + h)
    param = torch.nn.Parameter(p0.to(DEV))
    opt = G.SelectiveAdam([{"params": [param], "lr": lr}], eps=eps, betas=(b1, b2))
    m = v = torch.zeros(shape)
    worst = 0.0
    for step in range(tc.ADAM_CHAIN_STEPS):
        _, g, _, _, never = tc.adam_values(shape, 310 + 10 * h + step)
        valid = tc.adam_mask("random60", n_rows, 40 + step)
        before = (param.detach().cpu().clone(), g, m, v)
        param.grad = g.to(DEV)
        opt.step(valid.to(DEV))
        state = opt.state[param]
        m, v = state["exp_avg"].cpu().clone(), state["exp_avg_sq"].cpu().clone()
        # a never-seen row is one whose gradient AND moments are 0: only in the first step, where the state starts from zero
        worst = max(worst, tc.adam_check(param.detach(), m, v, before, valid, never if step == 0 else None, (lr, b1, b2, eps)))
    print(f"SelectiveAdam {shape} h{h}: error / bound {worst:.3f}")
    assert worst <= 1.0


# ---- relocation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_opacity", tc.RELOC_MIN_OPACITIES)
def test_relocation_grid_per_element(G, min_opacity):
    o, scales, ratios = tc.relocation_grid()
    dev_ratios = ratios.to(DEV)
    new_o, new_s = G.compute_relocation(o.to(DEV), scales.to(DEV), dev_ratios, tc.binoms().to(DEV), min_opacity=min_opacity)
    assert torch.equal(dev_ratios.cpu(), ratios), "ratios inside [1, n_max] are not to be changed"
    r_o, r_s, ref = tc.relocation_check(o, scales, ratios, tc.binoms(), min_opacity, new_o, new_s)
    print(f"relocation min_opacity {min_opacity}: opacity error / bound {r_o:.3f}, scale error / bound {r_s:.3f} "
          f"(largest bound {ref['rel'].max():.2e})")
    assert ref["rel"].max() < tc.RELOC_MAX_BOUND  # every row is value-checked: nothing is left out
    assert r_o <= 1.0 and r_s <= 1.0


def test_relocation_clamps_ratios_in_place(G):
    o, scales, ratios, table = tc.relocation_small()
    given = ratios.to(DEV)
    new_o, new_s = G.compute_relocation(o.to(DEV), scales.to(DEV), given, table.to(DEV), min_opacity=0.005)
    clamped = ratios.clamp(1, tc.RELOC_SMALL_N_MAX)
    assert torch.equal(given.cpu(), clamped), "the caller's ratios come back clamped to [1, n_max]"
    want_o, want_s = G.compute_relocation(o.to(DEV), scales.to(DEV), clamped.to(DEV), table.to(DEV), min_opacity=0.005)
    assert tc.bits_equal(new_o, want_o) and tc.bits_equal(new_s, want_s)
    r_o, r_s, _ = tc.relocation_check(o, scales, ratios, table, 0.005, new_o, new_s)
    print(f"relocation 12 x 12 table: opacity error / bound {r_o:.3f}, scale error / bound {r_s:.3f}")
    assert r_o <= 1.0 and r_s <= 1.0


def test_relocation_corners(G):
    """Opacity 1 - 2^-24 and 1.0: the new opacity is the upper clamp at ratio 1 and within its bound otherwise. Nothing is asserted
    about the scales (kappa > 3e4: the float32 sum is noise, here as in the reference implementation); they are printed."""
    o, scales, ratios = tc.relocation_corners()
    new_o, new_s = G.compute_relocation(o.to(DEV), scales.to(DEV), ratios.to(DEV), tc.binoms().to(DEV), min_opacity=0.005)
    r_o, _, ref = tc.relocation_check(o, scales, ratios, tc.binoms(), 0.005, new_o, new_s)
    for i in range(len(o)):
        s = new_s[i].cpu()
        print(f"relocation corner o = 1 - {1.0 - float(o[i].double()):.1e}, ratio {int(ratios[i])}: new opacity {float(new_o[i]):.9g}, "
              f"kappa {ref['kappa'][i]:.3g}, scales {s.tolist()} (finite: {bool(torch.isfinite(s).all())}, "
              f"signs {torch.sign(s).tolist()})")
    upper = torch.tensor(tc.RELOC_UPPER, dtype=torch.float32)
    assert bool((new_o.cpu()[ratios == 1] == upper).all())
    assert r_o <= 1.0


# ---- SGLD perturb ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", tc.PERTURB_PARAMS + (tc.PERTURB_ZERO_SCALE,))
@pytest.mark.parametrize("n", tc.PERTURB_ROWS)
def test_perturb_per_element(G, n, params):
    ns, t, k = params
    cs = tc.perturb_case(n)
    args = (cs["pos"], cs["quats"], cs["log_scales"], cs["logits"], cs["noise"])
    ref, tol, _ = tc.perturb_ref(*args, ns, t, k)
    dev = [a.to(DEV) for a in args]
    out = dev[0].clone()
    torch.ops.gsplat.mcmc_perturb_positions(out, *dev[1:], ns, t, k)
    for a, b in zip(dev[1:], args[1:]):
        assert tc.bits_equal(a, b), "an input was written"
    r = tc.ratio(out, ref, tol)
    print(f"perturb {n} rows, {params}: error / bound {r:.3f}")
    assert r <= 1.0
    if ns == 0.0:
        assert tc.bits_equal(out, cs["pos"])  # w = 0
    else:
        assert n < 255 or not tc.bits_equal(out, cs["pos"])
        if tc.perturb_w_is_zero(t, k):  # logit +30: density 1.0f, expf(k (1 - t)) overflows, w = 0
            assert bool(cs["hi"].any()) == (n >= 255)
            assert tc.bits_equal(out.cpu()[cs["hi"]], cs["pos"][cs["hi"]])


# ---- statistics ------------------------------------------------------------------------------------------------------------
def _accumulate_gpu(G, N, C, grad_view, radii, state, absgrad, track):
    strat = G.DefaultStrategy(refine_scale2d_stop_iter=100 if track else 0, absgrad=absgrad, verbose=False)
    assert ("radii" in strat.initialize_state()) == track
    strat._accumulate({"means": torch.zeros(N, 3, device=DEV)}, state, tc.accumulate_info(grad_view, radii, C, absgrad), packed=False)
    return state


@pytest.mark.parametrize("name", [c.name for c in tc.ACC_CASES])
def test_accumulate_per_element(G, name):
    case = tc.ACC_BY_NAME[name]
    inp = tc.accumulate_inputs(case.N, case.C)
    start = inp["state"]
    ref = tc.accumulate_ref(inp["grad"], inp["radii"], start if case.track else {k: start[k] for k in ("grad2d", "count")},
                            *tc.accumulate_scalars(case.C))
    grad_view = tc.accumulate_layout(inp["grad"], case.layout, DEV)
    radii = inp["radii"].to(DEV)
    got = _accumulate_gpu(G, case.N, case.C, grad_view, radii, {k: v.to(DEV).clone() for k, v in start.items()}, case.absgrad,
                          case.track)
    assert tc.bits_equal(grad_view.contiguous(), inp["grad"]) and torch.equal(radii.cpu(), inp["radii"])
    r = tc.accumulate_check(got, ref)
    print(f"accumulate {name}: error / bound {r:.3f}")
    assert r <= 1.0
    if not case.track:
        assert tc.bits_equal(got["radii"], start["radii"]), "the running radius is not tracked and must stay untouched"


@pytest.mark.parametrize("which", ["radii-4-bytes-off", "state-of-one-element", "row-stride-1"])
def test_accumulate_guard_hands_over_to_the_tensor_op_form(G, which):
    """Inputs the one-launch kernel cannot take - radii that are not 8-byte aligned (it reads a pair as one int2), a state tensor that
    does not have N elements (it indexes it with the Gaussian's row), gradient rows closer than two floats - must give the
    reference's sums through the tensor-op form, not an error from the C side and not an access outside a tensor."""
    N, C = 257, 2
    inp = tc.accumulate_inputs(N, C, finite=(which == "row-stride-1"))
    start = {k: v.clone() for k, v in inp["state"].items()}
    grad, radii = inp["grad"], inp["radii"].to(DEV)
    grad_view = grad.to(DEV)
    if which == "radii-4-bytes-off":
        radii = tc.place(inp["radii"], True, DEV)
        assert radii.is_contiguous() and radii.data_ptr() % 8 == 4
    elif which == "state-of-one-element":
        start["radii"] = torch.tensor([0.02])  # broadcasts in the tensor-op form
    else:
        base = torch.randn(C * N + 1, generator=torch.Generator().manual_seed(5)) * 1e-4
        grad = base.as_strided((C, N, 2), (N, 1, 1))
        grad_view = base.to(DEV).as_strided((C, N, 2), (N, 1, 1))
        assert grad_view.stride() == (N, 1, 1)
    ref = tc.accumulate_ref(grad, inp["radii"], start, *tc.accumulate_scalars(C))
    got = _accumulate_gpu(G, N, C, grad_view, radii, {k: v.to(DEV).clone() for k, v in start.items()}, False, True)
    assert got["radii"].shape == (N,)
    r = tc.accumulate_check(got, ref)
    print(f"accumulate guard, {which}: error / bound {r:.3f}")
    assert r <= 1.0
