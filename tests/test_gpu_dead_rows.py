"""Rows without a cotangent in the per-Gaussian backward kernels (SH colours, EWA projection).

A row is dead for a kernel when every cotangent the kernel consumes for it compares equal to zero (-0.0 is zero, NaN is
live). The SH backward tests liveness per row: it reads nothing of a dead Gaussian and writes +0 rows. The projection backward
computes a dead row like any other (its products with zero are zeros of either sign). Both kernels are called through the
C-ABI with NaN-filled outputs, so a row a kernel forgot to write shows; expected values are the autograd of the oracle's
torch-CPU ops at the tolerances tests/test_gpu_ops.py uses for the same ops; dead rows are compared with == 0 exactly.

The projection tests guard UNCHANGED behaviour: project_bwd_kernel has no liveness test (two forms of one were measured
slower, profiles/r12_dead_rows.md), and these cases pin the kernel as it is for a later attempt."""
import pytest
import torch

from _util import assert_grad_close, make_scene

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SIZES = [64 * 3 + 5, 256 * 2 + 1]  # a partial last wave; a partial last workgroup


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd

    return gsplat_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle

    return oracle


def cpu(t):
    return None if t is None else t.detach().cpu()


def row_patterns(N, seed=0):
    """name -> bool [N], True = the row gets a cotangent."""
    g = torch.Generator().manual_seed(seed)
    groups = torch.rand(N, generator=g) > 0.3
    groups[:192] = False  # group 0: lane 0 only; group 1: nothing; group 2: lane 63 only
    groups[0] = groups[191] = True
    return {"all": torch.ones(N, dtype=torch.bool), "none": torch.zeros(N, dtype=torch.bool),
            "alternate": torch.arange(N) % 2 == 0, "groups": groups}


def assert_zero(t, rows, name, plus=False):
    t = cpu(t)[rows]
    assert (t == 0).all(), f"{name}: a dead row is not zero"
    assert not (plus and torch.signbit(t).any()), f"{name}: a dead row holds -0.0"


# ---- SH backward --------------------------------------------------------------------------------------------------------
def sh_inputs(deg, N, C, seed):
    sc, _, _ = make_scene(N=N, C=C, seed=seed)
    K = 25 if deg == 4 else 16  # 75 floats per row: every thread streams its own; 48: wave-cooperative tiles
    g = torch.Generator().manual_seed(seed + 100)
    return sc["means"], sc["viewmats"], torch.randn(N, K, 3, generator=g) * 0.3


def sh_bwd_gpu(deg, means, viewmats, coeffs, vc, radii=None, post=None, strided=False, want_means=True):
    """gsx_sh_bwd on dense rows; vc [C, N, 3] on the CPU. Returns (v_coeffs, v_means) - NaN wherever nothing was written."""
    from gsplat_amd import _cabi

    (C, N), K = vc.shape[:2], coeffs.shape[1]
    dev = lambda t: None if t is None else t.to(DEV).contiguous()  # noqa: E731
    means, viewmats, coeffs, radii, post = dev(means), dev(viewmats), dev(coeffs), dev(radii), dev(post)
    if strided:  # the colour columns of [R, 9] gradient rows
        rows = torch.randn(C * N, 9, device=DEV)
        rows[:, 5:8] = vc.reshape(-1, 3).to(DEV)
        view, stride = rows[:, 5:8], 9
    else:
        view, stride = vc.reshape(-1, 3).to(DEV).contiguous(), 3
    v_coeffs = torch.full((N, K, 3), NAN, device=DEV)
    v_means = torch.full((N, 3), NAN, device=DEV) if want_means else None
    _cabi.call("gsx_sh_bwd", deg, _cabi.ptr(means), _cabi.ptr(viewmats), _cabi.ptr(coeffs), None, None, None, None,
               1, C, N, -1, 1, K, 3, _cabi.ptr(radii), _cabi.ptr(post), _cabi.ptr_strided(view), stride, None,
               _cabi.ptr(v_coeffs), _cabi.ptr(v_means), None)
    torch.cuda.synchronize()
    return v_coeffs, v_means


def sh_bwd_ref(O, deg, means, viewmats, coeffs, vc_eff):
    """Autograd of the oracle's SH colours with the effective cotangent vc_eff [C, N, 3]."""
    mo, co = means.clone().requires_grad_(True), coeffs.clone().requires_grad_(True)
    col = O.spherical_harmonics(deg, mo[None], viewmats[None], co)[0]
    (col * vc_eff).sum().backward()
    return co.grad, (mo.grad if mo.grad is not None else torch.zeros_like(means))


def check_sh(deg, out, ref, dead, name):
    (v_coeffs, v_means), (r_coeffs, r_means) = out, ref
    assert not torch.isnan(v_coeffs).any(), f"{name}: a v_coeffs row was not written"
    assert_grad_close(cpu(v_coeffs), r_coeffs, rel=1e-5, name=f"{name} v_coeffs")
    assert_zero(v_coeffs, dead, f"{name} v_coeffs", plus=True)
    if v_means is not None:
        assert not torch.isnan(v_means).any(), f"{name}: a v_means row was not written"
        if deg > 0:
            assert_grad_close(cpu(v_means), r_means, rel=1e-4, name=f"{name} v_means")
        else:
            assert cpu(v_means).abs().max() < 1e-6
        assert_zero(v_means, dead, f"{name} v_means", plus=True)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_sh_bwd_row_patterns(O, G, deg, N):
    means, viewmats, coeffs = sh_inputs(deg, N, 1, seed=deg)
    g = torch.Generator().manual_seed(7)
    w = torch.randn(1, N, 3, generator=g)
    for pat, live in row_patterns(N).items():
        vc = w * live[None, :, None]
        ref = sh_bwd_ref(O, deg, means, viewmats, coeffs, vc)
        for strided in (False, True):
            for want_means in (True, False):
                out = sh_bwd_gpu(deg, means, viewmats, coeffs, vc, strided=strided, want_means=want_means)
                check_sh(deg, out, ref, ~live, f"deg {deg} N {N} {pat} strided={strided} means={want_means}")


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("deg", [3, 4])
def test_sh_bwd_dead_row_definitions(O, G, deg, strided):
    N = SIZES[0]
    means, viewmats, coeffs = sh_inputs(deg, N, 1, seed=11)
    g = torch.Generator().manual_seed(8)
    vc = torch.randn(1, N, 3, generator=g)
    post = torch.rand(1, N, 3, generator=g) + 0.1  # the forward's clamped colours: > 0 = the clamp let the gradient through
    radii = torch.full((1, N, 2), 3, dtype=torch.int32)
    idx = torch.arange(N)
    cut = idx % 7 == 1         # live by value, every channel cut by the clamp
    cut_one = idx % 7 == 2     # one channel cut: the row stays live
    off = idx % 7 == 3         # radii <= 0 with a non-zero cotangent
    neg_zero = idx % 7 == 4    # -0.0 in every channel
    post[0, cut] = 0.0
    post[0, cut_one, 1] = 0.0
    radii[0, off, 0] = 0
    radii[0, off & (idx % 2 == 0), 1] = -1
    vc[0, neg_zero] = -0.0
    vc_eff = torch.where(post > 0, vc, torch.zeros(())) * (radii > 0).all(-1, keepdim=True)
    dead = cut | off | neg_zero
    assert (vc_eff[0, dead] == 0).all() and (vc_eff[0, ~dead] != 0).any(-1).all()
    ref = sh_bwd_ref(O, deg, means, viewmats, coeffs, vc_eff)
    out = sh_bwd_gpu(deg, means, viewmats, coeffs, vc, radii=radii, post=post, strided=strided)
    check_sh(deg, out, ref, dead, f"deg {deg} definitions")
    # a NaN cotangent is live and propagates into its own Gaussian's rows, and into nothing else
    nan_row = 5
    assert not dead[nan_row]
    vc_nan = vc.clone()
    vc_nan[0, nan_row, 2] = NAN
    v_coeffs, v_means = sh_bwd_gpu(deg, means, viewmats, coeffs, vc_nan, radii=radii, post=post, strided=strided)
    nb = (deg + 1) ** 2
    assert torch.isnan(v_coeffs[nan_row, :nb, 2]).all() and torch.isnan(v_means[nan_row]).all()
    keep = idx != nan_row
    assert torch.equal(v_coeffs[keep], out[0][keep]) and torch.equal(v_means[keep], out[1][keep])
    # ... unless the clamp cuts it
    post_cut = post.clone()
    post_cut[0, nan_row, 2] = 0.0
    v_coeffs, v_means = sh_bwd_gpu(deg, means, viewmats, coeffs, vc_nan, radii=radii, post=post_cut, strided=strided)
    assert not torch.isnan(v_coeffs).any() and not torch.isnan(v_means).any()


@pytest.mark.parametrize("want_means", [True, False])
@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_sh_bwd_two_images(O, G, deg, want_means):
    """Several images per Gaussian: live in the second image only, in the first only, in both, in neither."""
    N = SIZES[1]
    means, viewmats, coeffs = sh_inputs(deg, N, 2, seed=20 + deg)
    g = torch.Generator().manual_seed(9)
    vc = torch.randn(2, N, 3, generator=g)
    idx = torch.arange(N)
    live = torch.stack([(idx % 4 == 1) | (idx % 4 == 2), (idx % 4 == 0) | (idx % 4 == 2)])
    live[:, 64:128] = False
    live[1, 64] = True  # one row of a whole group, in the second image
    vc = vc * live[..., None]
    ref = sh_bwd_ref(O, deg, means, viewmats, coeffs, vc)
    for strided in (False, True):
        out = sh_bwd_gpu(deg, means, viewmats, coeffs, vc, strided=strided, want_means=want_means)
        check_sh(deg, out, ref, ~live.any(0), f"deg {deg} two images strided={strided} means={want_means}")


# ---- projection backward ------------------------------------------------------------------------------------------------
W, H = 200, 150


class ProjCase:
    """One scene projected by the GPU forward and by the oracle (whose autograd graph is kept for every pattern)."""

    def __init__(self, G, O, N, C, use_covars):
        sc, _, _ = make_scene(N=N, C=C, width=W, height=H, seed=3)
        self.N, self.C, self.use_covars, self.sc = N, C, use_covars, sc
        a = {k: v.to(DEV) for k, v in sc.items()}
        self.covars_g = G.quat_scale_to_covar_preci(a["quats"], a["scales"], True, False, True)[0].contiguous() if use_covars else None
        self.rad, _, _, self.con, self.comp = G.fully_fused_projection(
            a["means"], self.covars_g, None if use_covars else a["quats"], None if use_covars else a["scales"], a["viewmats"],
            a["Ks"], W, H, eps2d=0.3, near_plane=0.01, far_plane=1e10, radius_clip=0.0, packed=False, calc_compensations=True,
            camera_model="pinhole")
        self.a = a
        lv = {k: sc[k].clone().requires_grad_(True) for k in ("means", "quats", "scales", "viewmats")}
        if use_covars:
            lv["covars"] = O.quat_scale_to_covar_preci(sc["quats"], sc["scales"], True, False, True)[0].detach().requires_grad_(True)
        out = O.fully_fused_projection(lv["means"][None], lv["covars"][None] if use_covars else None,
                                       None if use_covars else lv["quats"][None], None if use_covars else lv["scales"][None],
                                       lv["viewmats"][None], sc["Ks"][None], W, H, 0.3, 0.01, 1e10, 0.0, True, "pinhole", None)
        self.rad_o, self.m2_o, self.d_o, self.con_o, self.comp_o = [o[0] for o in out]
        self.leaves = lv
        self.names = ("means", "covars", "viewmats") if use_covars else ("means", "quats", "scales", "viewmats")
        self.valid = (cpu(self.rad) > 0).all(-1) & (self.rad_o > 0).all(-1)  # [C, N]
        assert self.valid.float().mean() > 0.3
        g = torch.Generator().manual_seed(5)
        self.w = dict(m2=torch.randn(C, N, 2, generator=g), d=torch.randn(C, N, generator=g),
                      con=torch.randn(C, N, 3, generator=g) * 1e-2, comp=torch.randn(C, N, generator=g),
                      op=torch.randn(C, N, generator=g))

    def cotangents(self, live, only=None):
        """The random cotangents on the rows `live` [C, N] (and visible in both forwards), zero elsewhere; `only` [C, N] of
        names keeps a single cotangent per row."""
        m = (live & self.valid).float()
        out = {k: v * (m[..., None] if v.dim() == 3 else m) for k, v in self.w.items()}
        if only is not None:
            for k, v in out.items():
                sel = torch.tensor([[o == k for o in row] for row in only]).float()
                out[k] = v * (sel[..., None] if v.dim() == 3 else sel)
        return out

    def ref(self, cot):
        loss = ((self.m2_o * cot["m2"]).sum() + (self.d_o * cot["d"]).sum() + (self.con_o * cot["con"]).sum()
                + (self.comp_o * cot["comp"]).sum())
        if not loss.requires_grad or all((cot[k] == 0).all() for k in ("m2", "d", "con", "comp")):
            grads = [torch.zeros_like(self.leaves[k]) for k in self.names]
        else:
            grads = torch.autograd.grad(loss, [self.leaves[k] for k in self.names], retain_graph=True, allow_unused=True)
            grads = [torch.zeros_like(self.leaves[k]) if g is None else g for k, g in zip(self.names, grads)]
        out = dict(zip(self.names, grads))
        out["opacities"] = cot["op"].sum(0)
        return out

    def gpu(self, cot, strided, pose):
        from gsplat_amd import _cabi

        N, C, a = self.N, self.C, self.a
        if strided:  # [R, 9] gradient rows: means2d, conics, colours, opacity
            rows = torch.randn(C * N, 9, device=DEV)
            rows[:, 0:2], rows[:, 2:5], rows[:, 8] = (cot["m2"].reshape(-1, 2).to(DEV), cot["con"].reshape(-1, 3).to(DEV),
                                                      cot["op"].reshape(-1).to(DEV))
            m2, con, op, strides = rows[:, 0:2], rows[:, 2:5], rows[:, 8], (9, 9, 9)
        else:
            m2, con, op, strides = cot["m2"].to(DEV).contiguous(), cot["con"].to(DEV).contiguous(), cot["op"].to(DEV).contiguous(), (2, 3, 1)
        v_d, v_comp = cot["d"].to(DEV).contiguous(), cot["comp"].to(DEV).contiguous()
        full = lambda *s: torch.full(s, NAN, device=DEV)  # noqa: E731
        out = dict(means=full(N, 3), opacities=full(N), viewmats=torch.zeros(C, 4, 4, device=DEV) if pose else None)
        if self.use_covars:
            out["covars"] = full(N, 6)
        else:
            out["quats"], out["scales"] = full(N, 4), full(N, 3)
        p = _cabi.ptr
        _cabi.call("gsx_project_ewa_bwd_opac", p(a["means"]), p(self.covars_g), None if self.use_covars else p(a["quats"]),
                   None if self.use_covars else p(a["scales"]), p(a["viewmats"]), p(a["Ks"]), 1, C, N, W, H, 0.3, 0,
                   p(self.rad.contiguous()), p(self.con.contiguous()), p(self.comp.contiguous()), _cabi.ptr_strided(m2),
                   strides[0], p(v_d), _cabi.ptr_strided(con), strides[1], p(v_comp), _cabi.ptr_strided(op), strides[2],
                   p(out["means"]), p(out.get("covars")), p(out.get("quats")), p(out.get("scales")), p(out["viewmats"]),
                   p(out["opacities"]))
        torch.cuda.synchronize()
        return out

    def check(self, cot, strided, pose, name):
        ref, out = self.ref(cot), self.gpu(cot, strided, pose)
        geometry_dead = ~((cot["m2"] != 0).any(-1) | (cot["con"] != 0).any(-1) | (cot["d"] != 0) | (cot["comp"] != 0)).any(0)
        for k in self.names:
            if k == "viewmats":
                if pose:
                    assert_grad_close(cpu(out[k])[:, :3], ref[k][:, :3], rel=2e-3, name=f"{name} v_viewmats")
                continue
            assert not torch.isnan(out[k]).any(), f"{name}: a v_{k} row was not written"
            assert_grad_close(cpu(out[k]), ref[k], rel=2e-3, name=f"{name} v_{k}")
            assert_zero(out[k], geometry_dead, f"{name} v_{k}")
        assert not torch.isnan(out["opacities"]).any(), f"{name}: a v_opacities row was not written"
        # a sum of at most three fp32 terms below 8 in magnitude, in either order: two roundings of at most ulp(8) / 2 each
        torch.testing.assert_close(cpu(out["opacities"]), ref["opacities"], rtol=0, atol=1e-6)
        return out


@pytest.fixture(scope="module")
def proj_cases(G, O):
    cache = {}

    def get(N, C, use_covars):
        key = (N, C, use_covars)
        if key not in cache:
            cache[key] = ProjCase(G, O, N, C, use_covars)
        return cache[key]

    return get


@pytest.mark.parametrize("use_covars", [False, True])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("N", SIZES)
def test_projection_bwd_row_patterns(proj_cases, N, C, use_covars):
    case = proj_cases(N, C, use_covars)
    for pat, live in row_patterns(N).items():
        live = live[None].expand(C, N).clone()
        if C > 1 and pat == "alternate":  # some Gaussians live in the last view only, some in the first only
            live[:-1, torch.arange(N) % 4 == 0] = False
            live[1:, torch.arange(N) % 4 == 2] = False
        cot = case.cotangents(live)
        for strided in (False, True):
            case.check(cot, strided, pose=False, name=f"N {N} C {C} covars={use_covars} {pat} strided={strided}")


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("N", SIZES)
def test_projection_bwd_viewmats(proj_cases, N, C):
    """The wave-level pose reduction with half of the rows dead, with all of them dead, and with whole groups dead."""
    case = proj_cases(N, C, False)
    pats = row_patterns(N)
    for pat in ("alternate", "none", "groups"):
        cot = case.cotangents(pats[pat][None].expand(C, N))
        out = case.check(cot, strided=True, pose=True, name=f"N {N} C {C} pose {pat}")
        assert cpu(out["viewmats"])[:, 3].abs().max() == 0
        if pat == "none":
            assert (out["viewmats"] == 0).all()


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("C", [1, 3])
def test_projection_bwd_single_cotangent(proj_cases, C, strided):
    """Rows whose only non-zero cotangent is v_depths, v_compensations or the per-view opacity column."""
    N = SIZES[0]
    case = proj_cases(N, C, False)
    kinds = ("d", "comp", "op", "none")
    only = [[kinds[g % 4] for g in range(N)] for _ in range(C)]
    cot = case.cotangents(torch.ones(C, N, dtype=torch.bool), only=only)
    for k in ("d", "comp", "op"):
        assert (cot[k] != 0).any()
    out = case.check(cot, strided, pose=False, name=f"C {C} single cotangent strided={strided}")
    depth_rows = torch.tensor([o == "d" for o in only[0]]) & case.valid.all(0)
    comp_rows = torch.tensor([o == "comp" for o in only[0]]) & case.valid.all(0)
    assert (cpu(out["means"])[depth_rows] != 0).any(-1).all(), "a depth-only row lost its gradient"
    assert (cpu(out["means"])[comp_rows] != 0).any(-1).all(), "a compensation-only row lost its gradient"


def test_projection_bwd_negative_zero_and_nan(proj_cases):
    N = SIZES[0]
    case = proj_cases(N, 1, False)
    live = torch.arange(N)[None] % 2 == 0
    cot = case.cotangents(live)
    base = case.check(cot, strided=True, pose=False, name="base")
    for k in cot:  # -0.0 everywhere a row is dead
        cot[k] = torch.where(cot[k] == 0, torch.full((), -0.0), cot[k])
    out = case.gpu(cot, strided=True, pose=False)
    dead = ~(live & case.valid)[0]
    for k in ("means", "quats", "scales"):
        assert_zero(out[k], dead, f"-0.0 v_{k}")
        assert torch.equal(out[k], base[k])
    row = int(torch.nonzero(dead & case.valid[0])[0])  # a visible row without a cotangent
    cot["con"][0, row, 1] = NAN
    out = case.gpu(cot, strided=True, pose=False)
    assert torch.isnan(out["scales"][row]).any() and torch.isnan(out["quats"][row]).any()
    keep = torch.arange(N) != row
    for k in ("means", "quats", "scales"):
        assert torch.equal(out[k][keep], base[k][keep])


def dirty_allocator(nbytes=8 << 20):
    """A freed NaN block larger than the outputs: a torch.empty output some path forgot to write then shows as NaN."""
    torch.full((nbytes // 4,), NAN, device=DEV)
    torch.cuda.synchronize()


@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("pat", ["alternate", "none", "groups"])
def test_sh_bwd_packed_rows(G, O, gathered, pat):
    """Packed rows: gathered coefficients (one thread per row, sh3_bwd_packed_kernel) and coefficients read through gaussian_ids
    (the Gaussian-major walk through a row map), with rows whose cotangent is zero."""
    from gsplat_amd import _ops

    N, C = SIZES[1], 2
    means, viewmats, coeffs = sh_inputs(3, N, C, seed=40)
    g = torch.Generator().manual_seed(4)
    vis = torch.rand(C, N, generator=g) > 0.4
    live = row_patterns(N)[pat][None].expand(C, N) & vis
    if pat == "alternate":
        live = live.clone()
        live[0, torch.arange(N) % 4 == 0] = False  # some Gaussians live in the second image only
    ci, gi = torch.where(vis)
    vc = torch.randn(C, N, 3, generator=g) * live[..., None]
    r_coeffs, r_means = sh_bwd_ref(O, 3, means, viewmats, coeffs, vc)
    dev_coeffs = coeffs.to(DEV)
    dirty_allocator()
    v_coeffs, v_means, _, _ = _ops.spherical_harmonics_bwd(
        3, means.to(DEV), viewmats.to(DEV), dev_coeffs[gi.to(DEV)] if gathered else dev_coeffs, None,
        torch.zeros_like(ci).to(DEV), ci.to(DEV), gi.to(DEV), None, vc[vis].to(DEV), True, False, False, _gathered=gathered)
    if gathered:  # [nnz, K, 3] rows -> per Gaussian
        assert not torch.isnan(v_coeffs).any()
        assert (cpu(v_coeffs)[~live[vis]] == 0).all()
        v_coeffs = torch.zeros(N, 16, 3).index_add_(0, gi, cpu(v_coeffs))
    assert not torch.isnan(v_coeffs).any() and not torch.isnan(v_means).any()
    assert_grad_close(cpu(v_coeffs), r_coeffs, rel=1e-5, name="packed v_coeffs")
    assert_grad_close(cpu(v_means), r_means, rel=1e-4, name="packed v_means")
    dead = ~live.any(0)
    assert_zero(v_coeffs, dead, "packed v_coeffs")
    assert_zero(v_means, dead, "packed v_means")
