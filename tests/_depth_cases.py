"""Case builders, float64 references and error bounds for the depth-supervision losses of csrc/depth_loss.hip - depth_l1_loss,
binocular_disparity_l1, pearson_depth_loss (gsplat/losses.py:209-320) and sampled_depth_l1_loss (the trainers' depth_loss=True
block, examples/simple_trainer.py:962-980). Shared by tests/test_depth_losses.py (CPU: the torch compositions against the pinned
reference, float32 restatements inside half of every bound, one wrong restatement per family outside) and
tests/test_gpu_depth_losses.py (GPU: the kernels against the same references and bounds). Everything here is seeded torch on
the CPU; the only use of the native library is gsx_depth_blocks(n), a host function, to find where the launch changes regime.

Element counts (dense losses): 0, 1, 2, 3, 63, 64, 65, then SPAN - 1, SPAN, SPAN + 1 with SPAN the largest count one workgroup
covers (gsx_depth_blocks(n) == 1) and CAP_N + 1 with CAP_N = cap * SPAN the most the capped grid covers at one span per
workgroup - one more and a workgroup takes more than one span. With the library as built: SPAN = 1024, cap = 1024 workgroups,
CAP_N + 1 = 1048577.

Value families: d3 / d20 / d100 = depths 3 +- 1, 20 +- 0.5, 100 +- 0.05 with gt = pred + noise (correlated; the noise has a floor,
so no disparity pair ties and sign(1/p - 1/g) is the same in float32 and float64); const = pred exactly 3 (the Pearson clamp
is active); anti = gt = 6 - pred + noise (loss near 2); zeros = d3 with zeros and negatives on both sides (disparity modes);
tiny = d3 with |values| of 5e-8 <= eps on both sides (binocular mode).
Masks: none, bool, uint8, float32, a broadcast [B, 1, W] mask, all zeros, all ones, exactly one / two elements left, and skip0 - a
mask that drops element 0, where pred holds 1e30 and gt NaN: values under the mask are not read.

References. Every reference takes the float32 inputs as given and promotes them to float64; SCALE = 1.75 and the coordinates
are exact in float32. `ref_dense` / `ref_sampled` restate the reference's formulas (boolean indexing, centred Pearson sums,
normalise-then-grid_sample), with the one departure this project defines: the gradient of where(d > 0, 1 / d, 0) is 0 at
d <= 0. Loss values are the reference's.

Bounds. EPS = 2^-24.
  * disparity gradients are elementwise, sign(d) (-1 / p^2) scale / count: 16 EPS |grad_i| per element (1 / p, its square, the
    scale / count factor and two products round in a float32 evaluation: at most 6 EPS, seen at most 0.24 of the bound); an
    element without gradient must be exactly 0.
  * reduced scalars (every loss) and the gradients that carry reduced quantities (Pearson, sampled): per family twice the
    largest error of the restated reference evaluated in float32 against its float64 evaluation over that family's cases -
    absolute for a loss, relative to max |grad| of the case for a gradient (`family_bounds`).
    Values that result (a float32 sum's error depends on the CPU's summation order: up to 2 x between CPUs), loss / gradient
    (the disparity gradients use the per-element bound): pearson d3 3.6e-07 / 1.1e-05,
    d20 2.4e-07 / 1.8e-06, d100 1.6e-07 / 1.0e-06, const 0 (the loss is exactly 1) / 1.3e-07, anti 4.1e-07 / 7.5e-06;
    l1 d3 4.0e-08, d20 2.4e-10, d100 9.7e-11, zeros 4.6e-08; bin d3 3.9e-08, d20 1.8e-10, d100 6.4e-11, zeros 5.6e-08,
    tiny 1.1e-08; sampled pos 4.6e-08 / 2.8e-06, defined 3.7e-08 / 4.3e-06.
Pearson cases with fewer than three selected elements are degenerate (r = +-1, analytic gradient 0): loss and finiteness only."""
import functools
import math
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
SCALE = 1.75   # scene_scale of the l1 and sampled cases: exact in float32
BIN_EPS = 1e-7  # binocular_disparity_l1's default threshold
ELEMENT_TOL = 16 * EPS


@functools.lru_cache(maxsize=None)
def launch_edges():
    """(SPAN, cap, CAP_N) probed from gsx_depth_blocks on the CPU: the largest count of one workgroup, the block cap, the
    largest count the capped grid covers with one span per workgroup."""
    from gsplat_amd import _cabi

    blocks = _cabi._lib.gsx_depth_blocks
    cap = int(blocks(1 << 40))

    def last_below(target, hi):  # largest n with blocks(n) < target (blocks is monotone)
        lo = 0
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if blocks(mid) < target else (lo, mid - 1)
        return lo

    span = last_below(2, 1 << 40)
    assert last_below(cap, 1 << 40) + 1 == (cap - 1) * span + 1  # one span per workgroup up to cap * span elements
    return span, cap, cap * span


def dense_counts():
    span, _, cap_n = launch_edges()
    return (0, 1, 2, 3, 63, 64, 65, span - 1, span, span + 1, cap_n + 1)


DenseCase = namedtuple("DenseCase", "name loss shape family mask layout")
SHAPE3 = (2, 7, 9)       # the mask and layout cases: 126 elements
MASKS3 = ("bool", "u8", "f32", "bcast", "zeros", "ones", "one", "two", "skip0")


@functools.lru_cache(maxsize=None)
def dense_cases():
    span, _, cap_n = launch_edges()
    out = []

    def add(loss, shape, family, mask="none", layout="contiguous"):
        shape = tuple(shape)
        out.append(DenseCase(f"{loss}-{'x'.join(map(str, shape))}-{family}-{mask}-{layout}", loss, shape, family, mask, layout))

    for loss in ("l1", "bin", "pearson"):
        for n in dense_counts():
            add(loss, (n,), "d3")
            if loss != "l1":
                add(loss, (n,), "d3", "bool")
        for n in (65, span + 1):
            for family in ("d20", "d100") + (("const", "anti") if loss == "pearson" else ("zeros",)):
                add(loss, (n,), family)
            if loss == "bin":
                add(loss, (n,), "tiny")
        if loss != "l1":
            for mask in MASKS3:
                add(loss, SHAPE3, "d20" if loss == "pearson" else "zeros", mask)
            add(loss, SHAPE3 + (1,), "d3", "u8", "channel3")
        add(loss, SHAPE3 + (1,), "d3", "none", "channel3")
    add("pearson", (cap_n + 1,), "d100")
    add("pearson", (cap_n + 1,), "const")
    return tuple(out)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _values(family, n, g):
    """(pred, gt) float32 [n]."""
    u = torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1
    noise = torch.randn(n, generator=g, dtype=torch.float64)
    noise = torch.sign(noise) * (0.2 + noise.abs())  # |noise| >= 0.2: no pair ties
    centre, spread = {"d20": (20.0, 0.5), "d100": (100.0, 0.05)}.get(family, (3.0, 1.0))
    pred = centre + spread * u
    gt = pred + 0.1 * spread * noise
    if family == "const":
        pred = torch.full((n,), 3.0, dtype=torch.float64)
        gt = 3.0 + 0.25 * noise
    elif family == "anti":
        gt = 2 * centre - pred + 0.02 * spread * noise
    elif family in ("zeros", "tiny"):
        kind_p = torch.randint(0, 10, (n,), generator=g)
        kind_g = torch.randint(0, 10, (n,), generator=g)
        special = 0.0 if family == "zeros" else 5e-8
        pred = torch.where(kind_p < 2, torch.full_like(pred, special), torch.where(kind_p == 2, -pred, pred))
        gt = torch.where(kind_g == 0, torch.full_like(gt, -special), torch.where(kind_g == 1, -gt, gt))
    return pred.float(), gt.float()


def _mask(kind, shape, g):
    n = math.prod(shape)
    if kind == "none":
        return None
    if kind == "bool":
        return torch.rand(shape, generator=g) > 0.3
    if kind == "u8":
        return (torch.rand(shape, generator=g) > 0.3).to(torch.uint8) * torch.randint(1, 8, shape, generator=g).to(torch.uint8)
    if kind == "f32":
        return torch.randint(0, 3, shape, generator=g).float() * 0.5
    if kind == "bcast":  # [B, 1, W]-style
        return torch.rand((shape[0], 1) + tuple(shape[2:]), generator=g) > 0.3
    if kind == "skip0":  # element 0 is dropped; dense_inputs puts what must not be read there
        m = torch.rand(shape, generator=g) > 0.3
        m.view(-1)[0] = False
        return m
    if kind == "zeros":
        return torch.zeros(shape)
    if kind == "ones":
        return torch.ones(shape, dtype=torch.bool)
    m = torch.zeros(n, dtype=torch.uint8)
    m[torch.randperm(n, generator=g)[:{"one": 1, "two": 2}[kind]]] = 1
    return m.reshape(shape)


@functools.lru_cache(maxsize=None)
def dense_inputs(case):
    """(pred, gt, mask) on the CPU, contiguous float32 (mask: its own dtype or None). Never modified by a test."""
    g = _gen(case.name)
    pred, gt = _values(case.family, math.prod(case.shape), g)
    if case.mask == "skip0":  # an outlier and a NaN under the mask: neither may be read, nor cost the sums their precision
        pred[0], gt[0] = 1e30, float("nan")
    return pred.reshape(case.shape), gt.reshape(case.shape), _mask(case.mask, case.shape, g)


def place_dense(case, device):
    """(pred, gt, mask) on `device` in the case's layout: contiguous, or pred as channel 3 of a [C, H, W, 4] tensor whose
    other channels hold NaN (the depth channel of an RGB+ED render; the NaNs must not be read)."""
    pred, gt, mask = dense_inputs(case)
    gt = gt.to(device)
    mask = None if mask is None else mask.to(device)
    if case.layout == "contiguous":
        return pred.to(device).clone(), gt, mask
    wide = torch.full(case.shape[:3] + (4,), float("nan"), device=device)
    wide[..., 3:4] = pred.to(device)
    view = wide[..., 3:4]
    assert not view.is_contiguous()
    return view, gt, mask


def selected_count(case):
    pred, gt, mask = dense_inputs(case)
    sel = torch.ones(case.shape, dtype=torch.bool) if mask is None else (mask != 0).expand(case.shape)
    if case.loss == "bin":
        sel = sel & (pred.abs() > BIN_EPS) & (gt.abs() > BIN_EPS)
    return int(sel.sum())


def degenerate(case):
    return case.loss == "pearson" and selected_count(case) < 3


def _disp(d):
    """where(d > 0, 1 / d, 0) with the gradient this project defines at d <= 0: zero."""
    pos = d > 0
    return torch.where(pos, 1.0 / torch.where(pos, d, torch.ones_like(d)), torch.zeros_like(d))


def _masked_mean(x, sel):
    picked = x[sel]
    return picked.mean() if picked.numel() else x.sum() * 0.0


def dense_formula(loss, p, g, mask, wrong=None):
    """The reference's formula on tensors of one dtype (gsplat/losses.py:209-320 restated; boolean indexing as there).
    `wrong`: a deliberately wrong restatement - "raw" = Pearson from raw moments, "all" = a masked mean divided by all
    elements."""
    if loss == "l1":
        return (_disp(p) - _disp(g)).abs().mean() * SCALE
    sel = torch.ones_like(p, dtype=torch.bool) if mask is None else (mask != 0).expand_as(p)
    if loss == "bin":
        vp, vg = p.abs() > BIN_EPS, g.abs() > BIN_EPS
        ones = torch.ones_like(p)
        d = (1.0 / torch.where(vp, p, ones) - 1.0 / torch.where(vg, g, ones)).abs()
        sel = sel & vp & vg
        if wrong == "all":
            return torch.where(sel, d, torch.zeros_like(d)).sum() / max(d.numel(), 1)
        return _masked_mean(d, sel)
    pf, gf = p[sel], g[sel]
    if pf.numel() < 2:
        return p.sum() * 0.0
    if wrong == "raw":
        n = pf.numel()
        spp, sgg = (pf * pf).sum() - pf.sum() ** 2 / n, (gf * gf).sum() - gf.sum() ** 2 / n
        return 1.0 - ((pf * gf).sum() - pf.sum() * gf.sum() / n) / (spp * sgg).clamp(min=1e-12).sqrt()
    pc, gc = pf - pf.mean(), gf - gf.mean()
    return 1.0 - (pc * gc).sum() / (pc.pow(2).sum() * gc.pow(2).sum()).clamp(min=1e-12).sqrt()


def _evaluate(fn, x, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    val = fn(x)
    if val.requires_grad:
        val.backward()
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    return val.detach().double(), grad.detach().double()


@functools.lru_cache(maxsize=None)
def ref_dense(case, dtype=torch.float64, wrong=None):
    """(loss, grad of pred) of the restated reference evaluated in `dtype`, as float64 tensors. Shared, never modified."""
    pred, gt, mask = dense_inputs(case)
    return _evaluate(lambda p: dense_formula(case.loss, p, gt.to(dtype), mask, wrong), pred, dtype)


# ---- the sampled loss ---------------------------------------------------------------------------------------------------------
SampledCase = namedtuple("SampledCase", "name shape M family")
SAMPLED_MAPS = ((1, 2, 2), (2, 16, 16), (1, 37, 53))
SAMPLED_M = (1, 64, 65, 300)


@functools.lru_cache(maxsize=None)
def sampled_cases():
    out = [SampledCase(f"sampled-{'x'.join(map(str, s))}-{m}-pos", s, m, "pos") for s in SAMPLED_MAPS for m in SAMPLED_M]
    out += [SampledCase(f"sampled-{'x'.join(map(str, s))}-{m}-defined", s, m, "defined")
            for s, ms in (((1, 2, 2), (64,)), ((2, 16, 16), (65, 300)), ((1, 37, 53), (65, 300))) for m in ms]
    return tuple(out)


def zero_block(shape):
    """(y, x) of the top-left pixel of the 2 x 2 block of zeros of a "defined" map."""
    _, H, W = shape
    return (H - 2) // 2, (W - 2) // 2


@functools.lru_cache(maxsize=None)
def sampled_inputs(case):
    """(depth_map [C, H, W], points [C, M, 2] = (x, y), depths_gt [C, M]) float32 on the CPU. "pos": a map positive everywhere,
    points in the image - strictly inside, on integer coordinates, exactly on the last row / column, several in one pixel.
    "defined": a 2 x 2 block of zeros with points inside it, points more than one pixel outside the image, the rest of the
    points strictly inside and at least one pixel away from the block."""
    g = _gen(case.name)
    C, H, W = case.shape
    M = case.M
    dm = 3.0 + torch.rand(C, H, W, generator=g, dtype=torch.float64) * 2 - 1
    u = torch.rand(C, M, 2, generator=g, dtype=torch.float64)
    size = torch.tensor([W - 1.0, H - 1.0], dtype=torch.float64)
    kind = (torch.arange(M) % 4).expand(C, M)
    inside = u * size
    if case.family == "pos":
        integer = torch.round(inside)
        last = torch.where(torch.rand(C, M, 2, generator=g) > 0.5, size.expand(C, M, 2), inside)
        last[..., 0] = torch.where((last != size).all(-1), size[0], last[..., 0])
        shared = 0.25 + 0.5 * u
        pts = torch.where((kind == 1)[..., None], integer, inside)
        pts = torch.where((kind == 2)[..., None], last, pts)
        pts = torch.where((kind == 3)[..., None], shared, pts)
    else:
        by, bx = zero_block(case.shape)
        dm[:, by:by + 2, bx:bx + 2] = 0.0
        in_block = torch.tensor([bx, by], dtype=torch.float64) + 0.125 + 0.75 * u
        outside = torch.where(u > 0.5, size + 1.25 + 3 * u, -1.25 - 3 * u)
        if W >= 8:  # strictly inside, left of the block by at least one pixel
            away = torch.stack([u[..., 0] * (bx - 1.0), u[..., 1] * (H - 1.0)], -1)
        else:
            away = outside
        pts = torch.where((kind == 1)[..., None], in_block, away)
        pts = torch.where((kind == 2)[..., None], outside, pts)
    dgt = 3.0 + torch.rand(C, M, generator=g, dtype=torch.float64) * 2 - 1 + 0.3
    return dm.float(), pts.float(), dgt.float()


def sampled_formula(dm, pts, dgt, align_corners=True):
    """The trainer's block (examples/simple_trainer.py:962-980) on tensors of one dtype: normalise, F.grid_sample, disparity L1."""
    C, H, W = dm.shape
    grid = torch.stack([pts[:, :, 0] / (W - 1) * 2 - 1, pts[:, :, 1] / (H - 1) * 2 - 1], dim=-1).unsqueeze(2)
    d = F.grid_sample(dm.unsqueeze(1), grid, align_corners=align_corners).squeeze(3).squeeze(1)
    return (_disp(d) - _disp(dgt)).abs().mean() * SCALE


@functools.lru_cache(maxsize=None)
def ref_sampled(case, dtype=torch.float64, align_corners=True):
    dm, pts, dgt = sampled_inputs(case)
    return _evaluate(lambda m: sampled_formula(m, pts.to(dtype), dgt.to(dtype), align_corners), dm, dtype)


# ---- bounds -------------------------------------------------------------------------------------------------------------------
def family_of(case):
    return ("sampled" if isinstance(case, SampledCase) else case.loss, case.family)


def _ref(case, dtype):
    return ref_sampled(case, dtype) if isinstance(case, SampledCase) else ref_dense(case, dtype)


def loss_error(got, case):
    """|got - float64 reference| of a loss; both NaN (depth_l1_loss of nothing: a mean over no element) counts as 0."""
    ref = float(_ref(case, torch.float64)[0])
    got = float(got)
    if math.isnan(ref) or math.isnan(got):
        return 0.0 if math.isnan(ref) and math.isnan(got) else math.inf
    return abs(got - ref)


def grad_error(got, case):
    """max |got - float64 reference| / max |reference| of a gradient (0 for an empty one; an all-zero reference must be met
    exactly)."""
    ref = _ref(case, torch.float64)[1]
    got = got.detach().cpu().double().reshape(ref.shape)
    if ref.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err, top = float((got - ref).abs().max()), float(ref.abs().max())
    return err / top if top > 0 else (0.0 if err == 0 else math.inf)


@functools.lru_cache(maxsize=None)
def family_bounds():
    """{family: (loss bound, gradient bound)}: twice the largest error of the restated reference in float32 against float64
    over the family's cases (degenerate Pearson cases enter the loss bound only)."""
    worst = {}
    for case in dense_cases() + sampled_cases():
        loss32, grad32 = _ref(case, torch.float32)
        le = loss_error(loss32, case)
        ge = 0.0 if isinstance(case, DenseCase) and degenerate(case) else grad_error(grad32, case)
        a, b = worst.get(family_of(case), (0.0, 0.0))
        worst[family_of(case)] = (max(a, le), max(b, ge))
    return {k: (2 * a, 2 * b) for k, (a, b) in worst.items()}


def element_ratio(got, case):
    """Largest |got_i - ref_i| / (ELEMENT_TOL |ref_i|) of a disparity gradient; an element whose reference is 0 must be 0."""
    ref = ref_dense(case)[1]
    got = got.detach().cpu().double().reshape(ref.shape)
    if ref.numel() == 0:
        return 0.0
    err, tol = (got - ref).abs(), ELEMENT_TOL * ref.abs()
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))
    return float(r.max())


def check(case, loss, grad, share=1.0, element_share=None):
    """Assert a (loss, gradient) pair of `case` against the float64 reference within `share` of the bounds (`element_share` of
    the per-element bound of a disparity gradient; default `share`); returns the figures (loss error, gradient error or share
    of the per-element bound) for reports."""
    element_share = share if element_share is None else element_share
    lb, gb = family_bounds()[family_of(case)]
    le = loss_error(loss, case)
    assert le <= share * lb, (case.name, "loss", float(loss), float(_ref(case, torch.float64)[0]), le, lb)
    if isinstance(case, DenseCase) and degenerate(case):
        assert bool(torch.isfinite(grad).all()), (case.name, "gradient not finite")
        return le, 0.0
    if isinstance(case, DenseCase) and case.loss != "pearson":
        r = element_ratio(grad, case)
        assert r <= element_share, (case.name, "gradient, share of the per-element bound", r)
        return le, r
    ge = grad_error(grad, case)
    assert ge <= share * gb, (case.name, "gradient", ge, gb)
    return le, ge


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
