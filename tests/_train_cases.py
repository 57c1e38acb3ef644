"""Case builders, float64 references and per-element error bounds for the five training-step kernels of csrc/optim.hip -
adam_kernel / adam_vec4_kernel (op gsplat::adam, SelectiveAdam), relocation_kernel (compute_relocation), mcmc_perturb_kernel
(gsplat::mcmc_perturb_positions) and strategy_accumulate_kernel (DefaultStrategy._accumulate) - at the shapes where each launch
changes regime: both Adam kernels, pointers that are and are not 16-byte aligned, element / vector counts on both sides of a
256-lane block. Shared by tests/test_train_cases.py (CPU: float32 restatements lie inside every bound, one wrong restatement
per family falls outside) and tests/test_gpu_train_kernels.py (GPU: the kernels against the same references and bounds).
Everything here is seeded torch / numpy on the CPU; nothing imports the GPU package.

Conventions. EPS = 2^-24 (half a float32 ulp, relative). Every reference takes the float32 inputs as given and promotes them to
float64; a scalar hyperparameter is first rounded to float32 (that is what the kernel receives) and 1 - b is then formed in
float64, where it is exact. Each bound counts the roundings of the kernel's own expression, with or without fma contraction, and
carries a factor 2 over what a float32 evaluation on the CPU was seen to need (at most 0.50 of each bound).

Adam (no bias correction):  m' = b1 m + (1-b1) g,  v' = b2 v + (1-b2) g^2,  den = sqrt(v') + eps,  u = lr m'/den,  p' = p - u
    tol_m = 4 EPS (|b1 m| + |(1-b1) g|)
    tol_v = 8 EPS v'
    tol_p = 2 EPS |p'| + lr tol_m / den + |u| (8 EPS + tol_v / (2 sqrt(v') den))          (last quotient 0 where v' = 0)
Relocation (3DGS-as-MCMC, Eq. 9), n = clamp(ratio, 1, n_max):
    o' = clamp(1 - (1-o)^(1/n), min_opacity, 1 - 2^-23), bound ABSOLUTE 8 EPS (1 - o and 1 - pow carry absolute float32 error)
    scale' = scale o / S,  S = sum_{r=1..n} sum_{k<r} C(r-1, k) (-1)^k o'^(k+1) / sqrt(k+1), evaluated AT THE KERNEL'S OWN o'
    (so the error of the clamp and the error of the sum stay apart) with the float32 table as given;
    relative bound ((T + 2n + 8) kappa + 8) EPS with T = n (n+1) / 2 terms and kappa = sum |terms| / |S|.
SGLD perturb:  Sigma = R diag(exp s)^2 R^T (normalised quaternion),  w = noise_scale sigmoid(-k (sigmoid(logit) - t)),
    out = pos + Sigma (noise w);  bound per component 2 EPS |out| + (4 |k| (1 + |t|) + 48) EPS max(exp s)^2 ||noise w||_1.
Statistics, over the views with both radii > 0:  count exact;  radii within 3 EPS relative of max(state, max(r) / max_dim);
    grad2d within (C + 6) EPS (state_0 + sum_c norm_c)."""
import functools
import itertools
import math
from collections import namedtuple

import numpy as np
import torch

EPS = 2.0 ** -24
JUNK = (float("nan"), float("inf"), float("-inf"), 3.0e38, -1.0e30)  # what rows that must not be read carry


def f32(x):
    """A Python scalar as the kernel receives it: rounded to float32, promoted back."""
    return float(np.float32(x))


def ratio(got, ref, tol):
    """Largest |got - ref| / tol over all elements, as a float; an element with tol == 0 must be equal (else inf), a NaN or an
    infinity on either side counts as inf. 0.0 for empty tensors."""
    got, ref, tol = (torch.as_tensor(x, dtype=torch.float64).reshape(-1) for x in (got.detach().cpu(), ref, tol))
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    r = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    r = torch.where(torch.isfinite(err) & torch.isfinite(tol), r, torch.full_like(r, math.inf))
    return float(r.max())


def bits_equal(a, b):
    """Bit-for-bit equality of two float32 tensors (NaN payloads and the sign of zero included)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def place(t, misaligned, device):
    """A fresh contiguous copy of `t` on `device`: at the start of its own allocation (16-byte aligned), or - `misaligned` - one
    element into a larger buffer, `buf[1:1 + numel].view(shape)`, which is contiguous and 4 bytes off every wider alignment."""
    if not misaligned:
        return t.to(device).clone()
    buf = torch.empty(t.numel() + 2, dtype=t.dtype, device=device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def strided_bool(valid, device):
    """`valid` as a non-contiguous bool view (a column of a two-column tensor)."""
    view = torch.stack([valid, ~valid], dim=1).to(device)[:, 0]
    assert not view.is_contiguous() or valid.numel() <= 1
    return view


def _log_uniform(g, shape, lo, hi, signed):
    x = torch.exp(torch.empty(shape, dtype=torch.float64).uniform_(math.log(lo), math.log(hi), generator=g))
    if signed:
        x = x * (torch.randint(0, 2, shape, generator=g).double() * 2.0 - 1.0)
    return x.float()


# ---- Adam ------------------------------------------------------------------------------------------------------------------
ADAM_HYPER = ((1e-2, 0.9, 0.999, 1e-8), (1.6e-4, 0.9, 0.999, 1e-15), (5e-2, 0.0, 0.5, 1e-3))  # [1] is the trainer's
ADAM_WIDTHS = (1, 2, 3, 4, 5, 8, 45, 48)
# shape -> what it reaches (elements for the scalar kernel, float4 vectors for the vector one)
ADAM_SHAPES = (
    (1,), (255,), (256,), (257,), (1025,),          # D = 1: 1 / 255 / 256 / 257 / 1025 elements
    (130, 2),                                        # D = 2: 260 elements
    (85, 3), (86, 3),                                # D = 3: 255 / 258 elements
    (1, 4), (255, 4), (256, 4), (257, 4),            # D = 4: n_vec 1 / 255 / 256 / 257
    (52, 5),                                         # D = 5: 260 elements
    (128, 8), (129, 8),                              # D = 8: n_vec 256 / 258
    (6, 15, 3),                                      # D = 45: 270 elements (SH rows)
    (21, 16, 3), (22, 16, 3),                        # D = 48: n_vec 252 / 264
    (), (0, 3),                                      # a 0-dim parameter, a parameter with no rows
)
ADAM_MASKS = ("none", "all", "nothing", "alternating", "first", "last", "random60", "random60-strided")
ADAM_MISALIGN = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1))  # (param, grad, m, v)
ADAM_V_FLOOR = 1e-30  # v' is 0 or at least this: no subnormal enters a case

AdamCase = namedtuple("AdamCase", "name shape hyper mask misalign")


def adam_rows_width(shape):
    """(n_rows, row width) as gsplat::adam derives them from the parameter's shape."""
    n_rows = shape[0] if len(shape) > 0 else 1
    numel = int(np.prod(shape)) if len(shape) > 0 else 1
    return n_rows, (numel // n_rows if n_rows > 0 else 0)


def adam_takes_vec4(D, ptrs):
    """The host rule of gsx_adam restated: the float4 kernel runs when the row width is a multiple of 4 and the four base
    pointers (param, grad, exp_avg, exp_avg_sq) are multiples of 16."""
    return D % 4 == 0 and all(int(p) % 16 == 0 for p in ptrs)


def adam_launch_items(shape, vec4):
    """Work items of the launch: float4 vectors for the vector kernel, elements for the scalar one."""
    n_rows, D = adam_rows_width(shape)
    return n_rows * D // 4 if vec4 else n_rows * D


def _adam_case_list():
    cases = []

    def add(shape, h, mask, mis=ADAM_MISALIGN[0]):
        name = "x".join(map(str, shape)) or "scalar"
        cases.append(AdamCase(f"{name}-h{h}-{mask}-off{''.join(map(str, mis))}", tuple(shape), h, mask, tuple(mis)))

    for shape, h, mask in itertools.product(ADAM_SHAPES, range(len(ADAM_HYPER)), ("none", "random60")):
        add(shape, h, mask)
    for shape, mask in itertools.product(((257,), (86, 3), (257, 4), (22, 16, 3)), ADAM_MASKS):
        if mask not in ("none", "random60"):
            add(shape, 1, mask)
    for shape, mis, mask in itertools.product(((257, 4), (129, 8), (22, 16, 3)), ADAM_MISALIGN[1:], ("none", "alternating")):
        add(shape, 0 if mask == "none" else 2, mask, mis)
    return tuple(cases)


ADAM_CASES = _adam_case_list()
ADAM_BY_NAME = {c.name: c for c in ADAM_CASES}
# SelectiveAdam, three chained steps: (shape, hyper index)
ADAM_CHAINS = (((257, 4), 1), ((86, 3), 1), ((1025,), 0), ((22, 16, 3), 2), ((), 1))
ADAM_CHAIN_STEPS = 3


def adam_mask(kind, n_rows, seed):
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(7000 + seed)
    if kind == "all":
        return torch.ones(n_rows, dtype=torch.bool)
    valid = torch.zeros(n_rows, dtype=torch.bool)
    if kind == "nothing" or n_rows == 0:
        return valid
    if kind == "alternating":
        valid[::2] = True
    elif kind == "first":
        valid[0] = True
    elif kind == "last":
        valid[-1] = True
    else:
        valid = torch.rand(n_rows, generator=g) < 0.6
    return valid


def adam_values(shape, seed, with_state=True):
    """(p, g, m, v, never_seen rows): random signs, log-uniform magnitudes (|p| 1e-4..1e2, |g| and |m| 1e-9..1e1, v 1e-18..1e2),
    every 7th v, 11th m and 13th g exactly 0, and - from three rows on - every 5th row with g = m = v = 0 (a Gaussian that was
    never seen: its parameter must come back bit-identical, its moments exactly 0). `with_state=False`: m = v = 0 everywhere."""
    gen = torch.Generator().manual_seed(1000 + seed)
    shape = tuple(shape)
    p = _log_uniform(gen, shape, 1e-4, 1e2, True)
    g = _log_uniform(gen, shape, 1e-9, 1e1, True)
    m = _log_uniform(gen, shape, 1e-9, 1e1, True)
    v = _log_uniform(gen, shape, 1e-18, 1e2, False)
    n = p.numel()
    flat = torch.arange(n)
    v.view(-1)[flat % 7 == 6] = 0.0
    m.view(-1)[flat % 11 == 10] = 0.0
    g.view(-1)[flat % 13 == 12] = 0.0
    if not with_state:
        m.zero_(), v.zero_()
    n_rows, _ = adam_rows_width(shape)
    never = torch.zeros(n_rows, dtype=torch.bool)
    if n_rows >= 3 and len(shape) > 0:
        never[2::5] = True
        g[never], m[never], v[never] = 0.0, 0.0, 0.0
    return p, g, m, v, never


def poison_rows(tensors, rows):
    """Fill `rows` (bool per row) of every tensor with NaN, +-Inf and large finite values, cycling per element."""
    junk = torch.tensor(JUNK)
    for t in tensors:
        if t.dim() == 0:
            if bool(rows.reshape(-1)[0]):
                t.fill_(JUNK[0])
            continue
        k = int(rows.sum()) * (t[0].numel() if t.shape[0] else 0)
        if k:
            t[rows] = junk[torch.arange(k) % len(JUNK)].reshape((-1,) + tuple(t.shape[1:]))


@functools.lru_cache(maxsize=None)
def adam_case(name):
    """CPU tensors of a case: dict(p, g, m, v, valid (bool [rows] or None), never (bool [rows]), lr, b1, b2, eps, D, n_rows).
    In a masked case the rows that are not selected carry NaN, +-Inf and large finite values in all four tensors."""
    c = ADAM_BY_NAME[name]
    seed = ADAM_CASES.index(c)
    p, g, m, v, never = adam_values(c.shape, seed)
    n_rows, D = adam_rows_width(c.shape)
    valid = adam_mask(c.mask, n_rows, seed)
    if valid is not None:
        poison_rows((p, g, m, v), ~valid)
    lr, b1, b2, eps = ADAM_HYPER[c.hyper]
    out = dict(p=p, g=g, m=m, v=v, valid=valid, never=never, lr=lr, b1=b1, b2=b2, eps=eps, D=D, n_rows=n_rows)
    ref = adam_ref(p, g, m, v, valid, lr, b1, b2, eps)
    sel = _row_select(valid, p)
    v_ref = ref[2][sel]
    assert bool(((v_ref == 0) | (v_ref >= ADAM_V_FLOOR)).all()), "a subnormal second moment entered the case"
    return out


def _row_select(valid, like):
    """Element-wise bool of `like`'s shape from a per-row mask (None = every row)."""
    if valid is None:
        return torch.ones(like.shape, dtype=torch.bool)
    if like.dim() == 0:
        return valid.reshape(())
    return valid.reshape((-1,) + (1,) * (like.dim() - 1)).expand(like.shape)


def adam_ref(p, g, m, v, valid, lr, b1, b2, eps):
    """Float64 Adam step of the float32 inputs. Returns p_ref, m_ref, v_ref, tol_p, tol_m, tol_v (float64, the inputs' shape);
    rows with valid == False hold the promoted inputs and a bound of 0 (they are compared bit-for-bit, not by value)."""
    sel = _row_select(valid, p)
    p64, g64, m64, v64 = (torch.where(sel, t.detach().cpu(), torch.zeros_like(t.detach().cpu())).double() for t in (p, g, m, v))
    lr, b1, b2, eps = f32(lr), f32(b1), f32(b2), f32(eps)
    am, ag = b1 * m64, (1.0 - b1) * g64
    m_ref = am + ag
    v_ref = b2 * v64 + (1.0 - b2) * g64 * g64
    root = torch.sqrt(v_ref)
    den = root + eps
    u = lr * m_ref / den
    p_ref = p64 - u
    tol_m = 4.0 * EPS * (am.abs() + ag.abs())
    tol_v = 8.0 * EPS * v_ref
    quot = torch.where(v_ref > 0, tol_v / (2.0 * root * den).clamp_min(1e-300), torch.zeros_like(v_ref))
    tol_p = 2.0 * EPS * p_ref.abs() + lr * tol_m / den + u.abs() * (8.0 * EPS + quot)
    zero = torch.zeros_like(p64)
    keep = [t.detach().cpu().double() for t in (p, m, v)]
    return (torch.where(sel, p_ref, keep[0]), torch.where(sel, m_ref, keep[1]), torch.where(sel, v_ref, keep[2]),
            torch.where(sel, tol_p, zero), torch.where(sel, tol_m, zero), torch.where(sel, tol_v, zero))


def adam_check(got_p, got_m, got_v, before, valid, never, hyper):
    """Compare one step's float32 results with adam_ref of `before` = (p, g, m, v) float32 inputs. Returns the largest
    error / bound over the selected rows; asserts that rows that are not selected are bit-identical in all three tensors and that
    selected never-seen rows keep their parameter bit-for-bit with moments exactly 0."""
    p, g, m, v = (t.detach().cpu() for t in before)
    got = [t.detach().cpu() for t in (got_p, got_m, got_v)]
    refs = adam_ref(p, g, m, v, valid, *hyper)
    sel = _row_select(valid, p)
    worst = 0.0
    for name, out, old, ref, tol in zip("pmv", got, (p, m, v), refs[:3], refs[3:]):
        assert out.shape == old.shape
        assert bits_equal(out[~sel], old[~sel]), f"{name}: a row that is not selected changed"
        worst = max(worst, ratio(out[sel], ref[sel], tol[sel]))
    if never is not None and p.dim() > 0 and bool(never.any()):
        rows = never if valid is None else never & valid
        assert bits_equal(got[0][rows], p[rows]), "never-seen rows: the parameter changed"
        assert bool((got[1][rows] == 0).all()) and bool((got[2][rows] == 0).all()), "never-seen rows: a moment is not 0"
    return worst


# ---- relocation ------------------------------------------------------------------------------------------------------------
RELOC_N_MAX = 51
RELOC_OPACITIES = (1e-4, 0.004, 0.005, 0.01, 0.3, 0.7, 0.9, 0.99, 0.999)
RELOC_RATIOS = (1, 2, 3, 5, 11, 12, 20, 35, 50, 51)
RELOC_MIN_OPACITIES = (0.005, 0.0)
RELOC_MIN_ROWS = 257
RELOC_MAX_BOUND = 2e-2  # condition on the grid: every row's relative scale bound is below this (9.8e-3 at o 0.999, n 51)
RELOC_TOL_O = 8.0 * EPS
RELOC_UPPER = 1.0 - 2.0 ** -23
RELOC_SMALL_N_MAX = 12
RELOC_SMALL_RATIOS = (0, -3, 13, 1000)
RELOC_CORNER_OPACITIES = (1.0 - 2.0 ** -24, 1.0)
RELOC_CORNER_RATIOS = (1, 51)


@functools.lru_cache(maxsize=None)
def binoms(n_max=RELOC_N_MAX):
    """The float32 table of MCMCStrategy.initialize_state: C(n, k) for n, k < n_max."""
    return torch.tensor([[float(math.comb(n, k)) if k <= n else 0.0 for k in range(n_max)] for n in range(n_max)])


def _reloc_rows(opacities, ratios, min_rows, seed):
    pairs = list(itertools.product(opacities, ratios))
    reps = max(1, -(-min_rows // len(pairs)))
    o = torch.tensor([p[0] for p in pairs] * reps, dtype=torch.float64).float()
    r = torch.tensor([p[1] for p in pairs] * reps, dtype=torch.int64)
    g = torch.Generator().manual_seed(seed)
    scales = torch.rand(len(o), 3, generator=g) * 0.1 + 0.01
    return o, scales, r


@functools.lru_cache(maxsize=None)
def relocation_grid():
    """(opacities [R], scales [R, 3], ratios int64 [R]): the 9 x 10 grid tiled to at least 257 rows, fresh scales per row."""
    return _reloc_rows(RELOC_OPACITIES, RELOC_RATIOS, RELOC_MIN_ROWS, 31)


@functools.lru_cache(maxsize=None)
def relocation_small():
    """Ratios outside [1, n_max] for the 12 x 12 table: (opacities, scales, ratios int64, the table)."""
    return _reloc_rows(RELOC_OPACITIES, RELOC_SMALL_RATIOS, 1, 32) + (binoms()[:RELOC_SMALL_N_MAX, :RELOC_SMALL_N_MAX].contiguous(),)


@functools.lru_cache(maxsize=None)
def relocation_corners():
    return _reloc_rows(RELOC_CORNER_OPACITIES, RELOC_CORNER_RATIOS, 1, 33)


def relocation_ref(o, scales, ratios, table, min_opacity, o_new_used):
    """Float64 reference (see the module docstring). Returns a dict of float64 arrays: o_new (clamped), tol_o, n, coeff, S, A,
    kappa, T, scales (coeff x scale, [R, 3]) and rel (the relative bound of each scale component, [R])."""
    n_max = table.shape[0]
    o = o.detach().cpu().double().numpy()
    used = o_new_used.detach().cpu().double().numpy()
    n = np.clip(ratios.detach().cpu().numpy().astype(np.int64), 1, n_max)
    with np.errstate(all="ignore"):
        o_new = np.clip(1.0 - np.power(1.0 - o, 1.0 / n), f32(min_opacity), RELOC_UPPER)
    B = table.detach().cpu().double().numpy()
    cum = np.concatenate([np.zeros((1, n_max)), np.cumsum(B, axis=0)], axis=0)  # cum[n, k] = sum_{r <= n} C(r-1, k)
    k = np.arange(n_max)
    mag = cum[n] / np.sqrt(k + 1.0) * used[:, None] ** (k + 1.0)  # [R, n_max]: all terms of one k share a sign
    S = (mag * np.where(k % 2 == 0, 1.0, -1.0)).sum(axis=1)
    A = mag.sum(axis=1)
    with np.errstate(all="ignore"):
        kappa = A / np.abs(S)
        coeff = o / S
    T = n * (n + 1) / 2.0
    rel = (T + 2.0 * n + 8.0) * EPS * kappa + 8.0 * EPS
    return dict(o_new=o_new, tol_o=np.full_like(o_new, RELOC_TOL_O), n=n, coeff=coeff, S=S, A=A, kappa=kappa, T=T,
                scales=coeff[:, None] * scales.detach().cpu().double().numpy(), rel=rel)


def relocation_check(o, scales, ratios, table, min_opacity, new_o, new_s):
    """(largest opacity error / bound, largest scale error / bound, the reference dict) of a float32 result."""
    ref = relocation_ref(o, scales, ratios, table, min_opacity, new_o)
    r_o = ratio(new_o, torch.from_numpy(ref["o_new"]), torch.from_numpy(ref["tol_o"]))
    tol_s = np.abs(ref["scales"]) * ref["rel"][:, None]
    r_s = ratio(new_s, torch.from_numpy(ref["scales"]), torch.from_numpy(tol_s))
    return r_o, r_s, ref


def relocation_f32(o, scales, ratios, table, min_opacity, clamp_first=True):
    """The kernel's expression in numpy float32, term by term in the kernel's order. `clamp_first=False` is the deliberately
    wrong variant: the scale is computed from the unclamped opacity and the clamp applied afterwards."""
    n_max = table.shape[0]
    o = o.numpy().astype(np.float32)
    n = np.clip(ratios.numpy().astype(np.int64), 1, n_max)
    B = table.numpy().astype(np.float32)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        raw = one - np.power(one - o, one / n.astype(np.float32)).astype(np.float32)
        clamped = np.minimum(np.maximum(raw, np.float32(min_opacity)), np.float32(RELOC_UPPER))
        x = clamped if clamp_first else raw
        denom = np.zeros_like(o)
        for r in range(1, n_max + 1):
            live = r <= n
            if not live.any():
                break
            pw, sign = x.copy(), 1.0
            for k in range(r):
                term = (B[r - 1, k] * (np.float32(sign) / np.sqrt(np.float32(k + 1)))) * pw
                denom = np.where(live, denom + term, denom).astype(np.float32)
                pw = (pw * x).astype(np.float32)
                sign = -sign
        coeff = (o / denom).astype(np.float32)
        new_s = (coeff[:, None] * scales.numpy().astype(np.float32)).astype(np.float32)
    return torch.from_numpy(clamped), torch.from_numpy(new_s)


# ---- SGLD perturb ----------------------------------------------------------------------------------------------------------
PERTURB_ROWS = (1, 255, 256, 257)
PERTURB_PARAMS = ((0.01, 0.005, 100.0), (1.0, 0.005, 100.0), (0.25, 0.25, 8.0), (0.8, 0.005, 100.0))
PERTURB_ZERO_SCALE = (0.0, 0.005, 100.0)  # noise_scale 0: every position bit-identical (run at 257 rows)
PERTURB_HI_ROWS, PERTURB_LO_ROWS = (3, -1), (7,)  # rows with logit +30 / -30 (in cases of 255 rows and more)
PERTURB_OVERFLOW = 88.8  # expf(x) is +inf in float32 from x = 88.73 on


def perturb_w_is_zero(t, k):
    """Whether a logit of +30 (density exactly 1.0f) makes the kernel's expf(k (density - t)) overflow, so that w = 0 exactly."""
    return f32(k) * (1.0 - f32(t)) > PERTURB_OVERFLOW


@functools.lru_cache(maxsize=None)
def perturb_case(n):
    """dict(pos [n, 3], quats [n, 4] unnormalised, log_scales [n, 3] in -6..2, logits [n] in -12..12, noise [n, 3], hi, lo):
    float32 CPU tensors; `hi` / `lo` are the rows whose logit is +30 / -30."""
    g = torch.Generator().manual_seed(500 + n)
    pos = torch.randn(n, 3, generator=g)
    pos = torch.where(pos.abs() < 1e-3, torch.full_like(pos, 0.5), pos)  # non-zero positions
    quats = torch.randn(n, 4, generator=g)
    log_scales = torch.rand(n, 3, generator=g) * 8.0 - 6.0
    logits = torch.rand(n, generator=g) * 24.0 - 12.0
    noise = torch.randn(n, 3, generator=g)
    hi = torch.zeros(n, dtype=torch.bool)
    lo = torch.zeros(n, dtype=torch.bool)
    if n >= 255:
        hi[list(PERTURB_HI_ROWS)] = True
        lo[list(PERTURB_LO_ROWS)] = True
        logits[hi], logits[lo] = 30.0, -30.0
    return dict(pos=pos, quats=quats, log_scales=log_scales, logits=logits, noise=noise, hi=hi, lo=lo)


def perturb_ref(pos, quats, log_scales, logits, noise, noise_scale, t, k):
    """Float64 reference. Returns out_ref [n, 3], tol [n, 3], w_ref [n]."""
    pos, q, s, lg, nz = (x.detach().cpu().double() for x in (pos, quats, log_scales, logits, noise))
    noise_scale, t, k = f32(noise_scale), f32(t), f32(k)
    q = q / q.norm(dim=-1, keepdim=True)
    w_, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w_ * z), 2 * (x * z + w_ * y),
                     2 * (x * y + w_ * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w_ * x),
                     2 * (x * z - w_ * y), 2 * (y * z + w_ * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    e = torch.exp(s)
    M = R * e[:, None, :]
    sigma = M @ M.transpose(-1, -2)
    w = noise_scale * torch.sigmoid(-k * (torch.sigmoid(lg.reshape(-1)) - t))
    nw = nz * w[:, None]
    out = pos + torch.einsum("nij,nj->ni", sigma, nw)
    amp = e.amax(dim=-1) ** 2 * nw.abs().sum(dim=-1)
    tol = 2.0 * EPS * out.abs() + (4.0 * abs(k) * (1.0 + abs(t)) + 48.0) * EPS * amp[:, None]
    return out, tol, w


# ---- DefaultStrategy statistics --------------------------------------------------------------------------------------------
ACC_N = (1, 255, 256, 257, 1000)
ACC_C = (1, 2, 5)
ACC_LAYOUTS = ("contiguous", "rows")  # "rows": a column pair (3:5) of 9-float rows
ACC_W, ACC_H = 640, 360
ACC_HIDDEN = ((0, 5), (5, 0), (-1, 7), (0, 0))
AccCase = namedtuple("AccCase", "name N C layout absgrad track")
ACC_CASES = tuple(
    [AccCase(f"N{n}-C{c}-{lay}-{'abs' if a else 'grad'}-track", n, c, lay, a, True)
     for n, c, lay, a in itertools.product(ACC_N, ACC_C, ACC_LAYOUTS, (False, True))]
    + [AccCase(f"N257-C{c}-{lay}-grad-notrack", 257, c, lay, False, False) for c, lay in itertools.product(ACC_C, ACC_LAYOUTS)])
ACC_BY_NAME = {c.name: c for c in ACC_CASES}


@functools.lru_cache(maxsize=None)
def accumulate_inputs(N, C, finite=False):
    """dict(grad [C, N, 2] float32, radii [C, N, 2] int32, state = dict(grad2d, count, radii: [N] float32 start values)). About a third of the
    (view, Gaussian) pairs are hidden by one of the patterns (0, 5), (5, 0), (-1, 7), (0, 0); with C >= 2 view 1 is hidden
    entirely. Hidden rows carry NaN / +-Inf gradients (`finite=True`: ordinary values, for layouts whose rows overlap)."""
    g = torch.Generator().manual_seed(900 + 10 * N + C)
    grad = torch.randn(C, N, 2, generator=g) * 1e-4
    radii = torch.randint(1, 40, (C, N, 2), generator=g, dtype=torch.int32)
    which = torch.randint(0, 3 * len(ACC_HIDDEN), (C, N), generator=g)  # < len(ACC_HIDDEN): hidden by that pattern
    if C >= 2:
        which[1] = torch.arange(N) % len(ACC_HIDDEN)
    pats = torch.tensor(ACC_HIDDEN, dtype=torch.int32)
    hidden = which < len(ACC_HIDDEN)
    radii[hidden] = pats[which[hidden]]
    if not finite:
        k = int(hidden.sum())
        junk = torch.tensor(JUNK[:3])
        grad[hidden] = junk[torch.arange(2 * k) % 3].reshape(k, 2)
    state = dict(grad2d=torch.rand(N, generator=g), count=torch.full((N,), 3.0), radii=torch.full((N,), 0.01))
    state["radii"][::4] = 0.5  # a running maximum that no radius of this step exceeds
    return dict(grad=grad, radii=radii, state=state)


def accumulate_scalars(C):
    """(half_w, half_h, max_dim) as DefaultStrategy._accumulate forms them for C cameras of ACC_W x ACC_H."""
    return 0.5 * ACC_W * C, 0.5 * ACC_H * C, float(max(ACC_W, ACC_H))


def accumulate_ref(grad, radii, state, half_w, half_h, max_dim):
    """Float64 reference over the views where both radii are > 0. `state` holds the float32 start values (grad2d, count and,
    where tracked, radii). Returns dict(grad2d, tol_grad2d, count, radii, tol_radii) in float64 (radii entries None if untracked)."""
    N = radii.shape[-2]
    g = grad.detach().cpu().reshape(-1, N, 2)
    C = g.shape[0]
    r = radii.detach().cpu().reshape(C, N, 2)
    seen = (r > 0).all(dim=-1)
    g64 = torch.where(seen[..., None], g, torch.zeros_like(g)).double()
    norms = torch.sqrt((g64[..., 0] * f32(half_w)) ** 2 + (g64[..., 1] * f32(half_h)) ** 2)
    norms = torch.where(seen, norms, torch.zeros_like(norms))
    s0 = state["grad2d"].detach().cpu().double()
    total = s0 + norms.sum(dim=0)
    out = dict(grad2d=total, tol_grad2d=(C + 6.0) * EPS * total, count=state["count"].detach().cpu().double() + seen.sum(dim=0).double(),
               radii=None, tol_radii=None)
    if state.get("radii") is not None:
        rel = torch.where(seen, r.amax(dim=-1).double() / float(max_dim), torch.zeros(C, N, dtype=torch.float64))
        out["radii"] = torch.maximum(state["radii"].detach().cpu().double().expand(N), rel.amax(dim=0))
        out["tol_radii"] = 3.0 * EPS * out["radii"]
    return out


def accumulate_check(got, ref):
    """Largest error / bound of grad2d and (where tracked) radii; the view counts must be equal."""
    assert torch.equal(got["count"].detach().cpu().double(), ref["count"]), "view counts differ"
    worst = ratio(got["grad2d"], ref["grad2d"], ref["tol_grad2d"])
    if ref["radii"] is not None:
        worst = max(worst, ratio(got["radii"], ref["radii"], ref["tol_radii"]))
    return worst


class GradHolder:
    """Stands in for info["means2d"]: the strategy only reads `.grad` / `.absgrad` (a strided view cannot be assigned to the
    `.grad` of a contiguous leaf)."""

    def __init__(self, grad, absgrad):
        self.grad = None if absgrad else grad
        self.absgrad = grad if absgrad else None


def accumulate_layout(grad, layout, device):
    """The gradient on `device` as a contiguous tensor or as columns 3:5 of 9-float rows whose other columns are NaN."""
    if layout == "contiguous":
        return grad.to(device).clone()
    wide = torch.full(grad.shape[:-1] + (9,), float("nan"), device=device)
    wide[..., 3:5] = grad.to(device)
    view = wide[..., 3:5]
    assert not view.is_contiguous() or grad.numel() == 2  # a single row is contiguous whatever its stride
    return view


def accumulate_info(grad_view, radii, C, absgrad):
    return {"width": ACC_W, "height": ACC_H, "n_cameras": C, "radii": radii, "gaussian_ids": None,
            "means2d": GradHolder(grad_view, absgrad)}
