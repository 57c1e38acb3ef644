"""Cases of the colour-correction tests (test_color_correct.py on the CPU, test_gpu_color_correct.py on the GPU) and of
tools/pin_color_correct_against_reference.py, which runs the reference on them and writes tests/golden/color_correct_ref.npz.

Inputs are built from seeds with numpy; the tests of the small inputs read the arrays the reference was run on from the fixture
(and check that the builders still give them), the large input is a fixed permutation of a small one's pixels.

Guard band. The quadratic fit selects its rows by comparing values with two thresholds, so one value changing sides moves a
2 k-pixel fit by more than any rounding bound. Every non-singular input therefore satisfies, in a float64 evaluation
(`trace64`): no value of img, of ref or of the image after any iteration lies within GUARD of float32(eps) or float32(1 - eps)
unless it equals the threshold exactly (the planted ones), and every scaled Cholesky pivot of every system is above MIN_PIVOT.
The seeds below were searched for that (the pin tool's --search) and the pin tool refuses to write a fixture otherwise."""
import math
import os
from collections import namedtuple

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "color_correct_ref.npz")

EPS = 0.5 / 255   # the default of color_correct_quadratic
EPS2 = 6.0 / 255  # the second eps of the variants
GUARD = 1e-5
MIN_PIVOT = 1e-6
STRIDE = 4099     # the large case keeps every STRIDE-th output element
SMALL = 3200      # pixels up to which a case stores its inputs and whole outputs
PLANTED = 24      # values of img and of ref set to each threshold in the "thresholds" input

Input = namedtuple("Input", "key kind shape seed")
Case = namedtuple("Case", "name input num_iters eps")


def launch_edges():
    """(span, cap, cap_n) of gsx_cc_blocks: one workgroup up to `span` pixels, at most `cap` workgroups, reached at `cap_n`."""
    from gsplat_amd import _cabi

    blocks = _cabi._lib.gsx_cc_blocks
    span = 1
    while blocks(2 * span) == 1:
        span *= 2
    lo, hi = span, 2 * span  # blocks(lo) == 1 < blocks(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if blocks(mid) == 1 else (lo, mid)
    cap = blocks(1 << 50)
    return lo, cap, lo * cap


SEEDS = {"nat-37x53": 6, "nat-2x19x23": 1, "nat-span-1": 2, "nat-span": 1, "nat-span+1": 1, "thr-37x53": 7, "poison-23x19": 1}


def inputs_table():
    span, _cap, cap_n = launch_edges()
    rows = [
        Input("nat-37x53", "natural", (37, 53, 3), SEEDS["nat-37x53"]),
        Input("nat-2x19x23", "natural", (2, 19, 23, 3), SEEDS["nat-2x19x23"]),
        Input("nat-span-1", "natural", (span - 1, 3), SEEDS["nat-span-1"]),
        Input("nat-span", "natural", (span, 3), SEEDS["nat-span"]),
        Input("nat-span+1", "natural", (span + 1, 3), SEEDS["nat-span+1"]),
        Input("thr-37x53", "thresholds", (37, 53, 3), SEEDS["thr-37x53"]),
        Input("poison-23x19", "poisoned", (23, 19, 3), SEEDS["poison-23x19"]),
        Input("tiled-cap+1", "tiled", (cap_n + 1, 3), 0),  # one pixel past the capped grid: nat-37x53's pixels, permuted
    ]
    return {r.key: r for r in rows}


def cases():
    """Every non-singular case: each input with the defaults, and the variants on the first."""
    out = [Case(f"{key}-i5", key, 5, EPS) for key in inputs_table()]
    out += [Case("nat-37x53-i0", "nat-37x53", 0, EPS), Case("nat-37x53-i1", "nat-37x53", 1, EPS),
            Case("nat-37x53-i5-eps2", "nat-37x53", 5, EPS2)]
    return out


def thresholds(eps):
    """(float32(eps), float32(1 - eps)) as Python floats: what torch compares a float32 tensor with."""
    return float(np.float32(eps)), float(np.float32(1.0 - eps))


def _scene(n_pixels, width, rng):
    """A smooth scene [n, 3] that leaves [0, 1] on roughly a tenth of its values."""
    i = np.arange(n_pixels, dtype=np.float64)
    u, v = (i % width) / width, np.floor(i / width) / max(1.0, math.ceil(n_pixels / width))
    s = np.empty((n_pixels, 3))
    for c in range(3):
        fu, fv, gu, gv = rng.uniform(0.4, 1.6, 4)
        p, q = rng.uniform(0.0, 2.0 * math.pi, 2)
        s[:, c] = 0.5 + 0.42 * np.sin(2.0 * math.pi * (fu * u + fv * v) + p) + 0.22 * np.sin(2.0 * math.pi * (2.3 * gu * u - 1.7 * gv * v) + q)
    return s


def _natural(shape, rng):
    n = int(np.prod(shape[:-1]))
    s = _scene(n, shape[-2] if len(shape) > 2 else 37, rng)
    twist = np.eye(3) + rng.uniform(-0.15, 0.15, (3, 3))
    quad = rng.uniform(-0.12, 0.12, (3, 3))
    img = s @ twist + (s * s) @ quad + rng.uniform(-0.04, 0.04, 3) + 0.01 * rng.standard_normal((n, 3))
    return np.clip(img, 0.0, 1.0).astype(np.float32).reshape(shape), np.clip(s, 0.0, 1.0).astype(np.float32).reshape(shape)


def build(inp, base=None):
    """(img, ref) float32 numpy arrays of an Input; `base` = (img, ref) of nat-37x53 for the tiled one."""
    if inp.kind == "tiled":
        img0, ref0 = (a.reshape(-1, 3) for a in (base if base is not None else build(inputs_table()["nat-37x53"])))
        idx = (np.arange(inp.shape[0], dtype=np.int64) * 7919) % img0.shape[0]  # 7919 is prime to 37 * 53
        return img0[idx], ref0[idx]
    rng = np.random.default_rng([inp.seed, sum(map(ord, inp.key))])
    img, ref = _natural(inp.shape, rng)
    if inp.kind == "thresholds":
        lo, hi = np.float32(EPS), np.float32(1.0 - EPS)
        where = rng.permutation(img.size)[:4 * PLANTED].reshape(4, PLANTED)
        img.reshape(-1)[where[0]], img.reshape(-1)[where[1]] = lo, hi
        ref.reshape(-1)[where[2]], ref.reshape(-1)[where[3]] = lo, hi
    if inp.kind == "poisoned":  # where ref is saturated it says nothing about the scene: 0 or 1 by a coin
        sat = (ref <= 0.0) | (ref >= 1.0)
        ref[sat] = rng.integers(0, 2, int(sat.sum())).astype(np.float32)
    return img, ref


def singular_inputs():
    """{name: (img, ref)} float32 tensors whose quadratic systems are rank-deficient."""
    img, ref = (torch.from_numpy(a) for a in build(Input("singular", "natural", (23, 19, 3), 5)))
    ones = ref.clone()
    ones[..., 1] = 1.0
    return {"grey": (img[..., :1].expand(23, 19, 3).contiguous(), ref), "ref-channel-all-ones": (img, ones),
            "one-pixel": (img[3, 4].reshape(1, 3).clone(), ref[3, 4].reshape(1, 3).clone())}


def features(x):
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    return np.stack([r * r, r * g, r * b, g * g, g * b, b * b, r, g, b, np.ones_like(r)], axis=1)


def trace64(img, ref, num_iters, eps):
    """The quadratic correction in float64 by normal equations, thresholds as float32 decides them.
    Returns ([the image after 0, 1, ... num_iters iterations], smallest scaled Cholesky pivot)."""
    lo, hi = thresholds(eps)
    x, r = img.reshape(-1, 3).astype(np.float64), ref.reshape(-1, 3).astype(np.float64)
    ok0 = (x >= lo) & (x <= hi) & (r >= lo) & (r <= hi)
    steps, pivot = [x], math.inf
    for _ in range(num_iters):
        A = features(x)
        W = np.zeros((10, 3))
        for c in range(3):
            m = ok0[:, c] & (x[:, c] >= lo) & (x[:, c] <= hi)
            G, y = A[m].T @ A[m], A[m].T @ r[m, c]
            d = np.sqrt(np.diag(G))
            if not (d > 0).all():
                return steps, 0.0
            S = G / np.outer(d, d)
            try:
                L = np.linalg.cholesky(S)
            except np.linalg.LinAlgError:
                return steps, 0.0
            pivot = min(pivot, float((np.diag(L) ** 2).min()))
            W[:, c] = np.linalg.solve(S, y / d) / d
        x = np.clip(A @ W, 0.0, 1.0)
        steps.append(x)
    return steps, pivot


def guard_report(img, ref, num_iters, eps):
    """(closest approach of a non-planted value to a threshold, smallest pivot) of the float64 evaluation."""
    steps, pivot = trace64(img, ref, num_iters, eps)
    gap = math.inf
    for t in thresholds(eps):
        for a in steps + [ref.reshape(-1, 3).astype(np.float64)]:
            d = np.abs(a - t)
            d = d[d > 0.0]  # a value exactly on a threshold is decided the same in every precision
            gap = min(gap, float(d.min()) if d.size else math.inf)
    return gap, pivot


def holds(img, ref, num_iters, eps):
    gap, pivot = guard_report(img, ref, num_iters, eps)
    return gap > GUARD and pivot > MIN_PIVOT


def load_inputs(pinned, case_or_key):
    """(img, ref) float32 tensors of a case: the fixture's arrays for a small input, the builder's for the tiled one."""
    inp = inputs_table()[case_or_key.input if isinstance(case_or_key, Case) else case_or_key]
    if inp.kind == "tiled":
        arrays = build(inp, (pinned["in/nat-37x53/img"], pinned["in/nat-37x53/ref"]))
    else:
        arrays = (pinned[f"in/{inp.key}/img"], pinned[f"in/{inp.key}/ref"])
    return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in arrays)


def expected(pinned, name, out):
    """(`out` restricted to the elements the fixture keeps for quadratic case / affine input `name`, their float64 reference,
    the reference's own float32 error e32)."""
    want = torch.from_numpy(pinned[f"{name}/out64"])
    got = out.detach().cpu().double()
    got = got.reshape(-1)[::STRIDE] if want.numel() != got.numel() else got.reshape(want.shape)
    return got, want, float(pinned[f"{name}/e32"])
