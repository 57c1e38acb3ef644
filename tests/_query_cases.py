"""Case builders and a plain float64 reference walk for the query rasterizers (csrc/raster_query.hip: num_contributing,
contributing_ids, top_contributing, their sparse twins and the gsx_raster3d_pair_stats counters) and for
rasterize_to_indices_in_range (csrc/raster_indices.hip). Shared by tests/test_query_cases.py (CPU: the cases reach what they
claim, the fp32 C oracle agrees with the walk) and tests/test_gpu_query.py (GPU: the kernels against the walk).

Inputs are made on the CPU - make_scene -> oracle.fully_fused_projection -> oracle.isect_tiles / isect_offset_encode (sparse:
oracle.sparse_tile_layout / isect_tiles_sparse) - and uploaded as they are, so that the kernels and the reference decide on
identical fp32 numbers.

The reference is a per-pixel front-to-back walk in float64 (numpy, vectorised over the pixels of a tile), over the batches
[range_start, range_end) of tile_size^2 list entries and from a per-pixel transmittance T0, so it serves the indices op too:
    sigma = a dx^2 / 2 + c dy^2 / 2 + b dx dy,  d = mean - pixel centre;  alpha = min(0.99, opacity exp(-sigma))
    a candidate contributes when sigma >= 0 and alpha >= 1/255; the pixel stops (exclusive) when T (1 - alpha) <= 1e-4.
Top-K follows include/gsplat_amd.h: a sample replaces the first weakest kept slot only if strictly stronger; the slots are
re-sorted by depth index; unused slots (-1, 0) come last.

A pixel is DECIDED when, among the candidates it evaluates before it stops (the stopping one included), float64 is outside a
margin on every decision an fp32 kernel could take the other way. Only undecided pixels may be skipped by a comparison.

Measured on the CPU with these builders and the margins below (tests/test_query_cases.py asserts the regimes and the caps: walk
<= 5 %, top-K <= 10 %; the GPU tests recompute the shares). "sigma < 0" counts the walked candidates on that branch.

    case     tiles (empty)  longest list  counts    saturating  sigma < 0  undecided walk  undecided top-K (K: share)
    deep16        9            1492       25..93      100 %       2461        1.96 %       1: 2.15 %  4: 3.09 %  24: 4.29 %
    thin16       27            1315       74..229      33 %          0        2.55 %       1: 3.11 %  4: 4.74 %  (24: 13.4 %)
    t12          12             934       26..108     100 %          0        1.45 %       1: 1.71 %  4: 3.09 %
    t8           30             670       29..116     100 %       1089        1.33 %       1: 1.52 %  4: 2.40 %  24: 4.80 %
    t4           99             200       29..81       28 %          0        0.63 %       1: 0.77 %  4: 1.47 %  24: 4.34 %
    holes16      30 (12)         72        0..12        0 %          0        0.00 %       1: 0.05 %  4: 0.09 %  24, 48: 0 %
    holes8       90 (30)         40        0..12        0 %          0        0.00 %       1: 0.05 %  4: 0.09 %  24: 0 %

thin16 at K = 24 is over the cap and therefore not a case. In the holes cases 38 % of the pixels have no contributor and 63 %
fewer than 4. Windows of the indices op (RANGES, in order): deep16 1.89 / 1.89 / 2.84 / 0 %, thin16 0.27 / 0.57 / 1.83 / 0 %,
t8 0 / 1.01 / 2.27 / 0 %. A share can move by a pixel between machines (numpy's exp is not the same everywhere)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from _util import make_scene

ALPHA_THRESHOLD = 1.0 / 255.0
MAX_ALPHA = 0.99
T_THRESHOLD = 1e-4

# ---- margins of the decided flag (relative) --------------------------------------------------------------------------------
# alpha against 1/255: the staged base-2 form of the kernels is documented (csrc/raster3d.hpp) as ~1e-6 relative on alpha, and
# fp32 rounding of dx, dy about the tile centre adds at most ~1e-5.
ALPHA_MARGIN = 1e-4
# T (1 - alpha) against 1e-4: per step the fp32 update is off by <= ~1e-5 alpha; over a walk that sums to ~1e-5 ln(1 / T),
# ~1e-4 at saturation.
T_MARGIN = 1e-3
# sigma against 0, relative to |a dx^2 / 2| + |c dy^2 / 2| + |b dx dy| (the terms whose fp32 roundings do not cancel)
SIGMA_MARGIN = 1e-5
# top-K: every `w > w_min` of the rule, and the gap between the two weakest kept slots when one of them is replaced; the
# error of alpha T is that of alpha plus that of T, well below
TOPK_MARGIN = 1e-3

WALK_UNDECIDED_CAP = 0.05
TOPK_UNDECIDED_CAP = 0.10

# ---- cases -----------------------------------------------------------------------------------------------------------------
# N, C, W, H, tile size, scale range, seed; indefinite = share of rows whose conic gets b = +-1.5 sqrt(a c) (sigma < 0 on part
# of the plane); opacity = factor on the opacities; holes = radii zeroed where mean.x + radius.x > 2 W / 3 (empty tiles)
CASES = {
    "deep16": dict(N=4000, C=1, W=44, H=36, ts=16, scales=(0.05, 0.4), seed=11, indefinite=0.02),
    "thin16": dict(N=4000, C=3, W=44, H=36, ts=16, scales=(0.05, 0.4), seed=11, opacity=0.3),
    "t12": dict(N=3000, C=1, W=44, H=36, ts=12, scales=(0.05, 0.4), seed=12),
    "t8": dict(N=3000, C=1, W=44, H=36, ts=8, scales=(0.05, 0.4), seed=13, indefinite=0.02),
    "t4": dict(N=1500, C=1, W=42, H=34, ts=4, scales=(0.05, 0.3), seed=14),
    "holes16": dict(N=600, C=2, W=72, H=40, ts=16, scales=(0.02, 0.1), seed=15, holes=True),
    "holes8": dict(N=600, C=2, W=72, H=40, ts=8, scales=(0.02, 0.1), seed=15, holes=True),
}
CASE_NAMES = tuple(CASES)
PACKED_CASES = ("deep16", "t8", "holes16")
SPARSE_CASES = ("t12", "t8", "t4", "holes8")
STATS_CASES = ("deep16", "t8", "holes16")
RANGE_CASES = ("deep16", "thin16", "t8")
TOPK = {"deep16": (1, 4, 24), "thin16": (1, 4), "t12": (1, 4), "t8": (1, 4, 24), "t4": (1, 4, 24), "holes16": (1, 4, 24, 48),
        "holes8": (1, 4, 24)}
TOPK_PAIRS = tuple((n, k) for n in CASE_NAMES for k in TOPK[n])
# at 256 threads per tile the top-K scratch is 11264 + 3072 K bytes of LDS: 48 is the last K that fits, 49 the first refused
TOPK_LAST_FITTING, TOPK_FIRST_REFUSED = 48, 49
# windows of the indices op, in batches of tile_size^2 list entries; each starts from the walk's transmittance after the one
# before it. The last lies beyond every list.
FULL_RANGE = (0, 10 ** 6)
RANGES = ((0, 1), (1, 3), (3, 10 ** 6), (10 ** 6, 10 ** 6 + 5))


def _oracle():
    from oracle import oracle

    return oracle


@functools.lru_cache(maxsize=None)
def case(name):
    """CPU tensors of one case (shared: do not modify): means2d [C, N, 2], conics [C, N, 3], opacities [C, N], radii, depths,
    offsets int32 [C, th, tw], flatten_ids int32 [M], and the geometry W, H, ts, tw, th, C, N."""
    O = _oracle()
    p = CASES[name]
    sc, W, H = make_scene(N=p["N"], C=p["C"], width=p["W"], height=p["H"], seed=p["seed"], scale_range=p["scales"])
    opac = sc["opacities"] * p.get("opacity", 1.0)
    rad, m2, d, con, _ = (t[0] if t is not None else None for t in O.fully_fused_projection(
        sc["means"][None], None, sc["quats"][None], sc["scales"][None], sc["viewmats"][None], sc["Ks"][None], W, H,
        opacities=opac[None]))
    C, N, ts = p["C"], p["N"], p["ts"]
    rng = np.random.default_rng(p["seed"])
    con = con.clone()
    if p.get("indefinite"):
        pick = torch.from_numpy(rng.random((C, N)) < p["indefinite"])
        sign = torch.from_numpy(np.where(rng.random((C, N)) < 0.5, -1.0, 1.0).astype(np.float32))
        b = 1.5 * sign * torch.sqrt(con[..., 0] * con[..., 2])
        con[..., 1] = torch.where(pick, b, con[..., 1])
    rad = rad.clone()
    if p.get("holes"):
        rad[(m2[..., 0] + rad[..., 0].float()) > 2.0 * W / 3.0] = 0
    op = opac[None].expand(C, N).contiguous()
    tw, th = math.ceil(W / ts), math.ceil(H / ts)
    _, ids, fl = O.isect_tiles(m2, rad, d, ts, tw, th)
    off = O.isect_offset_encode(ids, C, tw, th)
    return SimpleNamespace(name=name, means2d=m2.contiguous(), conics=con.contiguous(), opacities=op, radii=rad.contiguous(),
                           depths=d.contiguous(), offsets=off, flatten_ids=fl, W=W, H=H, ts=ts, tw=tw, th=th, C=C, N=N)


@functools.lru_cache(maxsize=None)
def packed_case(name):
    """The same Gaussians as packed rows (the visible ones): means2d [nnz, 2], ..., image_ids / gaussian_ids [nnz], and the
    intersection of the packed rows - list for list the dense one (asserted in tests/test_query_cases.py)."""
    O = _oracle()
    cs = case(name)
    ci, gi = torch.where((cs.radii > 0).all(-1))
    rows = ci * cs.N + gi
    m2 = cs.means2d.reshape(-1, 2)[rows].contiguous()
    con = cs.conics.reshape(-1, 3)[rows].contiguous()
    op, d = cs.opacities.reshape(-1)[rows].contiguous(), cs.depths.reshape(-1)[rows].contiguous()
    rad = cs.radii.reshape(-1, 2)[rows].contiguous()
    _, ids, fl = O.isect_tiles(m2, rad, d, cs.ts, cs.tw, cs.th, image_ids=ci, n_images=cs.C)
    off = O.isect_offset_encode(ids, cs.C, cs.tw, cs.th)
    return SimpleNamespace(means2d=m2, conics=con, opacities=op, image_ids=ci, gaussian_ids=gi, rows=rows, offsets=off,
                           flatten_ids=fl)


def list_bounds(cs):
    """(start, end) of every tile's list, int64 [C * th * tw]."""
    start = cs.offsets.reshape(-1).numpy().astype(np.int64)
    return start, np.concatenate([start[1:], [cs.flatten_ids.numel()]])


# ---- the float64 walk ------------------------------------------------------------------------------------------------------
def _walk_tile(px, py, mx, my, ca, cb, cc, op, T0):
    """Pixels [P] of one tile against its list window [L], all float64. Returns per pixel: contributes [P, L], weights
    [P, L], T after the walk, entries walked, decided, walked candidates with sigma < 0."""
    P, L = px.shape[0], mx.shape[0]
    dx, dy = mx[None, :] - (px[:, None] + 0.5), my[None, :] - (py[:, None] + 0.5)
    ta, tb, tc = 0.5 * ca[None] * dx * dx, cb[None] * dx * dy, 0.5 * cc[None] * dy * dy
    sigma = ta + tc + tb
    with np.errstate(over="ignore"):
        alpha = np.minimum(MAX_ALPHA, op[None] * np.exp(-sigma))
    sig_ok = sigma >= 0.0
    valid = sig_ok & (alpha >= ALPHA_THRESHOLD)
    T_after = T0[:, None] * np.cumprod(np.where(valid, 1.0 - alpha, 1.0), axis=1)  # if the pixel has not stopped before
    T_before = np.concatenate([T0[:, None], T_after[:, :-1]], axis=1)
    stops = valid & (T_after <= T_THRESHOLD)
    stop = np.where(stops.any(1), stops.argmax(1), L)  # index of the stopping entry
    j = np.arange(L)[None, :]
    undecided = (np.abs(sigma) <= SIGMA_MARGIN * (np.abs(ta) + np.abs(tb) + np.abs(tc)))
    undecided |= sig_ok & (np.abs(alpha - ALPHA_THRESHOLD) <= ALPHA_MARGIN * ALPHA_THRESHOLD)
    undecided |= valid & (np.abs(T_after - T_THRESHOLD) <= T_MARGIN * T_THRESHOLD)
    decided = ~(undecided & (j <= stop[:, None])).any(1)
    contributes = valid & (j < stop[:, None])
    T_end = np.where(stop < L, T_before[np.arange(P), np.minimum(stop, L - 1)], T_after[:, -1])
    return contributes, alpha * T_before, T_end, np.minimum(stop + 1, L), decided, (~sig_ok & (j <= stop[:, None])).sum(1)


def _window(name, part):
    if part == "full":
        return FULL_RANGE, None
    k = int(part)
    return RANGES[k], (None if k == 0 else walk(name, k - 1).T_end.astype(np.float32))


@functools.lru_cache(maxsize=None)
def walk(name, part="full"):
    """The reference walk of one case over one window: part "full" = every batch from T0 = 1; part k = RANGES[k] from the
    transmittance after part k - 1 rounded to fp32 (T0, float32 [C * H * W], is what both sides are given).
    Arrays over the pixels in (image, row, column) order: ids int64 [P, max count] (-1 behind the count), weights float64
    (0 behind it), count, alpha = 1 - T, T_end, walked (window entries up to and including the stopping one), list_len (of the
    window), decided, sigma_neg (walked candidates with sigma < 0: the branch `e > lo` of the kernels). Shared: do not
    modify."""
    cs = case(name)
    (rs, re), T0 = _window(name, part)
    P = cs.C * cs.H * cs.W
    T0 = np.ones(P, dtype=np.float32) if T0 is None else T0
    m2, con = cs.means2d.reshape(-1, 2).numpy().astype(np.float64), cs.conics.reshape(-1, 3).numpy().astype(np.float64)
    op, fl = cs.opacities.reshape(-1).numpy().astype(np.float64), cs.flatten_ids.numpy().astype(np.int64)
    start, end = list_bounds(cs)
    bs = cs.ts * cs.ts
    count, walked, list_len = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P, np.int64)
    T_end, decided, sigma_neg = T0.astype(np.float64), np.ones(P, bool), np.zeros(P, np.int64)
    per_tile = []
    for blk in range(cs.C * cs.th * cs.tw):
        img, ty, tx = blk // (cs.th * cs.tw), (blk // cs.tw) % cs.th, blk % cs.tw
        ys, xs = np.meshgrid(np.arange(ty * cs.ts, min((ty + 1) * cs.ts, cs.H)),
                             np.arange(tx * cs.ts, min((tx + 1) * cs.ts, cs.W)), indexing="ij")
        pix = (img * cs.H + ys.reshape(-1)) * cs.W + xs.reshape(-1)
        lo, hi = start[blk] + bs * rs, min(end[blk], start[blk] + bs * re)
        if hi <= lo:
            continue
        rows = fl[lo:hi]
        list_len[pix] = hi - lo
        contributes, w, T_end[pix], walked[pix], decided[pix], sigma_neg[pix] = _walk_tile(
            xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64), m2[rows, 0], m2[rows, 1], con[rows, 0],
            con[rows, 1], con[rows, 2], op[rows], T0[pix].astype(np.float64))
        count[pix] = contributes.sum(1)
        per_tile.append((pix, rows % cs.N, contributes, w))
    kmax = int(count.max())
    ids, wts = np.full((P, kmax), -1, np.int64), np.zeros((P, kmax), np.float64)
    for pix, gids, contributes, w in per_tile:
        p, j = np.nonzero(contributes)  # row-major: list order inside a pixel
        slot = (np.cumsum(contributes, axis=1) - 1)[p, j]
        ids[pix[p], slot], wts[pix[p], slot] = gids[j], w[p, j]
    return SimpleNamespace(ids=ids, weights=wts, count=count, alpha=1.0 - T_end, T_end=T_end, walked=walked, list_len=list_len,
                           decided=decided, sigma_neg=sigma_neg, T0=T0)


@functools.lru_cache(maxsize=None)
def topk(name, K):
    """The top-K rule on the full walk: (ids int64 [P, K], weights float64 [P, K], decided [P])."""
    wk = walk(name)
    P, D = wk.ids.shape
    ar = np.arange(P)
    sw, sd, si = np.zeros((P, K)), np.full((P, K), 2 ** 32 - 1, np.int64), np.full((P, K), -1, np.int64)
    undecided = np.zeros(P, bool)
    for d in range(D):
        live = wk.count > d
        w = wk.weights[:, d]
        kmin = sw.argmin(1)  # the first weakest
        wmin = sw[ar, kmin]
        full = live & (wmin > 0.0)  # an unused slot is the weakest on both sides, and any weight beats it
        undecided |= full & (np.abs(w - wmin) <= TOPK_MARGIN * wmin)
        if K > 1:
            second = np.partition(sw, 1, axis=1)[:, 1]
            undecided |= full & (w > wmin) & (second - wmin <= TOPK_MARGIN * wmin)
        rep = live & (w > wmin)
        sw[ar[rep], kmin[rep]], sd[ar[rep], kmin[rep]], si[ar[rep], kmin[rep]] = w[rep], d, wk.ids[rep, d]
    order = np.argsort(sd, axis=1, kind="stable")
    return np.take_along_axis(si, order, 1), np.take_along_axis(sw, order, 1), wk.decided & ~undecided


# ---- sparse pixel sets -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sparse_set(name, kind="many"):
    """A pixel set of one case and its layout, built with the oracle: kind "many" = some pixels of about 70 % of the tiles -
    a number of active tiles that is no multiple of 8, empty tiles among them where the case has any; kind "one" = one pixel.
    Returns pixels int64 [P, 2] (row, column), image_ids int64 [P], the layout (numpy) and offsets / flatten_ids (torch)."""
    O = _oracle()
    cs = case(name)
    rng = np.random.default_rng(1000 + cs.ts)
    n_tiles = cs.C * cs.th * cs.tw
    start, end = list_bounds(cs)
    if kind == "one":
        tiles = np.array([n_tiles // 2])
    else:
        tiles = np.flatnonzero(rng.random(n_tiles) < 0.7)
        empty = np.flatnonzero(end == start)
        if empty.size:
            tiles = np.union1d(tiles, empty[:2])
        if tiles.size % 8 == 0:
            tiles = tiles[:-1]
    px, im = [], []
    for t in tiles:
        img, ty, tx = t // (cs.th * cs.tw), (t // cs.tw) % cs.th, t % cs.tw
        ys, xs = np.meshgrid(np.arange(ty * cs.ts, min((ty + 1) * cs.ts, cs.H)),
                             np.arange(tx * cs.ts, min((tx + 1) * cs.ts, cs.W)), indexing="ij")
        cand = np.stack([ys.reshape(-1), xs.reshape(-1)], -1)
        k = 1 if kind == "one" else int(rng.integers(1, cand.shape[0] + 1))
        px.append(cand[rng.permutation(cand.shape[0])[:k]])
        im.append(np.full(k, img))
    px, im = np.concatenate(px), np.concatenate(im)
    shuffle = rng.permutation(px.shape[0])  # the caller's order is not the layout's
    px, im = px[shuffle].astype(np.int64), im[shuffle].astype(np.int64)
    act, tmask, pmask, cum, pmap = O.sparse_tile_layout(px, im, cs.C, cs.ts, cs.tw, cs.th)
    off, fl = O.isect_tiles_sparse(cs.means2d, cs.radii, cs.depths, tmask, act, cs.C, cs.ts, cs.tw, cs.th)
    return SimpleNamespace(pixels=px, image_ids=im, active_tiles=act, tile_mask=tmask, pixel_mask=pmask, pixel_cumsum=cum,
                           pixel_map=pmap, offsets=off, flatten_ids=fl)
