"""Ordering of the splats on the square parameter grid before PNG compression.

The reference sorts with PLAS, *Parallel Linear Assignment Sorting* (``plas.sort_with_plas``, github.com/fraunhoferhhi/PLAS,
un-pinned in the reference; gsplat/compression/sort.py:22-64), a third-party package that is not part of this image. Any
permutation is a valid input of the codec (decompression never needs it back), the ordering only decides how well the PNG
filters predict a pixel from its neighbours. ``sort_splats(method="auto")`` therefore picks, in this order:

1. the ``plas`` package when it is importable - same call, same keys as the reference;
2. the native grid sort of this module, ``plas_sort``, when the feature matrix is one the kernels of csrc/plas.hip serve
   (``_plas_fused_ok``: float32 on a ROCm device, at most 32 channels, fewer than 2^31 splats);
3. otherwise (CPU tensors) a space-filling curve: splats ordered by the Morton code of their (log-transformed) positions
   are written along the Z-order traversal of the grid cells. It looks at the positions alone and needs nothing beyond
   torch; it recovers part of the gain of the assignment search.

``method="plas"`` runs the native sort wherever the tensors live (the torch composition on the CPU), ``method="morton"``
forces the curve.

The native sort is a block-assignment sort in the spirit of PLAS ("Compact 3D Scene Representation via Self-Organizing
Gaussian Grids"); it does not reproduce the package's permutation. One step blurs the grid (``plas_blur_torch``), cuts it
into b x b blocks at a pseudo-random offset, deals each block's cells pseudo-randomly into groups of four (``plas_groups``,
integer arithmetic only) and gives each group's four rows to its four cells so that the summed squared distance to the
blurred grid is smallest (``plas_step_torch``: all 24 assignments, the identity wins ties). ``plas_sort_torch`` runs the
steps over a shrinking blur radius. The ``*_torch`` functions are the definition and run on any device; ``plas_sort`` runs
the same loop over gsx_plas_blur / gsx_plas_step where ``_plas_fused_ok`` holds, with one host read (improvement, total) per
step. The two share every integer decision and differ in float near-ties and in the rounding of the blur.
"""
from __future__ import annotations

import itertools
from typing import Dict, Tuple

import torch
from torch import Tensor


def _spread_bits(v: Tensor, stride: int, bits: int) -> Tensor:
    """bit i of v -> bit i * stride (int64)."""
    out = torch.zeros_like(v)
    for i in range(bits):
        out |= ((v >> i) & 1) << (i * stride)
    return out


def morton_order_3d(points: Tensor, bits: int = 16) -> Tensor:
    """Permutation that sorts [N, 3] points by the Morton code of their coordinates quantised to `bits` bits per axis."""
    lo, hi = points.amin(0), points.amax(0)
    q = ((points - lo) / (hi - lo).clamp_min(1e-30) * (2**bits - 1)).round().to(torch.int64).clamp_(0, 2**bits - 1)
    code = _spread_bits(q[:, 0], 3, bits) | (_spread_bits(q[:, 1], 3, bits) << 1) | (_spread_bits(q[:, 2], 3, bits) << 2)
    return torch.argsort(code, stable=True)


def z_curve_cells(side: int, device=None) -> Tensor:
    """The cells of a side x side grid (flat row-major indices) in Z-order."""
    ys, xs = torch.meshgrid(torch.arange(side, device=device), torch.arange(side, device=device), indexing="ij")
    bits = max(1, (side - 1).bit_length())
    code = _spread_bits(xs.reshape(-1), 2, bits) | (_spread_bits(ys.reshape(-1), 2, bits) << 1)
    return torch.argsort(code, stable=True)


# ---- the integer definition of a step's groups (csrc/plas.hip restates it in uint32 arithmetic) ---------------------------

_M32 = 0xFFFFFFFF
_GOLD = 0x9E3779B9
PLAS_MAX_C = 32  # csrc/plas.hip


def _mul32(x, c: int):
    """x * c mod 2^32 for x in [0, 2^32) (Python int or int64 tensor) without leaving 63 bits."""
    return (x * (c & 0xFFFF) + (((x * (c >> 16)) & 0xFFFF) << 16)) & _M32


def _mix32(x):
    """The xorshift-multiply finaliser (constants 0x7FEB352D, 0x846CA68B) on a Python int or an int64 tensor in [0, 2^32)."""
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7FEB352D)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846CA68B)
    return x ^ (x >> 16)


def _plas_step_hash(seed: int, t: int) -> int:
    """The 32-bit hash of (seed, t) that a step's block offset and block keys derive from."""
    return _mix32((_mix32(seed & _M32) + (t & _M32)) & _M32)


def plas_offset(b: int, seed: int, t: int) -> Tuple[int, int]:
    """(oy, ox), each in [0, b): where step t cuts the grid into b x b blocks."""
    h = _plas_step_hash(seed, t)
    return h & (b - 1), (h >> 16) & (b - 1)


def plas_slot_cells(b: int, seed: int, t: int, bid: Tensor) -> Tensor:
    """int64 [len(bid), b * b]: the cell (ly * b + lx inside the block) of every slot of the blocks `bid` in step t - a keyed
    bijection on m = 2 log2(b) bits. Three rounds of: multiply by an odd key, x ^= x >> max(1, m / 2), add a key, all mod 2^m;
    the six keys are hashed from (seed, t, bid)."""
    m = 2 * (b.bit_length() - 1)
    mask, shift = (1 << m) - 1, max(1, m // 2)
    kb = _mix32((_plas_step_hash(seed, t) + _mul32((bid.to(torch.int64) + 1) & _M32, _GOLD)) & _M32)[:, None]
    x = torch.arange(b * b, dtype=torch.int64, device=bid.device)[None, :]
    for rnd in range(3):
        mul = (_mix32((kb + (2 * rnd + 1)) & _M32) | 1) & mask
        add = _mix32((kb + (2 * rnd + 2)) & _M32) & mask
        x = (x * mul) & mask
        x = x ^ (x >> shift)
        x = (x + add) & mask
    return x


def plas_groups(H: int, W: int, b: int, seed: int, t: int, device=None) -> Tensor:
    """int64 [G, 4]: the flat cell indices of the groups of step t. The grid is cut into b x b blocks (b a power of two >= 2) at
    the offset `plas_offset`; only complete blocks take part, (H - oy) // b by (W - ox) // b of them, numbered row-major; group g
    of block bid is its slots 4 g .. 4 g + 3 (`plas_slot_cells`), position j of the group is slot 4 g + j. Integer arithmetic
    only."""
    if b < 2 or b & (b - 1):
        raise ValueError(f"plas_groups: b = {b} is not a power of two >= 2")
    oy, ox = plas_offset(b, seed, t)
    nby, nbx = max(0, (H - oy) // b), max(0, (W - ox) // b)
    if nby * nbx == 0:
        return torch.empty((0, 4), dtype=torch.int64, device=device)
    bid = torch.arange(nby * nbx, dtype=torch.int64, device=device)
    local = plas_slot_cells(b, seed, t, bid)
    lb = b.bit_length() - 1
    y = (oy + (bid // nbx) * b)[:, None] + (local >> lb)
    x = (ox + (bid % nbx) * b)[:, None] + (local & (b - 1))
    return (y * W + x).reshape(-1, 4)


# ---- the float definition ------------------------------------------------------------------------------------------------------

def plas_blur_torch(grid: Tensor, r: int) -> Tensor:
    """[H, W, C] -> the box mean of width 2 r + 1 along W, then along H, with reflect borders (no edge repeat).
    1 <= r <= min(H, W) - 1."""
    H, W, _ = grid.shape
    if not 1 <= r <= min(H, W) - 1:
        raise ValueError(f"plas_blur_torch: r = {r} outside [1, min(H, W) - 1] for a {H} x {W} grid")
    x = grid.permute(2, 0, 1)[None]
    pad, pool = torch.nn.functional.pad, torch.nn.functional.avg_pool2d
    x = pool(pad(x, (r, r, 0, 0), mode="reflect"), (1, 2 * r + 1), stride=1)
    x = pool(pad(x, (0, 0, r, r), mode="reflect"), (2 * r + 1, 1), stride=1)
    return x[0].permute(1, 2, 0).contiguous()


_PERMS = tuple(itertools.permutations(range(4)))  # lexicographic; p[j] = the row that moves to position j; [0] = identity


def _step_values(grid: Tensor, target: Tensor, index: Tensor, b: int, seed: int, t: int) -> Tensor:
    H, W, C = grid.shape
    g, tg, ix = grid.view(H * W, C), target.reshape(H * W, C), index.view(H * W)
    groups = plas_groups(H, W, b, seed, t, device=grid.device)
    if groups.shape[0] == 0:
        return torch.zeros(2, dtype=torch.float32, device=grid.device)
    x, tt = g[groups], tg[groups]  # [G, 4, C]
    diff = x[:, :, None, :] - tt[:, None, :, :]
    cost = (diff * diff).sum(-1)  # [G, 4 rows, 4 positions]
    perms = torch.tensor(_PERMS, dtype=torch.int64, device=grid.device)  # [24, 4]
    pos = torch.arange(4, device=grid.device)
    picked = cost[:, perms, pos]  # [G, 24, 4]: cost[p[j]][j]
    totals = ((picked[..., 0] + picked[..., 1]) + picked[..., 2]) + picked[..., 3]
    best = totals.min(dim=1).values
    which = torch.arange(24, device=grid.device).expand_as(totals)
    chosen = torch.where(totals == best[:, None], which, torch.full_like(which, 24)).min(dim=1).values  # lowest minimal index
    chosen = torch.where(chosen < 24, chosen, torch.zeros_like(chosen))  # NaN totals: nothing compares equal, stay put
    move = perms[chosen]  # [G, 4]
    g[groups] = torch.gather(x, 1, move[:, :, None].expand(-1, -1, C))
    ix[groups] = torch.gather(ix[groups], 1, move)
    identity = totals[:, 0]
    final = totals.gather(1, chosen[:, None])[:, 0]
    return torch.stack([(identity - final).sum(), identity.sum()])


def plas_step_torch(grid: Tensor, target: Tensor, index: Tensor, b: int, seed: int, t: int) -> Tuple[float, float]:
    """One assignment step on grid [H, W, C] (float32) and index [H, W] (int64), both contiguous and changed in place, against
    `target` [H, W, C]. For each group of `plas_groups` with rows x_0 .. x_3 and targets t_0 .. t_3 at its four positions:
    cost[i][j] = sum_c (x_i[c] - t_j[c])^2 in float32; of the 24 permutations in lexicographic order (p[j] = the row that moves
    to position j, total_p = sum_j cost[p[j]][j]) the one with the lowest total moves, the lowest index among equal totals -
    the identity wins ties. Returns (improvement, total): the sums over the groups of total_identity - total_chosen and of
    total_identity."""
    imp, tot = _step_values(grid, target, index, b, seed, t).tolist()
    return imp, tot


def _pow2floor(v: int) -> int:
    return 1 << (v.bit_length() - 1)


def _pow2ceil(v: int) -> int:
    return 1 << max(0, (v - 1).bit_length())


def _plas_schedule(H: int, W: int, radius_decay: float):
    """(r, b) per radius: rf = min(H, W) / 2 - 1, r = floor(rf) until r < 1, rf *= radius_decay."""
    rf = min(H, W) / 2 - 1
    while int(rf) >= 1:
        r = int(rf)
        yield r, min(_pow2floor(min(H, W)), max(4, _pow2ceil(r + 1)))
        rf *= radius_decay


def _plas_loop(H, W, seed, improvement_break, radius_decay, max_steps_per_radius, verbose, step) -> int:
    t = 0
    for r, b in _plas_schedule(H, W, radius_decay):
        for _ in range(max_steps_per_radius):
            improvement, total = step(r, b, t)
            t += 1
            if not improvement > improvement_break * total:
                break
        if verbose:
            print(f"plas_sort: radius {r}, block {b}, {t} steps so far, last improvement {improvement:.3e} of {total:.3e}")
    return t


def _check_sort_args(feats: Tensor, H: int, W: int, radius_decay: float) -> None:
    if feats.dim() != 2 or feats.shape[0] != H * W:
        raise ValueError(f"plas_sort: feats {tuple(feats.shape)} do not fill a {H} x {W} grid")
    if not 0 < radius_decay < 1:
        raise ValueError(f"plas_sort: radius_decay = {radius_decay} outside (0, 1)")


def plas_sort_torch(feats: Tensor, H: int, W: int, seed: int = 0, improvement_break: float = 1e-4, radius_decay: float = 0.9,
                    max_steps_per_radius: int = 64, verbose: bool = False) -> Tensor:
    """The grid sort composed of tensor operations, on feats' device: int64 order [N], cell k of the H x W grid holds input row
    order[k]. Per radius r (`_plas_schedule`) up to `max_steps_per_radius` steps of blur with r + `plas_step_torch`, left when
    improvement <= improvement_break * total. A grid with min(H, W) < 4 has no radius >= 1: the identity order."""
    _check_sort_args(feats, H, W, radius_decay)
    grid = feats.detach().float().reshape(H, W, -1).clone()
    index = torch.arange(H * W, dtype=torch.int64, device=feats.device).reshape(H, W)

    def step(r, b, t):
        return plas_step_torch(grid, plas_blur_torch(grid, r), index, b, seed, t)

    _plas_loop(H, W, seed, improvement_break, radius_decay, max_steps_per_radius, verbose, step)
    return index.reshape(-1)


def _plas_fused_ok(feats: Tensor) -> bool:
    """What csrc/plas.hip serves: float32 rows [N, C] on a ROCm device, 1 <= C <= 32, N < 2^31."""
    return (feats.device.type == "cuda" and feats.dtype == torch.float32 and feats.dim() == 2
            and 1 <= feats.shape[1] <= PLAS_MAX_C and feats.shape[0] < 2 ** 31)


fused_sorts = 0  # how many times the kernels ran a whole sort in this process (tests assert the path through it)
last_steps = 0   # steps of the most recent plas_sort over the kernels


def _blur_fused(grid: Tensor, r: int, target: Tensor = None, work: Tensor = None) -> Tensor:
    """gsx_plas_blur on a contiguous float32 device grid [H, W, C]: `plas_blur_torch` by sliding window sums."""
    from .. import _cabi

    H, W, c = grid.shape
    with torch.cuda.device(grid.device):
        target = torch.empty_like(grid) if target is None else target
        if work is None:
            work = torch.empty(_cabi.query("gsx_plas_workspace_bytes", H, W, c), dtype=torch.uint8, device=grid.device)
        _cabi.call("gsx_plas_blur", grid, H, W, c, r, target, work)
    return target


def _step_fused(grid: Tensor, target: Tensor, index: Tensor, b: int, seed: int, t: int, partials: Tensor = None,
                result: Tensor = None) -> Tensor:
    """gsx_plas_step, in place on the contiguous device tensors grid [H, W, C] float32 and index [H, W] int32: `plas_step_torch`
    with the 16 lanes of a DPP row per group. Returns the device tensor (improvement, total)."""
    from .. import _cabi

    H, W, c = grid.shape
    with torch.cuda.device(grid.device):
        if partials is None:
            partials = torch.empty(_cabi.query("gsx_plas_partials_floats", H, W), dtype=torch.float32, device=grid.device)
        result = torch.empty(2, dtype=torch.float32, device=grid.device) if result is None else result
        _cabi.call("gsx_plas_step", grid, target, index, H, W, c, b, seed & _M32, t & _M32, partials, result)
    return result


def _plas_sort_fused(feats, H, W, seed, improvement_break, radius_decay, max_steps_per_radius, verbose) -> Tensor:
    from .. import _cabi

    global fused_sorts, last_steps
    n, c = feats.shape
    dev = feats.device
    grid = feats.detach().contiguous().clone().reshape(H, W, c)
    index = torch.arange(n, dtype=torch.int32, device=dev).reshape(H, W)
    last_steps = 0
    if n:
        with torch.cuda.device(dev):
            target = torch.empty_like(grid)
            work = torch.empty(_cabi.query("gsx_plas_workspace_bytes", H, W, c), dtype=torch.uint8, device=dev)
            partials = torch.empty(_cabi.query("gsx_plas_partials_floats", H, W), dtype=torch.float32, device=dev)
            result = torch.empty(2, dtype=torch.float32, device=dev)

        def step(r, b, t):
            _blur_fused(grid, r, target, work)
            return _step_fused(grid, target, index, b, seed, t, partials, result).tolist()  # the one host read of the step

        last_steps = _plas_loop(H, W, seed, improvement_break, radius_decay, max_steps_per_radius, verbose, step)
    fused_sorts += 1
    return index.reshape(-1).to(torch.int64)


def plas_sort(feats: Tensor, H: int, W: int, seed: int = 0, improvement_break: float = 1e-4, radius_decay: float = 0.9,
              max_steps_per_radius: int = 64, verbose: bool = False) -> Tensor:
    """`plas_sort_torch` over the kernels of csrc/plas.hip where `_plas_fused_ok(feats)` holds (float32 on a ROCm device,
    C <= 32, N < 2^31): the same schedule and the same groups, gsx_plas_blur + gsx_plas_step per step, and one host read per
    step - the two floats improvement and total. Everything else is `plas_sort_torch`."""
    _check_sort_args(feats, H, W, radius_decay)
    if _plas_fused_ok(feats):
        return _plas_sort_fused(feats, H, W, seed, improvement_break, radius_decay, max_steps_per_radius, verbose)
    return plas_sort_torch(feats, H, W, seed, improvement_break, radius_decay, max_steps_per_radius, verbose)


_SORT_KEYS = ("means", "quats", "scales", "opacities", "sh0")


def _sort_features(splats: Dict[str, Tensor]) -> Tensor:
    """The reference's sort keys side by side, [N, C] float32, each channel min-max normalised to [0, 1] (constant -> 0)."""
    n = len(splats["means"])
    feats = torch.cat([splats[k].detach().reshape(n, -1).float() for k in _SORT_KEYS if k in splats], dim=-1)
    lo, hi = feats.amin(0), feats.amax(0)
    span = hi - lo
    return torch.where(span > 0, (feats - lo) / span.clamp_min(1e-38), torch.zeros_like(feats))


def sort_splats(splats: Dict[str, Tensor], verbose: bool = True, method: str = "auto", seed: int = 0) -> Dict[str, Tensor]:
    """Reorder every field of `splats` (in place, and returned) for the square grid (reference sort.py:22). `method`: "auto"
    (the plas package if importable, else the native sort where the kernels serve the features, else the Morton layout),
    "plas" (the native sort on whatever device holds the tensors) or "morton"."""
    if method not in ("auto", "plas", "morton"):
        raise ValueError(f"sort_splats: method = {method!r}, expected 'auto', 'plas' or 'morton'")
    n = len(splats["means"])
    side = int(n**0.5)
    assert side * side == n, "Must be a perfect square"
    sort_with_plas = None
    if method == "auto":
        try:
            from plas import sort_with_plas
        except ImportError:
            pass
    feats = None
    if sort_with_plas is None and method != "morton" and n > 0:
        feats = _sort_features(splats)
        if method == "auto" and not _plas_fused_ok(feats):
            feats = None
    if sort_with_plas is not None:
        keys = ["means", "quats", "scales", "opacities"] + (["sh0"] if "sh0" in splats else [])
        feats = torch.cat([splats[k].reshape(n, -1) for k in keys], dim=-1)
        shuffle = torch.randperm(n, device=feats.device)
        grid = feats[shuffle].reshape(side, side, -1)
        _, idx = sort_with_plas(grid.permute(2, 0, 1), improvement_break=1e-4, verbose=verbose)
        order = shuffle[idx.squeeze().flatten()]
    elif feats is not None:
        shuffle = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(feats.device)
        order = shuffle[plas_sort(feats[shuffle], side, side, seed=seed, improvement_break=1e-4, verbose=verbose)]
    else:
        means = splats["means"].detach().float()
        by_position = morton_order_3d(means)
        order = torch.empty(n, dtype=torch.int64, device=means.device)
        order[z_curve_cells(side, means.device)] = by_position
    for k, v in splats.items():
        splats[k] = v[order.to(v.device)]
    return splats
