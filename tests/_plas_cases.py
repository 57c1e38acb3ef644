"""Shared by tests/test_plas_sort.py and tests/test_gpu_plas_sort.py: inputs for the grid sort of gsplat_amd.compression.sort
(csrc/plas.hip), float64 evaluations of what a step and a blur should give, and the two measures of an ordering (roughness of
the grid, PNG bytes). Every generator runs on the CPU."""
import functools
import itertools
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24  # unit roundoff of float32
PERMS = torch.tensor(list(itertools.permutations(range(4))), dtype=torch.int64)  # lexicographic, [0] = identity


@functools.lru_cache(maxsize=None)
def fixture_splats(side):
    """side^2 splats with the garden scene's real points and colours (tests/golden/garden_scene.npz, a seeded draw of rows) and
    the other fields smooth functions of position and colour plus noise: fields correlated with one another the way a trained
    scene's are. Cached: treat as read-only."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "garden_scene.npz"))
    n = side * side
    g = torch.Generator().manual_seed(4000 + side)
    pick = torch.randperm(len(z["means"]), generator=g)[:n]
    means = torch.from_numpy(z["means"]).float()[pick]
    rgb = torch.from_numpy(z["colors_u8"]).float()[pick] / 255.0
    pos = (means - means.mean(0)) / means.std(0)
    mix = lambda rows, cols: torch.randn(rows, cols, generator=g)  # noqa: E731
    noise = lambda cols, s: s * torch.randn(n, cols, generator=g)  # noqa: E731
    scales = -3.0 + 0.5 * torch.tanh(pos @ mix(3, 3)) + 0.3 * (rgb - 0.5) @ mix(3, 3) + noise(3, 0.1)
    quats = torch.tanh(pos @ mix(3, 4)) + 0.5 * (rgb - 0.5) @ mix(3, 4) + noise(4, 0.1)
    opacities = 2.0 * torch.tanh((pos @ mix(3, 1))[:, 0]) + (rgb.mean(1) - 0.5) + noise(1, 0.2)[:, 0]
    sh0 = ((rgb - 0.5) / 0.2820948)[:, None, :]
    return dict(means=means, scales=scales, quats=quats, opacities=opacities, sh0=sh0)


@functools.lru_cache(maxsize=None)
def fixture_features(side):
    """[side^2, 14] float32: the sort's features of `fixture_splats` (means log-transformed and quats normalised as
    PngCompression does before it sorts), per-channel min-max normalised, rows shuffled with a seed. Cached: read-only."""
    from gsplat_amd.compression.png_compression import log_transform
    from gsplat_amd.compression.sort import _sort_features

    sp = dict(fixture_splats(side))
    sp["means"] = log_transform(sp["means"])
    sp["quats"] = torch.nn.functional.normalize(sp["quats"], dim=-1)
    feats = _sort_features(sp)
    return feats[torch.randperm(side * side, generator=torch.Generator().manual_seed(side))].contiguous()


def random_grid(H, W, C, seed=0):
    """Seeded uniform [0, 1) grid [H, W, C] float32."""
    return torch.rand(H, W, C, generator=torch.Generator().manual_seed(1_000_003 * H + 1_009 * W + 31 * C + seed))


def roughness(feats, order, H, W):
    """Mean absolute difference between neighbouring cells (along W and along H) of the grid that holds feats[order]."""
    grid = feats[order].reshape(H, W, -1).double()
    return float(((grid[:, 1:] - grid[:, :-1]).abs().mean() + (grid[1:] - grid[:-1]).abs().mean()) / 2)


def morton_order(means):
    """The layout sort_splats(method="morton") gives: int64 order [N] from the (log-transformed) positions."""
    from gsplat_amd.compression.sort import morton_order_3d, z_curve_cells

    n = len(means)
    order = torch.empty(n, dtype=torch.int64)
    order[z_curve_cells(int(n ** 0.5))] = morton_order_3d(means.float())
    return order


def png_bytes(directory):
    return sum(os.path.getsize(os.path.join(directory, f)) for f in os.listdir(directory) if f.endswith(".png"))


def blur_f64(grid, r):
    """The box mean of width 2 r + 1 along W then along H with reflect borders (no edge repeat), by direct window sums in
    float64."""
    H, W, _ = grid.shape

    def reflect(i, n):
        i = np.abs(i)
        return np.where(i >= n, 2 * (n - 1) - i, i)

    taps = np.arange(-r, r + 1)
    g = grid.double()
    g = g[:, torch.from_numpy(reflect(np.arange(W)[:, None] + taps[None, :], W))].mean(dim=2)  # [H, W, taps, C] -> [H, W, C]
    g = g[torch.from_numpy(reflect(np.arange(H)[:, None] + taps[None, :], H))].mean(dim=1)    # [H, taps, W, C] -> [H, W, C]
    return g


def blur_tolerance(grid, H, W, r):
    """2 (L + 1) u max|grid| per channel, L = max(H, W) + 2 r: a mean formed from float32 sums of at most L terms in any order is
    within L u max|x|, and there are two passes."""
    return 2.0 * (max(H, W) + 2 * r + 1) * U * grid.abs().amax(dim=(0, 1)).double()


def totals_f64(grid, target, groups):
    """[G, 24] float64: total_p = sum_j sum_c (x_p[j][c] - t_j[c])^2 for the 24 permutations in lexicographic order, of the
    float32 rows `grid` and `target` ([N, C]) at the cells `groups` [G, 4]."""
    x, t = grid.double()[groups], target.double()[groups]  # [G, 4, C]
    cost = ((x[:, :, None, :] - t[:, None, :, :]) ** 2).sum(-1)  # [G, rows, positions]
    return cost[:, PERMS, torch.arange(4)].sum(-1)


def chosen_permutation(index_before, index_after, groups):
    """[G] the index (into PERMS) of a permutation p with index_after[cell_j] == index_before[cell_p[j]] for every group; -1 where
    the four entries after are no permutation of the four before. The index values of a group must be distinct."""
    before, after = index_before[groups], index_after[groups]  # [G, 4]
    match = (before[:, PERMS] == after[:, None, :]).all(-1)  # [G, 24]
    which = torch.arange(24).expand_as(match)
    first = torch.where(match, which, torch.full_like(which, 24)).min(dim=1).values
    return torch.where(first < 24, first, torch.full_like(first, -1))
