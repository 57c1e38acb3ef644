"""GPU: the kernels of csrc/plas.hip (gsx_plas_blur, gsx_plas_step) against the torch definition of
gsplat_amd.compression.sort, and the whole native sort through plas_sort, sort_splats and PngCompression. Every test asserts
`_plas_fused_ok` on its input first, so none can pass through the torch composition. Inputs and float64 evaluations come from
tests/_plas_cases.py and are made on the CPU."""
import functools

import pytest
import torch

import _plas_cases as pc
from gsplat_amd.compression import PngCompression, plas_sort
from gsplat_amd.compression import sort as S
from gsplat_amd.compression.png_compression import log_transform

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(4, 4), (5, 9), (33, 20), (64, 64), (70, 130)]
CS = [1, 3, 14, 17, 32]
BS = [2, 4, 8, 16, 64]
SEED_T = [(0, 0), (12345, 7), (2 ** 32 - 1, 2 ** 31 + 5)]


def _radii(H, W):
    m = min(H, W)
    return sorted({r for r in (1, 2, m // 2 - 1, m - 1) if 1 <= r <= m - 1})


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_blur_against_the_float64_composition(H, W, C):
    """Per channel within 2 (L + 1) u max|grid|, L = max(H, W) + 2 r (tests/_plas_cases.py: blur_tolerance): a wrong tap or
    reflect index is off by about 1 / (2 r + 1), orders of magnitude more."""
    grid = pc.random_grid(H, W, C) * 3.0 - 1.0
    dev = grid.to(DEV)
    assert S._plas_fused_ok(dev.reshape(H * W, C))
    for r in _radii(H, W):
        got = S._blur_fused(dev, r).cpu()
        assert torch.equal(dev.cpu(), grid)  # the input is left alone
        err = (got.double() - S.plas_blur_torch(grid.double(), r)).abs().amax(dim=(0, 1))
        tol = pc.blur_tolerance(grid, H, W, r)
        print(f"{H}x{W}x{C} r={r}: largest error {float((err / tol).max()):.3f} of the tolerance")
        assert (err <= tol).all(), (r, err, tol)


@functools.lru_cache(maxsize=None)
def _step_case(H, W, C):
    """(feats [N, C], index int64 [N], target [N, C]): a shuffled uniform grid and its blur with r = 2. Cached: read-only."""
    feats = pc.random_grid(H, W, C).reshape(H * W, C)
    index = torch.randperm(H * W, generator=torch.Generator().manual_seed(H + W + C))
    target = S.plas_blur_torch(feats[index].reshape(H, W, C), 2).reshape(H * W, C)
    return feats, index, target


def _run_step(rows, target, index, H, W, b, seed, t):
    """One gsx_plas_step on copies: (rows after, index after as int64, (improvement, total) as a float32 tensor), on the CPU."""
    C = rows.shape[1]
    grid = rows.to(DEV).reshape(H, W, C).contiguous()
    idx = index.to(DEV, torch.int32).reshape(H, W).contiguous()
    assert S._plas_fused_ok(grid.reshape(H * W, C))
    res = S._step_fused(grid, target.to(DEV).reshape(H, W, C).contiguous(), idx, b, seed, t)
    return grid.cpu().reshape(H * W, C), idx.cpu().reshape(-1).long(), res.cpu()


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("H,W", [(70, 130), (64, 64)])
def test_step_against_the_definition(H, W, C, b):
    """With plas_groups as the definition of who may move: cells outside the groups keep their bits, a group's index entries are
    permuted among its cells, rows follow the index bit for bit. The permutation taken is, in float64, within 2 e total_chosen of
    the cheapest of the 24, e = (C + 5) u: a difference is rounded once, its square is within 3 u to first order, C terms are
    summed and three more additions form a total - the argument of tests/_kmeans_cases.py: tolerance. improvement and total are
    within (G + C + 5) u (the float64 sum of the absolute terms added: the identity totals for total, the identity and the
    chosen totals for improvement) of their float64 values, and bit-equal on a second run."""
    feats, index, target = _step_case(H, W, C)
    rows = feats[index]
    for seed, t in SEED_T:
        groups = S.plas_groups(H, W, b, seed, t)
        G = len(groups)
        rows_after, index_after, res = _run_step(rows, target, index, H, W, b, seed, t)
        outside = torch.ones(H * W, dtype=torch.bool)
        outside[groups.reshape(-1)] = False
        assert torch.equal(index_after[outside], index[outside]) and torch.equal(rows_after[outside], rows[outside])
        assert torch.equal(rows_after, feats[index_after])
        chosen = pc.chosen_permutation(index, index_after, groups)
        assert (chosen >= 0).all()
        tot64 = pc.totals_f64(rows, target, groups)
        picked = tot64.gather(1, chosen[:, None])[:, 0]
        tol = 2.0 * (C + 5) * pc.U * picked
        excess = picked - tot64.min(dim=1).values
        share = float((excess / tol.clamp_min(1e-300)).max()) if G else 0.0
        print(f"{H}x{W}x{C} b={b} seed={seed} t={t}: G={G}, {int((chosen > 0).sum())} groups moved, largest excess over the float64 "
              f"minimum {share:.3f} of the tolerance")
        assert (excess <= tol).all()
        improvement, total = res.double().tolist()
        want_total, want_improvement = float(tot64[:, 0].sum()), float((tot64[:, 0] - picked).sum())
        assert abs(total - want_total) <= (G + C + 5) * pc.U * want_total
        assert abs(improvement - want_improvement) <= (G + C + 5) * pc.U * float((tot64[:, 0] + picked).sum())
        assert improvement >= 0.0
        if G:
            assert (chosen > 0).any() and improvement > 0.0
        rows_again, index_again, res_again = _run_step(rows, target, index, H, W, b, seed, t)
        assert torch.equal(res_again, res) and torch.equal(index_again, index_after) and torch.equal(rows_again, rows_after)


@pytest.mark.parametrize("b", [2, 8, 64])
def test_step_ties_go_to_the_identity(b):
    H, W, C = 70, 130, 14
    start = torch.arange(H * W)
    constant = torch.full((H * W, C), 0.37)
    grid = pc.random_grid(H, W, C).reshape(H * W, C)
    seed = 3
    t = next(t for t in range(100000) if all(n - o >= b for n, o in zip((H, W), S.plas_offset(b, seed, t))))  # a step with groups
    # a constant grid against its own blur, and target == grid: every total ties or loses against the identity
    for rows, target in ((constant, S.plas_blur_torch(constant.reshape(H, W, C), 3).reshape(H * W, C)), (grid, grid.clone())):
        rows_after, index_after, res = _run_step(rows, target, start, H, W, b, seed, t)
        assert torch.equal(index_after, start) and torch.equal(rows_after, rows)
        assert float(res[0]) == 0.0
    # groups made of four identical rows keep their index entries whatever the target is; the others still move
    groups = S.plas_groups(H, W, b, seed, t)
    same = groups[::2]
    rows = grid.clone()
    rows[same.reshape(-1)] = rows[same[:, :1]].expand(-1, 4, -1).reshape(-1, C)
    target = S.plas_blur_torch(rows.reshape(H, W, C), 2).reshape(H * W, C)
    _, index_after, res = _run_step(rows, target, start, H, W, b, seed, t)
    assert torch.equal(index_after[same], start[same])
    if len(groups) > 1:
        assert float(res[0]) > 0.0 and not torch.equal(index_after, start)


@functools.lru_cache(maxsize=None)
def _torch_sort_on_cpu(side, seed):
    return S.plas_sort_torch(pc.fixture_features(side), side, side, seed=seed)


def test_whole_sort_on_the_correlated_fixture():
    """The kernels' sort is a permutation, the same on a second run, smoother than the Morton layout, and at most 1.10 x as rough
    as the torch composition's for the same fixture and seed: the two share every integer decision and differ in float
    near-ties and blur rounding; seeds move the result by +-1.5 %, the unsorted grid sits at 5.4 x."""
    side = 64
    feats = pc.fixture_features(side)
    dev = feats.to(DEV)
    assert S._plas_fused_ok(dev)
    before = S.fused_sorts
    order = plas_sort(dev, side, side, seed=0)
    assert S.fused_sorts == before + 1 and S.last_steps > 0
    assert order.dtype == torch.int64 and order.device.type == "cuda"
    assert torch.equal(order.cpu().sort().values, torch.arange(side * side))
    assert torch.equal(plas_sort(dev, side, side, seed=0), order)
    fused = pc.roughness(feats, order.cpu(), side, side)
    composed = pc.roughness(feats, _torch_sort_on_cpu(side, 0), side, side)
    unsorted = pc.roughness(feats, torch.arange(side * side), side, side)
    # the Morton layout of the same splats: the first three feature channels are the normalised log-positions
    morton = pc.roughness(feats, pc.morton_order(feats[:, :3]), side, side)
    print(f"roughness: kernels {fused:.4f} in {S.last_steps} steps, torch composition {composed:.4f}, Morton {morton:.4f}, "
          f"unsorted {unsorted:.4f}")
    assert fused < morton
    assert fused <= 1.10 * composed


def test_sort_splats_on_the_device_takes_the_kernels():
    side = 16
    sp = {k: v.to(DEV) for k, v in pc.fixture_splats(side).items()}
    sp["probe"] = torch.arange(side * side, dtype=torch.float32, device=DEV)
    ref = {k: v.clone() for k, v in sp.items()}
    assert S._plas_fused_ok(S._sort_features(sp))
    before = S.fused_sorts
    out = S.sort_splats(sp, verbose=False)
    assert S.fused_sorts == before + 1
    order = out["probe"].long()
    assert torch.equal(order.cpu().sort().values, torch.arange(side * side))
    assert all(torch.equal(out[k], ref[k][order]) for k in ref)
    S.sort_splats({k: v.clone() for k, v in ref.items()}, verbose=False, method="morton")
    assert S.fused_sorts == before + 1
    out = S.sort_splats({k: v.clone() for k, v in ref.items()}, verbose=False, method="plas")
    assert S.fused_sorts == before + 2 and torch.equal(out["probe"].long(), order)


def test_png_compression_on_the_device_keeps_the_set_of_splats(tmp_path):
    """PngCompression under its defaults sorts with the kernels and decodes to the splats that the Morton layout decodes to, in
    another order: the quantisation of a splat does not depend on its cell."""
    side = 48
    sp = {k: v.to(DEV) for k, v in pc.fixture_splats(side).items()}
    sp["probe"] = torch.arange(side * side, dtype=torch.float32, device=DEV)
    pre = dict(sp, means=log_transform(sp["means"]), quats=torch.nn.functional.normalize(sp["quats"], dim=-1))
    assert S._plas_fused_ok(S._sort_features(pre))
    before = S.fused_sorts
    decoded, size = {}, {}
    for name, codec in (("auto", PngCompression(verbose=False)), ("morton", PngCompression(verbose=False, sort_method="morton"))):
        codec.compress(str(tmp_path / name), sp)
        back = codec.decompress(str(tmp_path / name))
        order = back["probe"].long()
        assert torch.equal(order.sort().values, torch.arange(side * side))
        inverse = torch.argsort(order)
        decoded[name] = {k: v[inverse] for k, v in back.items()}
        size[name] = pc.png_bytes(str(tmp_path / name))
    assert S.fused_sorts == before + 1
    for k in decoded["morton"]:
        assert torch.equal(decoded["auto"][k], decoded["morton"][k]), k
    print(f"PNG bytes: kernels {size['auto']}, Morton {size['morton']}")
    assert size["auto"] < size["morton"]
