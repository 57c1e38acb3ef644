"""GPU: the query rasterizers (csrc/raster_query.hip), their sparse twins, the gsx_raster3d_pair_stats counters and
rasterize_to_indices_in_range (csrc/raster_indices.hip) against a float64 walk of the same lists, at every launch shape (tile
sizes 16, 12, 8, 4), list length (empty tiles to six staging batches) and K (1, below and above a pixel's count, with the LDS
opt-in, the last that fits and the first that is refused). tests/_query_cases.py builds the cases and the walk on the CPU;
tests/test_query_cases.py checks them without a GPU.

Every comparison runs on EVERY decided pixel - a pixel where float64 is outside a margin on each decision it takes (margins and
their reasons: _query_cases.py). The undecided ones are the only pixels skipped, and each test recomputes their share and fails
above the cap (walk 5 %, top-K 10 %). Integer results are exact; alphas within the project's rtol 1e-4 / atol 5e-5 and weights
within rtol 2e-3 / atol 1e-6, no outliers allowed."""
import functools

import numpy as np
import pytest
import torch

import _query_cases as qc
from _util import assert_close_ratio

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = [(n, False) for n in qc.CASE_NAMES] + [(n, True) for n in qc.PACKED_CASES]
TOPK_ROWS = [(n, k, False) for n, k in qc.TOPK_PAIRS] + [(n, k, True) for n, k in qc.TOPK_PAIRS if n in qc.PACKED_CASES]


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd

    return gsplat_amd


def cpu(t):
    return t.detach().cpu()


@functools.lru_cache(maxsize=None)
def _inputs(name, packed):
    """(means2d, conics, opacities, offsets, flatten_ids, W, H, tile size) on the device, and the map from returned ids to
    Gaussian ids (packed rows return the row)."""
    cs = qc.case(name)
    src = qc.packed_case(name) if packed else cs
    tensors = tuple(t.to(DEV) for t in (src.means2d, src.conics, src.opacities, src.offsets, src.flatten_ids))
    return tensors + (cs.W, cs.H, cs.ts), (src.gaussian_ids.numpy() if packed else None)


def _gaussian_ids(ids, to_gaussian):
    ids = cpu(ids).numpy().astype(np.int64)
    return ids if to_gaussian is None else np.where(ids >= 0, to_gaussian[np.maximum(ids, 0)], ids)


def _walk_under_cap(name):
    wk = qc.walk(name)
    share = 1.0 - wk.decided.mean()
    print(f"{name}: undecided (walk) {share:.3%}")
    assert share <= qc.WALK_UNDECIDED_CAP
    return wk


def _assert_rows(ids, weights, want_ids, want_weights, rows, name):
    """[P, K] results against the reference on the pixels `rows`: ids and the (-1, 0) padding exact, weights in the band."""
    assert ids.shape == want_ids.shape, (ids.shape, want_ids.shape)
    bad = (ids[rows] != want_ids[rows]).any(1)
    assert not bad.any(), (f"{name}: ids differ on {int(bad.sum())} of {int(rows.sum())} decided pixels, "
                           f"first {np.flatnonzero(rows)[bad][:5]}")
    assert (weights[rows][want_ids[rows] < 0] == 0).all(), f"{name}: padding weights are not 0"
    assert_close_ratio(weights[rows], want_weights[rows], 2e-3, 1e-6, max_bad_ratio=0.0, name=name)


@pytest.mark.parametrize("name,packed", ROWS)
def test_num_contributing_matches_the_walk(G, name, packed):
    args, _ = _inputs(name, packed)
    cs, wk = qc.case(name), _walk_under_cap(name)
    counts, alphas = G.rasterize_num_contributing_gaussians(*args)
    assert counts.dtype == torch.int32 and counts.shape == (cs.C, cs.H, cs.W) and alphas.shape == counts.shape
    counts, alphas, dec = cpu(counts).reshape(-1).numpy(), cpu(alphas).reshape(-1).numpy(), wk.decided
    bad = counts[dec] != wk.count[dec]
    assert not bad.any(), f"counts differ on {int(bad.sum())} decided pixels, first {np.flatnonzero(dec)[bad][:5]}"
    assert_close_ratio(alphas[dec], wk.alpha[dec], 1e-4, 5e-5, max_bad_ratio=0.0, name="alphas")


@pytest.mark.parametrize("name,packed", ROWS)
def test_contributing_ids_match_the_walk(G, name, packed):
    args, to_gaussian = _inputs(name, packed)
    cs, wk = qc.case(name), _walk_under_cap(name)
    counts, _ = G.rasterize_num_contributing_gaussians(*args)
    ids, weights = G.rasterize_contributing_gaussian_ids(*args, counts)
    kmax = int(counts.max())
    assert ids.shape == (cs.C, cs.H, cs.W, kmax) and weights.shape == ids.shape and ids.dtype == torch.int32
    ids, weights = _gaussian_ids(ids, to_gaussian).reshape(-1, kmax), cpu(weights).reshape(-1, kmax).numpy()
    # the longest list may belong to an undecided pixel on either side: compare at the wider of the two widths
    wide = max(kmax, wk.ids.shape[1])
    pad = lambda a, v: np.pad(a, ((0, 0), (0, wide - a.shape[1])), constant_values=v)
    _assert_rows(pad(ids, -1), pad(weights, 0.0), pad(wk.ids, -1), pad(wk.weights, 0.0), wk.decided, "contributing ids")


@pytest.mark.parametrize("name,K,packed", TOPK_ROWS)
def test_top_contributing_matches_the_rule(G, name, K, packed):
    args, to_gaussian = _inputs(name, packed)
    cs = qc.case(name)
    want_ids, want_weights, decided = qc.topk(name, K)
    share = 1.0 - decided.mean()
    print(f"{name} K={K}: undecided (top-K) {share:.3%}")
    assert share <= qc.TOPK_UNDECIDED_CAP
    ids, weights = G.rasterize_top_contributing_gaussian_ids(*args, K)
    assert ids.shape == (cs.C, cs.H, cs.W, K) and weights.shape == ids.shape and ids.dtype == torch.int32
    ids, weights = _gaussian_ids(ids, to_gaussian).reshape(-1, K), cpu(weights).reshape(-1, K).numpy()
    _assert_rows(ids, weights, want_ids, want_weights, decided, f"top-{K}")


def test_top_contributing_refuses_the_first_k_that_does_not_fit(G):
    """256 threads per tile: K = 48 is the last whose scratch fits the LDS (run on holes16 above), 49 is an argument error - and
    nothing is launched: the outputs keep their fill."""
    from gsplat_amd import _cabi

    name, K = "holes16", qc.TOPK_FIRST_REFUSED
    assert qc.TOPK_LAST_FITTING in qc.TOPK[name] and qc.case(name).ts == 16
    args, _ = _inputs(name, False)
    with pytest.raises(ValueError, match="num_depth_samples"):
        G.rasterize_top_contributing_gaussian_ids(*args, K)
    cs = qc.case(name)
    m2, con, op, off, fl = args[:5]
    ids = torch.full((cs.C, cs.H, cs.W, K), -7, dtype=torch.int32, device=DEV)
    weights = torch.full((cs.C, cs.H, cs.W, K), -7.0, device=DEV)
    with pytest.raises(ValueError, match="num_depth_samples"):
        _cabi.call("gsx_raster3d_top_contributing", _cabi.ptr(m2), _cabi.ptr(con), _cabi.ptr(op), _cabi.ptr(off), _cabi.ptr(fl),
                   cs.C, fl.numel(), cs.N, cs.W, cs.H, cs.ts, cs.tw, cs.th, K, _cabi.ptr(ids), _cabi.ptr(weights))
    torch.cuda.synchronize()
    assert bool((ids == -7).all()) and bool((weights == -7.0).all())


@pytest.mark.parametrize("kind", ["many", "one"])
@pytest.mark.parametrize("name", qc.SPARSE_CASES)
def test_sparse_twins_equal_dense_at_the_pixels(G, name, kind):
    (m2, con, op, off, fl, W, H, ts), _ = _inputs(name, False)
    cs, sp = qc.case(name), qc.sparse_set(name, kind)
    P = sp.pixels.shape[0]
    layout = (torch.from_numpy(sp.active_tiles).to(DEV), sp.offsets.to(DEV), sp.flatten_ids.to(DEV),
              torch.from_numpy(sp.pixel_mask.view(np.int64)).to(DEV), torch.from_numpy(sp.pixel_cumsum).to(DEV),
              torch.from_numpy(sp.pixel_map).to(DEV))
    sel = tuple(torch.from_numpy(a).to(DEV) for a in (sp.image_ids, sp.pixels[:, 0], sp.pixels[:, 1]))
    geom = (W, H, ts, cs.tw, cs.th)

    cnt_s, al_s = G.rasterize_num_contributing_gaussians_sparse(m2, con, op, *layout, *geom)
    cnt_d, al_d = G.rasterize_num_contributing_gaussians(m2, con, op, off, fl, W, H, ts)
    assert cnt_s.shape == (P,) and cnt_s.dtype == torch.int32
    assert torch.equal(cnt_s, cnt_d[sel]) and torch.equal(al_s, al_d[sel])
    if kind == "many":
        assert int(cnt_s.max()) > 3

    ids_s, w_s = G.rasterize_contributing_gaussian_ids_sparse(m2, con, op, *layout, cnt_s, *geom)
    ids_d, w_d = G.rasterize_contributing_gaussian_ids(m2, con, op, off, fl, W, H, ts, cnt_d)
    K = int(cnt_s.max())
    assert ids_s.shape == (P, K)
    assert torch.equal(ids_s, ids_d[sel][:, :K]) and torch.equal(w_s, w_d[sel][:, :K])
    assert bool((ids_d[sel][:, K:] == -1).all())

    for K in (4, qc.TOPK[name][-1]):
        tid_s, tw_s = G.rasterize_top_contributing_gaussian_ids_sparse(m2, con, op, *layout, *geom, K)
        tid_d, tw_d = G.rasterize_top_contributing_gaussian_ids(m2, con, op, off, fl, W, H, ts, K)
        assert tid_s.shape == (P, K)
        assert torch.equal(tid_s, tid_d[sel]) and torch.equal(tw_s, tw_d[sel])


def _assert_indices(G, name, part):
    """One window of rasterize_to_indices_in_range against the walk of the same window from the same fp32 T0."""
    (m2, con, op, off, fl, W, H, ts), _ = _inputs(name, False)
    cs, wk = qc.case(name), qc.walk(name, part)
    share = 1.0 - wk.decided.mean()
    print(f"{name} window {part}: undecided {share:.3%}")
    assert share <= qc.WALK_UNDECIDED_CAP
    rs, re = qc.FULL_RANGE if part == "full" else qc.RANGES[part]
    T0 = torch.from_numpy(wk.T0).reshape(cs.C, H, W).to(DEV)
    g, p, i = (cpu(t).numpy() for t in G.rasterize_to_indices_in_range(rs, re, T0, m2, con, op, W, H, ts, off, fl))
    assert g.dtype == np.int64 and g.shape == p.shape == i.shape
    assert ((p >= 0) & (p < W * H) & (i >= 0) & (i < cs.C)).all()
    key = i * (W * H) + p
    assert (key[1:] >= key[:-1]).all(), "pairs are not in (image, pixel)-major order"
    keep = wk.decided[key]
    want_p, want_k = np.nonzero(wk.ids >= 0)
    sel = wk.decided[want_p]
    assert np.array_equal(key[keep], want_p[sel]), "decided pixels: pair counts differ"
    assert np.array_equal(g[keep], wk.ids[want_p[sel], want_k[sel]]), "decided pixels: id sequences differ"
    return g.size


@pytest.mark.parametrize("name", qc.CASE_NAMES)
def test_indices_full_range_matches_the_walk(G, name):
    assert _assert_indices(G, name, "full") > 0


@pytest.mark.parametrize("name", qc.RANGE_CASES)
def test_indices_windows_chained_through_the_transmittance(G, name):
    sizes = [_assert_indices(G, name, k) for k in range(len(qc.RANGES))]
    assert all(s > 0 for s in sizes[:-1]) and sizes[-1] == 0  # the last window lies beyond every list


@pytest.mark.parametrize("name", qc.STATS_CASES)
def test_pair_stats_counters(G, name):
    from gsplat_amd import _cabi

    (m2, con, op, off, fl, W, H, ts), _ = _inputs(name, False)
    cs, wk = qc.case(name), _walk_under_cap(name)
    counts, _ = G.rasterize_num_contributing_gaussians(m2, con, op, off, fl, W, H, ts)
    stats = torch.zeros(8, dtype=torch.int64, device=DEV)

    def run():
        _cabi.call("gsx_raster3d_pair_stats", _cabi.ptr(m2), _cabi.ptr(con), _cabi.ptr(op), _cabi.ptr(off), _cabi.ptr(fl), cs.C,
                   fl.numel(), W, H, ts, cs.tw, cs.th, _cabi.ptr(stats))
        return [int(v) for v in stats.tolist()]

    s = run()
    print(f"{name}: stats {s}")
    dec = wk.decided
    assert s[3] == int(counts.sum())
    assert wk.count[dec].sum() <= s[3] <= wk.count[dec].sum() + wk.list_len[~dec].sum()  # and that sum is the walk's
    assert wk.walked[dec].sum() <= s[0] <= wk.walked[dec].sum() + wk.list_len[~dec].sum()
    assert s[1] % 64 == 0 and s[3] <= s[2] <= min(s[0], s[1]) and s[4] <= s[1]
    assert s[5:] == [0, 0, 0]
    assert run() == [2 * v for v in s]  # the entry adds
