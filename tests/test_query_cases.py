"""CPU tests of tests/_query_cases.py: the cases of tests/test_gpu_query.py reach the regimes they are there for (padding
workgroups, several staging batches, saturation, counts below K, empty tiles, sigma < 0), the undecided shares stay under their
caps, and on decided pixels the fp32 C oracle - itself pinned to the reference - agrees exactly with the float64 walk on counts,
ids and top-K ids. Runs without a GPU."""
import numpy as np
import pytest
import torch

import _query_cases as qc
from oracle import oracle as O

Q_BATCH = 256  # csrc/raster_query.hip: kQBatch, list entries staged per round


def _lengths(cs):
    start, end = qc.list_bounds(cs)
    return end - start


def _saturating(wk):
    return wk.walked < wk.list_len  # stopped in front of the end of its list (a stop AT the last entry reads as open: rare)


# what each case is there for: name -> checks on (lengths per tile, full walk)
def test_case_regimes():
    L = {n: _lengths(qc.case(n)) for n in qc.CASE_NAMES}
    wk = {n: qc.walk(n) for n in qc.CASE_NAMES}
    for n in qc.CASE_NAMES:  # padding workgroups of grid = ceil8(tiles) run everywhere
        assert L[n].size % 8 != 0, n
    # deep16: every list takes several staging batches, every pixel saturates, sigma < 0 pairs are walked
    assert L["deep16"].size == 9 and L["deep16"].min() > 2 * Q_BATCH and L["deep16"].max() > 5 * Q_BATCH
    assert _saturating(wk["deep16"]).all() and wk["deep16"].count.min() >= 24 and wk["deep16"].sigma_neg.sum() > 1000
    # thin16: three images, part of the pixels saturate and part walk their whole list
    assert L["thin16"].size == 27 and 0.2 < _saturating(wk["thin16"]).mean() < 0.5 and wk["thin16"].count.max() > 200
    # t12: 144 of 256 threads live; t8 / t4: the 64-thread launch, 16 live lanes at 4; lists of more than one batch
    assert L["t12"].size == 12 and L["t12"].max() > 3 * Q_BATCH and _saturating(wk["t12"]).all()
    assert L["t8"].size == 30 and L["t8"].max() > 2 * Q_BATCH and _saturating(wk["t8"]).all()
    assert wk["t8"].sigma_neg.sum() > 500
    cs = qc.case("t4")
    assert L["t4"].size == 99 and cs.W % 4 != 0 and cs.H % 4 != 0  # ragged right and bottom tiles
    for n, empty in (("holes16", 12), ("holes8", 30)):  # empty tiles, pixels without a contributor, counts below every K >= 4
        assert int((L[n] == 0).sum()) == empty
        assert (wk[n].count == 0).mean() > 0.3 and (wk[n].count < 4).mean() > 0.5 and wk[n].count.max() < 24
        assert ((wk[n].count > 0) & (wk[n].count < 4)).any() and (wk[n].count > 4).any()
    for n in ("t12", "thin16"):  # ragged right tiles at 12 and 16 too
        assert qc.case(n).W % qc.case(n).ts != 0


@pytest.mark.parametrize("name", qc.CASE_NAMES)
def test_walk_is_consistent_and_under_its_cap(name):
    wk = qc.walk(name)
    share = 1.0 - wk.decided.mean()
    print(f"{name}: undecided (walk) {share:.3%}")
    assert share <= qc.WALK_UNDECIDED_CAP
    k = np.arange(wk.ids.shape[1])[None, :]
    assert ((wk.ids >= 0) == (k < wk.count[:, None])).all() and ((wk.weights > 0) == (k < wk.count[:, None])).all()
    assert wk.ids.max() < qc.case(name).N and (wk.walked <= wk.list_len).all()
    # the weights of a pixel sum to 1 - T
    np.testing.assert_allclose(wk.weights.sum(1), wk.alpha, rtol=0, atol=1e-12)
    assert (wk.T_end[_saturating(wk)] > qc.T_THRESHOLD).all()  # the stop is exclusive


@pytest.mark.parametrize("name,K", qc.TOPK_PAIRS)
def test_topk_is_consistent_and_under_its_cap(name, K):
    wk = qc.walk(name)
    ids, w, decided = qc.topk(name, K)
    share = 1.0 - decided.mean()
    print(f"{name} K={K}: undecided (top-K) {share:.3%}")
    assert share <= qc.TOPK_UNDECIDED_CAP
    kept = np.minimum(wk.count, K)
    k = np.arange(K)[None, :]
    assert ((ids >= 0) == (k < kept[:, None])).all() and ((w > 0) == (k < kept[:, None])).all()  # padding (-1, 0) last
    few = wk.count <= K  # nothing was ever replaced: the list itself
    pad = max(0, K - wk.ids.shape[1])
    assert np.array_equal(ids[few], np.pad(wk.ids, ((0, 0), (0, pad)), constant_values=-1)[few, :K])
    # the kept weights are the K largest of the pixel where no two weights tie
    top = -np.sort(-wk.weights, axis=1)[:, :K]
    np.testing.assert_array_equal(-np.sort(-w, axis=1)[decided][:, :top.shape[1]], top[decided])


def test_thin16_at_24_samples_is_over_the_cap():
    """Why K = 24 is not run on thin16: long walks of weak samples, many near-ties among the kept ones."""
    assert 24 not in qc.TOPK["thin16"] and 1.0 - qc.topk("thin16", 24)[2].mean() > qc.TOPK_UNDECIDED_CAP


@pytest.mark.parametrize("name", qc.PACKED_CASES)
def test_packed_rows_give_the_dense_lists(name):
    cs, pk = qc.case(name), qc.packed_case(name)
    assert torch.equal(pk.offsets, cs.offsets)
    assert torch.equal(pk.rows[pk.flatten_ids.long()], cs.flatten_ids.long())
    assert pk.rows.numel() < cs.C * cs.N  # some rows were culled: packed ids differ from Gaussian ids


@pytest.mark.parametrize("name", qc.CASE_NAMES)
def test_c_oracle_agrees_with_the_walk_where_decided(name):
    cs, wk = qc.case(name), qc.walk(name)
    lids, lwts, alphas = O.raster_contributions(cs.means2d, cs.conics, cs.opacities, cs.W, cs.H, cs.ts, cs.offsets,
                                                cs.flatten_ids)
    counts = np.array([len(x) for x in lids])
    dec = wk.decided
    assert np.array_equal(counts[dec], wk.count[dec])
    kmax = wk.ids.shape[1]
    padded = np.array([x[:kmax] + [-1] * (kmax - len(x[:kmax])) for x in lids], dtype=np.int64).reshape(-1, kmax)
    assert np.array_equal(padded[dec], wk.ids[dec])
    np.testing.assert_allclose(alphas.reshape(-1).numpy()[dec], wk.alpha[dec], rtol=1e-4, atol=5e-5)
    # the indices op of the oracle: tile-major; grouped by (image, pixel) it is the walk's sequence
    g, p, i = O.rasterize_to_indices(cs.means2d, cs.conics, cs.opacities, cs.W, cs.H, cs.ts, cs.offsets, cs.flatten_ids)
    key = (i * (cs.W * cs.H) + p).numpy()
    order = np.argsort(key, kind="stable")
    key, g = key[order], g.numpy()[order]
    keep = dec[key]
    want_p, want_k = np.nonzero(wk.ids[:, :] >= 0)
    sel = dec[want_p]
    assert np.array_equal(key[keep], want_p[sel]) and np.array_equal(g[keep], wk.ids[want_p[sel], want_k[sel]])
    for K in qc.TOPK[name]:
        oi, _ = O.top_contributions(lids, lwts, K)
        ti, _, tdec = qc.topk(name, K)
        assert np.array_equal(oi[tdec], ti[tdec]), K


@pytest.mark.parametrize("name", qc.RANGE_CASES)
def test_range_windows_chain_through_the_transmittance(name):
    cs, full = qc.case(name), qc.walk(name)
    parts = [qc.walk(name, k) for k in range(len(qc.RANGES))]
    assert parts[-1].count.sum() == 0 and parts[-1].list_len.max() == 0  # beyond every list
    assert all(p.count.sum() > 0 for p in parts[:-1]) and all(1.0 - p.decided.mean() <= qc.WALK_UNDECIDED_CAP for p in parts)
    assert np.array_equal(parts[1].T0, parts[0].T_end.astype(np.float32)) and (parts[1].T0 < 1).any()
    # a pixel that never stops inside a window walks, window by window, what the full walk walks; one that stops starts the
    # next window afresh (the stop is per call), so "split equals full" does not hold for it
    open_ = np.ones(full.count.shape, bool)
    for p in parts:
        open_ &= p.walked == p.list_len
    open_ &= full.walked == full.list_len
    assert open_.any() or name != "thin16"
    total = sum(p.count for p in parts)
    assert np.array_equal(total[open_], full.count[open_])
    stopped_early = np.zeros(full.count.shape, bool)
    for p in parts[:-2]:
        stopped_early |= p.walked < p.list_len
    assert (total[stopped_early] > full.count[stopped_early]).any()


@pytest.mark.parametrize("name", qc.SPARSE_CASES)
def test_sparse_sets_are_what_they_claim(name):
    cs = qc.case(name)
    many, one = qc.sparse_set(name, "many"), qc.sparse_set(name, "one")
    assert one.pixels.shape == (1, 2) and one.active_tiles.size == 1
    assert many.active_tiles.size % 8 != 0 and many.active_tiles.size > 4
    assert np.unique(np.concatenate([many.image_ids[:, None], many.pixels], 1), axis=0).shape[0] == many.pixels.shape[0]
    assert (many.pixels[:, 0] < cs.H).all() and (many.pixels[:, 1] < cs.W).all()
    L = _lengths(cs)
    if (L == 0).any():  # pixels of tiles without a single Gaussian
        assert (L[many.active_tiles] == 0).any()
    lens = np.diff(many.offsets.numpy())
    assert np.array_equal(lens, L[many.active_tiles])
    assert not np.array_equal(many.pixel_map, np.arange(many.pixel_map.size))  # the caller's order is not the layout's
