"""CPU tests of tests/_sort_cases.py: the case builders of tests/test_gpu_sort_edges.py build what they claim - exact list
lengths, keys that fit their bits, ascending ids, a stable reference order, short tie runs in long lists, depth bits on both sides
of both thresholds of the network choice. Runs without a GPU."""
import numpy as np
import pytest
import torch

import _sort_cases as sc


def _u64(t):
    return t.numpy().view(np.uint64)


def _check_sorted_stable(keys, vals, exp_keys, exp_vals, key_mask=None):
    """(exp_keys, exp_vals) is a permutation of the input, ascending in the unsigned (masked) key, equal keys in ascending id."""
    k = _u64(exp_keys) if key_mask is None else _u64(exp_keys) & key_mask
    assert (k[1:] >= k[:-1]).all(), "reference keys do not ascend as unsigned"
    tied = k[1:] == k[:-1]
    v = exp_vals.numpy().astype(np.int64)
    assert (v[1:][tied] > v[:-1][tied]).all(), "reference is not stable"
    back = np.argsort(v, kind="stable")  # ids are distinct and ascending in the input: this undoes the sort
    assert np.array_equal(v[back], vals.numpy().astype(np.int64)) and np.array_equal(_u64(exp_keys)[back], _u64(keys))


def _check_lists(keys, vals, lengths, n_tiles, n_images):
    tb = sc.bits_for(n_tiles)
    hi = _u64(keys) >> np.uint64(32)
    assert int(hi.max(initial=0)) < (1 << (tb + sc.bits_for(n_images))), "keys exceed 32 + tile + image bits"
    tile, img = hi & np.uint64((1 << tb) - 1), hi >> np.uint64(tb)
    assert int(tile.max(initial=0)) < n_tiles and int(img.max(initial=0)) < n_images
    lin = (img * np.uint64(n_tiles) + tile).astype(np.int64)
    assert np.array_equal(np.bincount(lin, minlength=n_tiles * n_images), np.asarray(lengths))
    v = vals.numpy().astype(np.int64)
    assert (v[1:] > v[:-1]).all() and v.min(initial=0) >= 0, "ids must ascend in emission order"
    return lin


def _check_run_bound(keys, lin):
    """No depth value more than RUN_BOUND times in a list longer than RUN_BOUND_ABOVE."""
    depth = _u64(keys) & np.uint64(sc.MASK32)
    for b in np.flatnonzero(np.bincount(lin) > sc.RUN_BOUND_ABOVE):
        counts = np.unique(depth[lin == b], return_counts=True)[1]
        assert counts.max() <= sc.RUN_BOUND, (int(b), int(counts.max()))


def _check_both_sides_of_both_thresholds(depth_bits):
    have = set(np.unique(depth_bits).tolist())
    for b in (sc.ODD_LO - 1, sc.ODD_LO, sc.ODD_LO + 1, sc.ODD_HI - 1, sc.ODD_HI, 0x7FFFFFFF, 0x7F800000, 0x7FC00000):
        assert b in have, hex(b)
    odd = sc.key_is_odd(np.array([sc.ODD_LO - 1, sc.ODD_LO, sc.ODD_HI - 1, sc.ODD_HI], dtype=np.uint32))
    assert odd.tolist() == [True, False, False, True]


def test_key_is_odd_restates_the_documented_range():
    odd = {b: bool(sc.key_is_odd(np.uint32(b))) for b in sc.EDGE_BITS}
    f64_ok = {0x00100000, 0x00100001, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000, 0x7FEFFFFF}
    assert {b for b, o in odd.items() if not o} == f64_ok  # float +inf and the quiet NaN 0x7FC00000 ride the f64 network


@pytest.mark.parametrize("family,spread_ids", [(f, False) for f in sc.DEPTH_FAMILIES] + [("normal", True)])
def test_tile_sort_cases(family, spread_ids):
    I, tw, th = sc.TILE_SORT_GRID
    keys, vals, (ek, ev) = sc.tile_sort_case(family, spread_ids=spread_ids)
    assert sorted(set(sc.TILE_SORT_LENGTHS)) == sorted(sc.TILE_SORT_WANTED)
    assert sc.TILE_SORT_LENGTHS[0] == 0 and sc.TILE_SORT_LENGTHS[-1] == 0
    assert (tw * th) & (tw * th - 1), "the grid is meant to leave a hole in the key space"
    lin = _check_lists(keys, vals, sc.TILE_SORT_LENGTHS, tw * th, I)
    _check_sorted_stable(keys, vals, ek, ev)
    _check_run_bound(keys, lin)
    depth = (_u64(keys) & np.uint64(sc.MASK32)).astype(np.uint32)
    if spread_ids:
        assert int(vals[-1]) == sc.INT32_MAX and int(vals[len(vals) // 2]) > 2**29
    if family in ("normal", "ties"):
        assert not sc.key_is_odd(depth).any()
    if family == "ties":  # exact ties are common in every list long enough to have some, the global-memory list included
        for b in np.flatnonzero(np.asarray(sc.TILE_SORT_LENGTHS) >= 127):
            d = depth[lin == b]
            assert np.unique(d).size < 0.9 * d.size, int(b)
    if family == "edge-bits":
        _check_both_sides_of_both_thresholds(depth)
        assert set(np.unique(depth[lin == 20]).tolist()) >= set(sc.EDGE_BITS)  # also in the 20 000-entry list
    if family == "one-odd":  # exactly one odd key per list: the last entry
        for b in np.flatnonzero(sc.TILE_SORT_LENGTHS):
            odd = sc.key_is_odd(depth[lin == b])
            assert odd.sum() == 1 and odd[-1] and depth[lin == b][-1] == sc.ODD_HI


def test_tile_sort_further_cases():
    keys, vals, (ek, ev) = sc.tile_sort_case("ties", lengths=(200, 0, 3000), grid=(3, 1, 1))
    lin = _check_lists(keys, vals, (200, 0, 3000), 1, 3)
    assert int((_u64(keys) >> np.uint64(32)).max()) == 2  # tile_bits == 0: the image id sits right above the depth
    _check_sorted_stable(keys, vals, ek, ev)
    _check_run_bound(keys, lin)
    keys, vals, (ek, ev) = sc.tile_sort_max_bins_case()
    n = keys.numel()
    lin = _check_lists(keys, vals, np.bincount((_u64(keys) >> np.uint64(32)).astype(np.int64), minlength=sc.MAX_BINS),
                       sc.MAX_BINS, 1)
    assert sc.MAX_BINS * -(-n // 32768) > 1_048_576, "the [bin][chunk] table must be long enough for the scan's carry"
    assert np.bincount(lin).max() <= sc.RUN_BOUND_ABOVE
    _check_sorted_stable(keys, vals, ek, ev)


@pytest.mark.parametrize("family", sc.ISECT_FAMILIES)
@pytest.mark.parametrize("layout", sorted(sc.ISECT_LAYOUTS))
def test_isect_cases(layout, family):
    tw, th, ts = sc.ISECT_GRID
    c = sc.isect_case(layout, family)
    N = c["tile"].size
    want = np.zeros(tw * th, dtype=np.int64)
    for (tx, ty), n in sc.ISECT_LAYOUTS[layout]:
        want[ty * tw + tx] = n
    ids = torch.arange(N, dtype=torch.int32)
    lin = _check_lists(c["keys"], ids, want, tw * th, 1)
    assert np.array_equal(lin, c["tile"])
    # every row lands in exactly its tile: the box [mean - 1, mean + 1] lies strictly inside it
    m, r = c["means2d"][0].numpy().astype(np.float64), c["radii"][0].numpy()
    lo, hi = np.floor((m - r) / ts), np.ceil((m + r) / ts)
    assert ((hi - lo) == 1).all() and np.array_equal((lo[:, 1] * tw + lo[:, 0]).astype(np.int64), c["tile"])
    assert np.array_equal(c["depths"][0].numpy().view(np.uint32), c["depth_bits"]), "depth bits must survive the float tensor"
    _check_sorted_stable(c["keys"], ids, c["isect_ids"], c["flatten_ids"])
    _check_run_bound(c["keys"], lin)
    assert np.array_equal(c["offsets"].reshape(-1).numpy(), np.cumsum(want) - want)
    assert torch.equal(c["offsets"], sc.offsets_reference(c["isect_ids"], 1, tw, th))
    if family == "edge-bits":
        _check_both_sides_of_both_thresholds(c["depth_bits"])


def test_isect_layouts_sit_in_the_bins_they_name():
    def bins(layout):
        return [(tx // 4, ty // 2) for (tx, ty), _ in sc.ISECT_LAYOUTS[layout]]

    assert len(set(bins("singles"))) == 8
    assert [n for _, n in sc.ISECT_LAYOUTS["singles"]] == [64, 65, 512, 513, 4096, 4097, 9152, 9153]
    for layout in ("two-2049", "eight-513", "4097-and-seven-100"):
        assert len(set(bins(layout))) == 1, layout
    assert sorted(n for _, n in sc.ISECT_LAYOUTS["4097-and-seven-100"]) == [100] * 7 + [4097]
    assert sc.ISECT_LAYOUTS["last-tile"][0][0] == (sc.ISECT_GRID[0] - 1, sc.ISECT_GRID[1] - 1)


@pytest.mark.parametrize("end_bit", sc.RADIX_END_BITS)
def test_radix_cases(end_bit):
    mask = sc.radix_mask(end_bit)
    for n in (1, 65, 4097):
        vals = torch.arange(n, dtype=torch.int32)
        fams = sc.RADIX_FAMILIES + (("above-end-bit",) if end_bit in sc.RADIX_ABOVE_END_BITS else ())
        for family in fams:
            keys = sc.radix_keys(n, end_bit, family)
            assert keys.dtype == torch.int64 and keys.numel() == n
            k = _u64(keys)
            if family == "above-end-bit":
                assert ((k >> np.uint64(end_bit)) != 0).all(), "every key carries a bit at or above end_bit"
            elif end_bit:
                assert (k <= mask).all(), (family, "keys must fit end_bit bits")
            if family == "ones" and end_bit:
                assert (k == mask).all()
            if family == "top-digit" and end_bit and n > 64:
                shift = np.uint64(8 * ((end_bit + 7) // 8 - 1))
                assert np.unique(k & ((np.uint64(1) << shift) - np.uint64(1))).size == 1 and np.unique(k).size > 1
            if family == "bit0" and end_bit and n > 64:
                assert np.unique(k >> np.uint64(1)).size == 1 and np.unique(k).size == 2
            ek, ev = sc.radix_reference(keys, end_bit)
            _check_sorted_stable(keys, vals, ek, ev, key_mask=mask)
    if end_bit == 64:
        assert int(mask) == 2**64 - 1
        keys = sc.radix_keys(4097, 64, "random")
        assert (keys < 0).any() and (keys >= 0).any()
        ek, _ = sc.radix_reference(keys, 64)
        assert bool((ek[: int((keys >= 0).sum())] >= 0).all()), "bit 63 set sorts last: the order is unsigned"


def test_scan_cases():
    assert sc.SCAN_SIZES[-2:] == (1_048_577, 2_097_153)
    assert [-(-n // sc.SCAN_CHUNK) for n in sc.SCAN_SIZES[-2:]] == [257, 513]  # the carry runs once and twice
    for n in (1, 4097):
        for family in sc.SCAN_FAMILIES + ("int32-max",):
            x = sc.scan_values(n, family)
            assert x.dtype == torch.int32 and x.numel() == n
        assert int(sc.scan_values(n, "one-first")[0]) == 1 and int(sc.scan_values(n, "one-last")[-1]) == 1
        assert int(sc.scan_values(n, "one-last").sum()) == 1
    assert int(sc.scan_values(4097, "rand-signed").min()) < 0 <= int(sc.scan_values(4097, "rand-nonneg").min())
    assert int(sc.scan_reference(sc.scan_values(8192, "int32-max"))[-1]) == 8192 * sc.INT32_MAX > 2**31


@pytest.mark.parametrize("name", sorted(sc.OFFSET_CASES))
def test_offset_cases(name):
    I, tw, th, occupied = sc.OFFSET_CASES[name]
    keys, off = sc.offset_case(name)
    k = _u64(keys)
    assert (k[1:] >= k[:-1]).all() and off.shape == (I, th, tw)
    counts = np.zeros(I * tw * th, dtype=np.int64)
    for b, c in occupied:
        counts[b] = c
    assert np.array_equal(off.reshape(-1).numpy(), np.cumsum(counts) - counts)
    _check_lists(keys, torch.arange(keys.numel(), dtype=torch.int32), counts, tw * th, I)
