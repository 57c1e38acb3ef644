"""GPU: the binned intersection's per-tile sort on lists just over a power of two (csrc/isect_binned.hip, bn_list_words /
bn_sort_list): a list of H < n <= H + H / 4 entries, H >= 256, is sorted as two runs - the first H dealt entries and the
tail - in H + round_up(n - H, 8) words of the bin's 4352-word arena and merged on the way out.

A 128 x 32 image is two bins of 4 x 2 tiles. Every row is a small Gaussian at the centre of one tile (radius 1, radius-box
mode), so each list length is exact. The layouts put every length on both sides of each rule (255 .. 257, 320 / 321, 511 ..
513, 520, 576 / 577, 640 / 641, 1023 .. 1025) into bins of these kinds: several split lists together, regions that sum to
exactly the arena, the arena + 8 (the last tile takes a second batch), an empty tile; one layout holds heads of 2048 and
4096. `list_words` restates the region rule; the layouts' sums are asserted from it, so a change of the rule or of the
arena's size fails here rather than silently testing other bins.

Which entries form the head is the order of the deal, i.e. row order up to the order of the LDS atomics of one trip of the
workgroup; the "odd" patterns put their zero, negative and denormal depth on the three first rows of every list (head) or the
three last (tail). Any of them sends the list to the integer network; the other lists of the call stay on the f64 network.

isect_ids, flatten_ids, isect_offsets and tiles_per_gauss must equal the CPU oracle bit for bit."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TW, TH, TS = 8, 2, 16  # 128 x 32 pixels
ARENA = 4352


def list_words(n):
    """Arena words of a list of n entries (bn_list_words)."""
    if n <= 0:
        return 0
    P = 64
    while P < n:
        P <<= 1
    H = P >> 1
    if H >= 256 and n - H <= H // 4:
        return H + ((n - H + 7) & ~7)
    return P


# name: (lengths of bin 0's eight tiles, lengths of bin 1's eight tiles, arena words of bin 0, of bin 1); a bin's tiles in the
# order of the greedy cut: x fastest, then y
LAYOUTS = {
    # seven split lists and an empty tile | every length that keeps its power of two, the regions sum to the arena exactly
    "split-and-padded": ((257, 320, 513, 520, 0, 576, 577, 640), (255, 256, 321, 511, 512, 641, 1023, 256), 3424, ARENA),
    # arena + 8: the eighth tile sorts in a second batch | eight split lists of 544 words each: the arena exactly
    "overflow-and-exact": ((1024, 1025, 640, 640, 512, 256, 128, 100), (544, 543, 542, 541, 540, 539, 538, 537), ARENA + 8, ARENA),
    # heads of 2048 (tails of 52 and of 512 entries: two batches) | a head of 4096, and 1281 entries: the power of two again
    "long-heads": ((2100, 0, 0, 2560, 0, 0, 0, 0), (0, 4100, 0, 0, 0, 0, 1281, 0), 2104 + 2560, 4104 + 2048),
}
WANTED = (255, 256, 257, 320, 321, 511, 512, 513, 520, 576, 577, 640, 641, 1023, 1024, 1025)
PATTERNS = ("equal", "odd-in-head", "odd-in-tail")
ODD = np.array([0.0, -1.5, 1e-40], dtype=np.float32)  # zero, negative, denormal: none orders like a positive normal double


def test_layouts_cover_the_issue():
    seen = {n for b0, b1, _, _ in LAYOUTS.values() for n in b0 + b1}
    assert set(WANTED) <= seen
    for name, (b0, b1, w0, w1) in LAYOUTS.items():
        assert (sum(map(list_words, b0)), sum(map(list_words, b1))) == (w0, w1), name
    assert [list_words(n) for n in (257, 320, 321, 513, 640, 641, 1025, 1280, 1281)] == [264, 320, 512, 520, 640, 1024, 1032, 1280, 2048]
    assert any(0 in b0 + b1 for b0, b1, _, _ in LAYOUTS.values())


@functools.lru_cache(maxsize=None)
def case(layout, pattern):
    """CPU inputs (means2d [1, N, 2], radii [1, N, 2], depths [1, N]) and the oracle's outputs. Shared: do not modify."""
    from oracle import oracle as O

    b0, b1, _, _ = LAYOUTS[layout]
    lengths = np.zeros(TW * TH, dtype=np.int64)
    for b, lens in enumerate((b0, b1)):
        for i, n in enumerate(lens):
            lengths[(i // 4) * TW + 4 * b + i % 4] = n
    rng = np.random.default_rng(11 + 5 * sorted(LAYOUTS).index(layout) + PATTERNS.index(pattern))
    tile = rng.permutation(np.repeat(np.arange(TW * TH), lengths))
    N = tile.size
    if pattern == "equal":
        depths = np.full(N, 2.5, dtype=np.float32)
    else:
        depths = (rng.random(N, dtype=np.float32) * np.float32(10.0) + np.float32(0.1)).astype(np.float32)
        for t in np.flatnonzero(lengths >= 3):
            rows = np.flatnonzero(tile == t)
            depths[rows[:3] if pattern == "odd-in-head" else rows[-3:]] = ODD
    means = np.stack([(tile % TW) * TS + TS / 2, (tile // TW) * TS + TS / 2], axis=-1).astype(np.float32)
    m2, rad = torch.from_numpy(means).reshape(1, N, 2), torch.ones(1, N, 2, dtype=torch.int32)
    d = torch.from_numpy(depths).reshape(1, N)
    tpg, ids, fl = O.isect_tiles(m2, rad, d, TS, TW, TH)
    off = O.isect_offset_encode(ids, 1, TW, TH)
    got_len = np.diff(np.concatenate([off.numpy().reshape(-1), [ids.numel()]]))
    assert np.array_equal(got_len, lengths), "the oracle's list lengths are the layout's"
    return dict(means2d=m2, radii=rad, depths=d, tpg=tpg, ids=ids, fl=fl, off=off)


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd

    return gsplat_amd


@pytest.mark.parametrize("network", ["f64", "int"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_split_lists_match_the_oracle(G, monkeypatch, layout, pattern, network):
    from gsplat_amd import _cabi

    c = case(layout, pattern)
    monkeypatch.setenv("GSX_ISECT_PATH", "binned")
    monkeypatch.delenv("GSX_ISECT_SORT", raising=False)
    if network == "int":
        monkeypatch.setenv("GSX_ISECT_SORT", "int")
    m2, rad, d = c["means2d"].to(DEV), c["radii"].to(DEV), c["depths"].to(DEV)
    _cabi.profile_begin()
    try:
        tpg, ids, fl = G.isect_tiles(m2, rad, d, TS, TW, TH)
        torch.cuda.synchronize()
    finally:
        ran = set(_cabi.profile_end())
    assert {"gsx_isect_binned_count", "gsx_isect_binned_emit_sort"} <= ran, sorted(ran)
    assert "gsx_isect_fused_emit_sort" not in ran, "the binned path sent the call back"
    off = G.isect_offset_encode(ids, 1, TW, TH)
    ids, fl = ids.cpu(), fl.cpu()
    if not (torch.equal(ids, c["ids"]) and torch.equal(fl, c["fl"])):
        assert ids.shape == c["ids"].shape
        bad = int(torch.nonzero((ids != c["ids"]) | (fl != c["fl"]))[0])
        t = int(c["ids"][bad]) >> 32
        start = int(c["off"].reshape(-1)[t])
        raise AssertionError(f"first difference at entry {bad}: tile {t}, position {bad - start} of its list; got key "
                             f"{int(ids[bad]):#x} id {int(fl[bad])}, expected key {int(c['ids'][bad]):#x} id {int(c['fl'][bad])}")
    assert torch.equal(off.cpu(), c["off"]), "isect_offsets"
    assert torch.equal(tpg.cpu(), c["tpg"]), "tiles_per_gauss"
