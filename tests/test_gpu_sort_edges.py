"""GPU: the device-wide prefix sum, the LSD radix sort and the per-tile sorts at every size and bit pattern where they change
algorithm (tests/_sort_cases.py builds the cases and the CPU references; tests/test_sort_cases.py checks the builders).

The three primitives are bit-exact by contract, so every comparison is torch.equal against plain torch / numpy on the CPU:
scan = cumsum on int64, sorts = a stable sort of the keys read as unsigned 64-bit, offsets = searchsorted. Every direct C-ABI
call gets guard bands: outputs with 64 extra elements, the workspace with 4096 extra bytes, both filled with a sentinel that
must still be there afterwards; inputs the header calls unmodified are compared too."""
import pytest
import torch

import _sort_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"
BAND, WS_BAND = 64, 4096
SENTINEL = {torch.int64: -0x0123456789ABCDEF, torch.int32: -0x01234567, torch.uint8: 0xA5}


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd

    return gsplat_amd


@pytest.fixture(params=["f64", "int"])
def network(request, monkeypatch):
    """Both sorting networks: GSX_ISECT_SORT unset (lists take the f64 network unless a key forbids it), and =int."""
    monkeypatch.delenv("GSX_ISECT_SORT", raising=False)
    if request.param == "int":
        monkeypatch.setenv("GSX_ISECT_SORT", "int")
    return request.param


def cpu(t):
    return t.detach().cpu()


def _banded(n, dtype, data=None):
    """Device buffer of n elements followed by a band of sentinels; the first n hold `data` (CPU tensor) or sentinels."""
    t = torch.full((n + BAND,), SENTINEL[dtype], dtype=dtype, device=DEV)
    if data is not None:
        t[:n] = data.to(DEV)
    return t


def _workspace(need):
    return torch.full((need + WS_BAND,), SENTINEL[torch.uint8], dtype=torch.uint8, device=DEV)


def _band_intact(t, n):
    return bool((t[n:] == SENTINEL[t.dtype]).all())


def _untouched(t, n):
    return bool((t[:n] == SENTINEL[t.dtype]).all())


# ---- A: scan ---------------------------------------------------------------------------------------------------------------
def _scan_raw(x_cpu):
    """gsx_scan_i32 with an exactly sized workspace; checks the bands and the input, returns the n results on the CPU."""
    from gsplat_amd import _cabi

    n = x_cpu.numel()
    need = _cabi.scan_workspace_bytes(n)
    x, out, ws = x_cpu.to(DEV), _banded(n, torch.int64), _workspace(need)
    _cabi.call("gsx_scan_i32", _cabi.ptr(x), n, _cabi.ptr(out), _cabi.ptr(ws), need)
    torch.cuda.synchronize()
    assert _band_intact(out, n), "scan wrote past its output"
    assert _band_intact(ws, need), "scan wrote past its workspace"
    assert torch.equal(cpu(x), x_cpu), "scan changed its input"
    return cpu(out[:n])


def _scan_cases():
    return [(n, f) for n in sc.SCAN_SIZES for f in sc.SCAN_FAMILIES + (("int32-max",) if n in sc.SCAN_MAX_SIZES else ())]


@pytest.mark.parametrize("n,family", _scan_cases())
def test_scan_at_chunk_and_carry_boundaries(G, n, family):
    """Chunks of 4096, rounds of 256 chunks: the last two sizes have 257 and 513 chunks (the carry is used once, twice - only
    the 513-chunk size tells a carry that accumulates from one that is overwritten). Negative addends, a lone 1 at either end,
    and (at two sizes) sums far above 2^31; through the raw call with guard bands and through _ops._scan_i32."""
    from gsplat_amd._ops import _scan_i32

    x = sc.scan_values(n, family)
    ref = sc.scan_reference(x)
    got = _scan_raw(x)
    if not torch.equal(got, ref):
        bad = int(torch.nonzero(got != ref)[0])
        raise AssertionError(f"first difference at {bad} of {n}: {int(got[bad])} != {int(ref[bad])}")
    assert torch.equal(cpu(_scan_i32(x.to(DEV))), ref), "through _ops._scan_i32"


def test_scan_host_behaviour(G):
    from gsplat_amd import _cabi

    _cabi.call("gsx_scan_i32", None, 0, None, None, 0)  # n = 0: OK, nothing to touch
    n = 4097
    need = _cabi.scan_workspace_bytes(n)
    x, out, ws = sc.scan_values(n, "rand-nonneg").to(DEV), _banded(n, torch.int64), _workspace(need)
    with pytest.raises(_cabi.GsplatAmdError):
        _cabi.call("gsx_scan_i32", _cabi.ptr(x), n, _cabi.ptr(out), _cabi.ptr(ws), need - 1)
    torch.cuda.synchronize()
    assert _untouched(out, n) and _band_intact(out, n) and _band_intact(ws, 0), "a refused call must not write"


# ---- B: radix sort ---------------------------------------------------------------------------------------------------------
def _sort_pairs(keys_cpu, end_bit, ws=None, need=None):
    """gsx_sort_pairs on values = arange(n). Returns the four banded device buffers and result_in_alt."""
    from gsplat_amd import _cabi

    n = keys_cpu.numel()
    need = _cabi.sort_workspace_bytes(n) if need is None else need
    ws = _workspace(need) if ws is None else ws
    k, v = _banded(n, torch.int64, keys_cpu), _banded(n, torch.int32, torch.arange(n, dtype=torch.int32))
    k2, v2 = _banded(n, torch.int64), _banded(n, torch.int32)
    in_alt = _cabi.sort_pairs(k[:n], v[:n], k2[:n], v2[:n], n, end_bit, ws[:need])
    torch.cuda.synchronize()
    for name, t in (("keys", k), ("vals", v), ("keys_alt", k2), ("vals_alt", v2)):
        assert _band_intact(t, n), f"sort wrote past {name}"
    assert _band_intact(ws, need), "sort wrote past its workspace"
    return (k, v, k2, v2), in_alt


@pytest.mark.parametrize("family", sc.RADIX_FAMILIES)
@pytest.mark.parametrize("end_bit", sc.RADIX_END_BITS)
@pytest.mark.parametrize("n", sc.RADIX_SIZES)
def test_radix_sort_sizes_end_bits_and_key_families(G, n, end_bit, family):
    """Wave run (64 / 1024) and workgroup chunk (4096) edges x every end_bit class (0, below a digit, a whole digit, one bit
    into the next, 64 with bit 63 set) x key families, the dead-lane pad value (all ones) among them. Values are arange(n), so
    the stable order is the only right answer; result_in_alt names the buffer that holds it."""
    keys = sc.radix_keys(n, end_bit, family)
    (k, v, k2, v2), in_alt = _sort_pairs(keys, end_bit)
    assert int(in_alt) == ((end_bit + 7) // 8) & 1, "result_in_alt"
    if end_bit == 0:  # nothing to sort by: both buffer pairs stay as they were
        assert torch.equal(cpu(k[:n]), keys) and torch.equal(cpu(v[:n]), torch.arange(n, dtype=torch.int32))
        assert _untouched(k2, n) and _untouched(v2, n)
        return
    ek, ev = sc.radix_reference(keys, end_bit)
    ks, vs = (k2, v2) if in_alt else (k, v)
    assert torch.equal(cpu(ks[:n]), ek), "sorted keys differ"
    assert torch.equal(cpu(vs[:n]), ev), "values differ (stability)"


@pytest.mark.parametrize("end_bit", sc.RADIX_ABOVE_END_BITS)
@pytest.mark.parametrize("n", sc.RADIX_SIZES)
def test_radix_sort_ignores_bits_at_and_above_end_bit(G, n, end_bit):
    """The contract is a sort by key bits [0, end_bit): a key bit at or above end_bit is carried along and moves nothing
    (end_bit 9 and 46 both end inside a digit)."""
    keys = sc.radix_keys(n, end_bit, "above-end-bit")
    (k, v, k2, v2), in_alt = _sort_pairs(keys, end_bit)
    assert int(in_alt) == ((end_bit + 7) // 8) & 1
    ek, ev = sc.radix_reference(keys, end_bit)
    ks, vs = (k2, v2) if in_alt else (k, v)
    assert torch.equal(cpu(ks[:n]), ek), "full keys must come out in the order of their low end_bit bits"
    assert torch.equal(cpu(vs[:n]), ev), "values differ (stability under the mask)"


def test_radix_sort_short_workspace_raises(G):
    from gsplat_amd import _cabi

    n = 4097
    need = _cabi.sort_workspace_bytes(n)
    with pytest.raises(_cabi.GsplatAmdError):
        _sort_pairs(sc.radix_keys(n, 46, "random"), 46, need=need - 1)


# ---- C: gsx_isect_tile_sort, direct ----------------------------------------------------------------------------------------
def _tile_sort(keys, vals, I, tw, th, need=None):
    """gsx_isect_tile_sort with guard bands; checks bands and inputs, returns (sorted keys, sorted ids) on the CPU."""
    from gsplat_amd import _cabi

    n = keys.numel()
    need = _cabi.tile_sort_workspace_bytes(n, I, tw, th) if need is None else need
    kd, vd = keys.to(DEV), vals.to(DEV)
    ko, vo, ws = _banded(n, torch.int64), _banded(n, torch.int32), _workspace(need)
    _cabi.call("gsx_isect_tile_sort", _cabi.ptr(kd), _cabi.ptr(vd), n, I, tw, th, _cabi.ptr(ko), _cabi.ptr(vo), _cabi.ptr(ws), need)
    torch.cuda.synchronize()
    assert _band_intact(ko, n) and _band_intact(vo, n), "tile sort wrote past its outputs"
    assert _band_intact(ws, need), "tile sort wrote past its workspace"
    assert torch.equal(cpu(kd), keys) and torch.equal(cpu(vd), vals), "tile sort changed its inputs"
    return cpu(ko[:n]), cpu(vo[:n])


def _assert_lists_equal(got_k, got_v, exp_k, exp_v, n_tiles):
    if torch.equal(got_k, exp_k) and torch.equal(got_v, exp_v):
        return
    bad = int(torch.nonzero((got_k != exp_k) | (got_v != exp_v))[0])
    hi = int(exp_k[bad]) >> 32
    tb = sc.bits_for(n_tiles)
    lin = (hi >> tb) * n_tiles + (hi & ((1 << tb) - 1))
    length = int(((exp_k >> 32) == hi).sum())
    raise AssertionError(f"first difference at entry {bad}: bin {lin} (list of {length}); got key {int(got_k[bad]):#x} id "
                         f"{int(got_v[bad])}, expected key {int(exp_k[bad]):#x} id {int(exp_v[bad])}")


@pytest.mark.parametrize("family", sc.DEPTH_FAMILIES)
def test_tile_sort_every_length_regime(G, network, family):
    """Lists of 0, 1, 2, 127 .. 129, 255 .. 257, 2047 .. 2049, 9151 .. 9153 and 20 000 entries in one call (2 images of 5 x 3
    tiles, first and last bin empty): every size class of the per-tile sort from both sides, under both networks."""
    I, tw, th = sc.TILE_SORT_GRID
    keys, vals, (ek, ev) = sc.tile_sort_case(family)
    gk, gv = _tile_sort(keys, vals, I, tw, th)
    _assert_lists_equal(gk, gv, ek, ev, tw * th)


def test_tile_sort_ids_up_to_int32_max(G, network):
    """Flatten ids are the low mantissa bits of the f64 network's words: ids spread up to 2^31 - 1."""
    I, tw, th = sc.TILE_SORT_GRID
    keys, vals, (ek, ev) = sc.tile_sort_case("normal", spread_ids=True)
    gk, gv = _tile_sort(keys, vals, I, tw, th)
    _assert_lists_equal(gk, gv, ek, ev, tw * th)


def test_tile_sort_single_tile_three_images(G, network):
    """n_tiles == 1: tile_bits == 0, the image id sits right above the depth."""
    keys, vals, (ek, ev) = sc.tile_sort_case("ties", lengths=(200, 0, 3000), grid=(3, 1, 1))
    gk, gv = _tile_sort(keys, vals, 3, 1, 1)
    _assert_lists_equal(gk, gv, ek, ev, 1)


def test_tile_sort_at_the_bin_limit(G):
    """36 864 bins (192 x 192 tiles), 1.2 M entries: the [bin][chunk] table has 36 864 x 37 > 1 048 576 entries (334 chunks: two
    rounds of 256), so the int32 exclusive scan behind the bucketing uses its carry once. That the carry accumulates over further
    rounds is pinned by the 513-chunk scan above: both instantiations share the kernel that carries."""
    from gsplat_amd import _cabi

    keys, vals, (ek, ev) = sc.tile_sort_max_bins_case()
    assert _cabi.tile_sort_supported(1, 192, 192)
    gk, gv = _tile_sort(keys, vals, 1, 192, 192)
    _assert_lists_equal(gk, gv, ek, ev, sc.MAX_BINS)


def test_tile_sort_refuses_what_it_cannot_do(G):
    from gsplat_amd import _cabi

    assert _cabi.tile_sort_supported(1, 36864, 1) and not _cabi.tile_sort_supported(1, 36865, 1)
    keys, vals, _ = sc.tile_sort_case("normal", lengths=(200, 0, 3000), grid=(3, 1, 1))
    with pytest.raises(ValueError):  # one bin too many for the LDS histogram (GSX_ERR_ARG)
        _tile_sort(keys, vals, 1, 36865, 1)
    with pytest.raises(_cabi.GsplatAmdError):  # workspace one byte short
        _tile_sort(keys, vals, 3, 1, 1, need=_cabi.tile_sort_workspace_bytes(keys.numel(), 3, 1, 1) - 1)


# ---- D: exact list lengths through isect_tiles, both paths -------------------------------------------------------------------
@pytest.mark.parametrize("family", sc.ISECT_FAMILIES)
@pytest.mark.parametrize("path", ["binned", "legacy"])
@pytest.mark.parametrize("layout", sorted(sc.ISECT_LAYOUTS))
def test_isect_exact_list_lengths(G, monkeypatch, network, layout, path, family):
    """Hand-built rows (radius-box mode, one image of 16 x 8 tiles of 16 px, every row inside one tile) give lists of exactly
    64 / 65 (one wave's floor), 512 / 513 (a list's share of the binned path's arena), 4096 / 4097 (the arena / the work list),
    9152 / 9153 (the work list's LDS / global memory), several lists that overflow the arena together (two batches), and a
    work-list tile beside arena tiles in one workgroup - through the tile-owner-major and the Gaussian-major path, which must
    really be the one that ran."""
    from gsplat_amd import _cabi

    tw, th, ts = sc.ISECT_GRID
    c = sc.isect_case(layout, family)
    m2, rad, d = c["means2d"].to(DEV), c["radii"].to(DEV), c["depths"].to(DEV)
    monkeypatch.setenv("GSX_ISECT_PATH", path)
    _cabi.profile_begin()
    try:
        tpg, ids, fl = G.isect_tiles(m2, rad, d, ts, tw, th)
        torch.cuda.synchronize()
    finally:
        ran = set(_cabi.profile_end())
    off = G.isect_offset_encode(ids, 1, tw, th)
    if path == "binned":
        assert {"gsx_isect_binned_count", "gsx_isect_binned_emit_sort"} <= ran, sorted(ran)
        assert "gsx_isect_fused_emit_sort" not in ran, "the binned path sent the call back"
    else:
        assert not any("binned" in k for k in ran) and "gsx_isect_fused_emit_sort" in ran, sorted(ran)
    assert torch.equal(cpu(tpg), torch.ones_like(c["radii"][..., 0])), "every row touches exactly one tile"
    _assert_lists_equal(cpu(ids), cpu(fl), c["isect_ids"], c["flatten_ids"], tw * th)
    assert torch.equal(cpu(off), c["offsets"]), "offsets = exclusive cumsum of the list lengths"


# ---- E: isect_offset_encode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.OFFSET_CASES))
def test_offset_encode_on_hand_built_ids(G, name):
    I, tw, th, _ = sc.OFFSET_CASES[name]
    keys, ref = sc.offset_case(name)
    off = G.isect_offset_encode(keys.to(DEV), I, tw, th)
    assert off.dtype == torch.int32 and tuple(off.shape) == (I, th, tw)
    assert torch.equal(cpu(off), ref)
