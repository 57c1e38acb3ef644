"""Case builders and CPU references for the three integer primitives ahead of compositing - the device-wide prefix sum, the LSD
radix sort (csrc/scan_sort.hip) and the per-tile sorts (csrc/tile_sort.hip, csrc/bitonic64.hpp, csrc/isect_binned.hip) - at the
sizes and bit patterns where each of them changes algorithm. Shared by tests/test_sort_cases.py (CPU: the builders build what
they claim) and tests/test_gpu_sort_edges.py (GPU: the kernels against the references). Everything here is seeded numpy / torch
on the CPU; every comparison made with it is exact.

References: scan = torch.cumsum on int64; sorts = numpy's stable argsort of the keys read as UNSIGNED 64-bit; offsets =
searchsorted on the linearised (image, tile)."""
import functools

import numpy as np
import torch

MASK32 = 0xFFFFFFFF
INT32_MAX = 2**31 - 1

# ---- which sorting network a list takes (csrc/bitonic64.hpp: bt_key_is_odd) ------------------------------------------------
# The f64 network is valid while every depth's float bits lie in [ODD_LO, ODD_HI); any other key sends its list to the integer one.
ODD_LO, ODD_HI = 0x00100000, 0x7FF00000
EDGE_BITS = (0x00000000, 0x00000001, 0x000FFFFF, 0x00100000, 0x00100001, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x7FC00000,
             0x7FEFFFFF, 0x7FF00000, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xBF800000, 0xFF800000, 0xFFFFFFFF)
# The tie pass behind the radix sorts of long lists is quadratic in the run length (documented; not what these cases are about):
# no depth value occurs more than RUN_BOUND times in a list longer than RUN_BOUND_ABOVE entries.
RUN_BOUND, RUN_BOUND_ABOVE = 32, 2048


def key_is_odd(depth_bits):
    """bt_key_is_odd restated from its documented range: odd = outside [0x00100000, 0x7FF00000)."""
    b = np.asarray(depth_bits).astype(np.uint64)
    return ~((b >= ODD_LO) & (b < ODD_HI))


def bits_for(count):
    return 0 if count <= 1 else int(count - 1).bit_length()


def _u64(t):
    return t.numpy().view(np.uint64)


def _i64(a):
    return torch.from_numpy(np.array(a, dtype=np.uint64, order="C", copy=True).view(np.int64))


def stable_order(keys):
    """Indices of a stable ascending sort of int64 `keys` read as unsigned 64-bit."""
    return torch.from_numpy(np.argsort(_u64(keys), kind="stable"))


# ---- A: scan ---------------------------------------------------------------------------------------------------------------
SCAN_CHUNK = 4096  # elements per workgroup; the chunk sums are scanned in rounds of 256 chunks (carry beyond 1 048 576 elements)
SCAN_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 1_048_575, 1_048_576, 1_048_577, 2_097_153)
SCAN_FAMILIES = ("rand-nonneg", "rand-signed", "one-first", "one-last")
SCAN_MAX_SIZES = (8192, 1_048_577)  # all INT32_MAX: sums far above 2^31


def scan_values(n, family):
    g = torch.Generator().manual_seed(n)
    if family == "rand-nonneg":
        return torch.randint(0, 50, (n,), generator=g, dtype=torch.int32)
    if family == "rand-signed":
        return torch.randint(-50, 50, (n,), generator=g, dtype=torch.int32)
    if family == "int32-max":
        return torch.full((n,), INT32_MAX, dtype=torch.int32)
    x = torch.zeros(n, dtype=torch.int32)
    x[{"one-first": 0, "one-last": n - 1}[family]] = 1
    return x


def scan_reference(x):
    return torch.cumsum(x.long(), 0)


# ---- B: radix sort ---------------------------------------------------------------------------------------------------------
RADIX_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8193, 300_001)
RADIX_END_BITS = (0, 1, 8, 9, 32, 46, 63, 64)
RADIX_FAMILIES = ("random", "equal", "ones", "ascending", "descending", "alternating", "top-digit", "bit0")
RADIX_ABOVE_END_BITS = (9, 46)  # the family with bits set at and above end_bit


def radix_mask(end_bit):
    return np.uint64((1 << end_bit) - 1)


def radix_keys(n, end_bit, family):
    """int64 keys of one family, masked to end_bit bits - but `above-end-bit`, and every family at end_bit 0 (where the call
    must touch nothing), keep all 64 random bits."""
    rng = np.random.default_rng(1000 * end_bit + len(family) + 7 * n)
    mask = radix_mask(end_bit)
    full = rng.integers(0, 2**64, n, dtype=np.uint64, endpoint=False)
    if family == "above-end-bit" or end_bit == 0:
        k = full
        if family == "above-end-bit":  # every key carries the bit end_bit itself or a higher one
            k = k | (np.uint64(1) << np.uint64(end_bit + rng.integers(0, 64 - end_bit, n).astype(np.uint64)))
        return _i64(k)
    passes = (end_bit + 7) // 8
    top = np.uint64(8 * (passes - 1))
    if family == "random":
        k = full & mask
    elif family == "equal":
        k = np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64) & mask
    elif family == "ones":  # at end_bit 64 this is the value dead lanes are padded with
        k = np.full(n, mask, dtype=np.uint64)
    elif family in ("ascending", "descending"):
        stride = np.uint64(max(1, int(mask) // max(n, 1)))  # spans every digit when the range allows; wraps below n values
        k = (np.arange(n, dtype=np.uint64) * stride) & mask
        if family == "descending":
            k = k[::-1]
    elif family == "alternating":
        two = np.array([0xAAAAAAAAAAAAAAAA, 0x5555555555555555], dtype=np.uint64) & mask
        k = two[np.arange(n) & 1]
    elif family == "top-digit":
        low = np.uint64(0x0123456789ABCDEF) & ((np.uint64(1) << top) - np.uint64(1))
        k = (low | (rng.integers(0, 256, n).astype(np.uint64) << top)) & mask
    elif family == "bit0":
        k = ((np.uint64(0x5A5A5A5A5A5A5A5A) & ~np.uint64(1)) | (full & np.uint64(1))) & mask
    else:
        raise KeyError(family)
    return _i64(k)


def radix_reference(keys, end_bit):
    """(keys, values) after a stable sort by key & (2^end_bit - 1), unsigned, of values = arange(n); full keys carried along."""
    vals = torch.arange(keys.numel(), dtype=torch.int32)
    order = torch.from_numpy(np.argsort(_u64(keys) & radix_mask(end_bit), kind="stable"))
    return keys[order], vals[order]


# ---- depth families --------------------------------------------------------------------------------------------------------
DEPTH_FAMILIES = ("normal", "ties", "edge-bits", "one-odd")


def _normals(rng, n):
    return (rng.random(n, dtype=np.float32) * np.float32(10.0) + np.float32(0.1)).view(np.uint32)


def enforce_run_bound(bits, rng):
    """In a list longer than RUN_BOUND_ABOVE, occurrences of one value beyond the first RUN_BOUND become fresh normals."""
    if bits.size <= RUN_BOUND_ABOVE:
        return bits
    bits = bits.copy()
    while True:
        _, inv, counts = np.unique(bits, return_inverse=True, return_counts=True)
        if counts.max() <= RUN_BOUND:
            return bits
        order = np.argsort(inv, kind="stable")  # positions grouped by value, in list order
        rank = np.arange(bits.size) - np.repeat(np.cumsum(counts) - counts, counts)
        excess = order[rank >= RUN_BOUND]
        bits[excess] = _normals(rng, excess.size)


def depth_bits(n, family, rng):
    """uint32 float bits of one list's depths, in emission order."""
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    d = _normals(rng, n)
    if family == "ties":  # short lists: ~200 values; long lists: ~4 entries per value
        q = np.float32(20.0) if n <= RUN_BOUND_ABOVE else np.float32(n / 40.0)
        d = (np.round(d.view(np.float32) * q) / q + np.float32(0.25)).astype(np.float32).view(np.uint32)
    elif family == "edge-bits":  # 1 : 4 with normals
        edge = rng.random(n) < 0.2
        d = np.where(edge, np.array(EDGE_BITS, dtype=np.uint32)[rng.integers(0, len(EDGE_BITS), n)], d)
    elif family == "one-odd":  # one key flips the whole list to the integer network
        d[-1] = ODD_HI
    elif family != "normal":
        raise KeyError(family)
    return enforce_run_bound(d.astype(np.uint32), rng)


def _deal(lengths, family, rng):
    """Entries of the lists interleaved: (list index per entry, depth bits per entry), both in emission order."""
    lengths = np.asarray(lengths, dtype=np.int64)
    which = rng.permutation(np.repeat(np.arange(lengths.size), lengths))
    bits = np.zeros(which.size, dtype=np.uint32)
    for b in np.flatnonzero(lengths):
        bits[which == b] = depth_bits(int(lengths[b]), family, rng)
    return which, bits


# ---- C: gsx_isect_tile_sort, direct ----------------------------------------------------------------------------------------
# one call: every threshold of the per-tile sort (128: smallest network, 2048: last bitonic size, 9152: LDS capacity) from
# both sides, the global-memory path (20 000), bins of both images, the first and the last bin empty
TILE_SORT_GRID = (2, 5, 3)  # images, tile_w, tile_h: 15 tiles, no power of two - the key space has a hole
TILE_SORT_LENGTHS = (0, 0, 1, 2, 127, 128, 129, 255, 0, 256, 257, 2047, 2048, 9151, 0,
                     2049, 9152, 0, 9153, 0, 20000, 0, 0, 0, 0, 0, 0, 0, 0, 0)
TILE_SORT_WANTED = (0, 1, 2, 127, 128, 129, 255, 256, 257, 2047, 2048, 2049, 9151, 9152, 9153, 20000)
MAX_BINS = 36864


def tile_keys(which, bits, n_tiles):
    """int64 keys (image << tile_bits | tile) << 32 | depth bits of entries of bins `which` (image-major)."""
    tb = bits_for(n_tiles)
    img, tile = which.astype(np.uint64) // np.uint64(n_tiles), which.astype(np.uint64) % np.uint64(n_tiles)
    hi = (img << np.uint64(tb)) | tile
    return _i64((hi << np.uint64(32)) | (bits.astype(np.uint64) & np.uint64(MASK32)))


def _spread_ids(n, rng):
    """n ascending ids spread over [0, 2^31 - 1], the last one 2^31 - 1."""
    ids = np.sort(rng.choice(INT32_MAX, size=n - 1, replace=False)) if n > 1 else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(np.concatenate([ids, [INT32_MAX]]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def tile_sort_case(family, lengths=TILE_SORT_LENGTHS, grid=TILE_SORT_GRID, spread_ids=False, seed=0):
    """(keys int64 [n], vals int32 [n], (expected keys, expected vals)) for lists of the given per-bin lengths. Entries of
    different bins are interleaved; vals (the flatten ids) ascend in emission order. Shared: do not modify."""
    I, tw, th = grid
    assert len(lengths) == I * tw * th
    rng = np.random.default_rng(seed + 17 * DEPTH_FAMILIES.index(family))
    which, bits = _deal(lengths, family, rng)
    keys = tile_keys(which, bits, tw * th)
    vals = _spread_ids(which.size, rng) if spread_ids else torch.arange(which.size, dtype=torch.int32)
    order = stable_order(keys)
    return keys, vals, (keys[order], vals[order])


@functools.lru_cache(maxsize=None)
def tile_sort_max_bins_case(n=1_200_000, seed=3):
    """36 864 bins (the limit), random entries: the [bin][chunk] table has 36 864 x 37 > 1 048 576 entries."""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, MAX_BINS, n)
    keys = tile_keys(which, _normals(rng, n), MAX_BINS)
    vals = torch.arange(n, dtype=torch.int32)
    order = stable_order(keys)
    return keys, vals, (keys[order], vals[order])


# ---- D: exact list lengths through isect_tiles -------------------------------------------------------------------------------
ISECT_GRID = (16, 8, 16)  # tile_w, tile_h, tile_size: one image; the binned path's bins are 4 x 2 tiles -> 4 x 4 bins


def _bin_tiles(bx, by):
    return [(4 * bx + x, 2 * by + y) for y in range(2) for x in range(4)]


ISECT_LAYOUTS = {  # name: [((tile x, tile y), list length), ...]
    # single lists in eight different bins: one wave's 64-word floor, the 512-word share of the arena, the arena itself
    # (4096 words), the work list's LDS capacity (9152) - each from both sides
    "singles": list(zip([(0, 0), (4, 0), (8, 0), (12, 0), (1, 2), (5, 3), (10, 4), (15, 6)],
                        [64, 65, 512, 513, 4096, 4097, 9152, 9153])),
    "two-2049": [((4, 2), 2049), ((5, 3), 2049)],  # one bin, padded 4096 + 4096: two batches
    "eight-513": [(t, 513) for t in _bin_tiles(2, 1)],  # one bin, 8 x 1024: two batches
    "4097-and-seven-100": [(t, 4097 if i == 3 else 100) for i, t in enumerate(_bin_tiles(0, 3))],  # work list + arena
    "last-tile": [((15, 7), 3000)],
}
ISECT_FAMILIES = ("normal", "edge-bits")


@functools.lru_cache(maxsize=None)
def isect_case(layout, family, seed=0):
    """Hand-built rows for isect_tiles in radius-box mode: every row sits at the centre of its tile with radius 1, so it lands in
    exactly that tile and each list length is exact. Returns a dict of CPU tensors: the inputs (means2d [1, N, 2], radii
    [1, N, 2], depths [1, N]), `lengths` per tile and the expected isect_ids, flatten_ids, offsets [1, th, tw]."""
    tw, th, ts = ISECT_GRID
    lengths = np.zeros(tw * th, dtype=np.int64)
    for (tx, ty), n in ISECT_LAYOUTS[layout]:
        lengths[ty * tw + tx] = n
    rng = np.random.default_rng(seed + 31 * sorted(ISECT_LAYOUTS).index(layout) + 7 * DEPTH_FAMILIES.index(family))
    tile, bits = _deal(lengths, family, rng)
    N = tile.size
    means = np.stack([(tile % tw) * ts + ts / 2, (tile // tw) * ts + ts / 2], axis=-1).astype(np.float32)
    keys = tile_keys(tile, bits, tw * th)
    order = stable_order(keys)
    offsets = np.cumsum(lengths) - lengths
    return dict(means2d=torch.from_numpy(means).reshape(1, N, 2), radii=torch.ones(1, N, 2, dtype=torch.int32),
                depths=torch.from_numpy(bits.view(np.float32).copy()).reshape(1, N), depth_bits=bits, tile=tile, lengths=lengths,
                keys=keys, isect_ids=keys[order], flatten_ids=torch.arange(N, dtype=torch.int32)[order],
                offsets=torch.from_numpy(offsets.astype(np.int32)).reshape(1, th, tw))


# ---- E: isect_offset_encode ------------------------------------------------------------------------------------------------
def _every_tile_once(I, tw, th):
    return [(b, 1) for b in range(I * tw * th)]


OFFSET_CASES = {  # name: (images, tile_w, tile_h, [(bin, entries), ...] ascending)
    "last-tile-of-last-image": (3, 5, 3, [(44, 7)]),
    "empty-middle-image": (3, 5, 3, [(0, 2), (7, 300), (14, 1), (30, 5), (44, 1)]),
    "one-entry": (2, 5, 3, [(16, 1)]),
    "every-tile-once": (2, 5, 3, _every_tile_once(2, 5, 3)),
    "one-tile-three-images": (3, 1, 1, [(0, 4), (2, 70)]),
}


def offset_case(name):
    """(sorted isect_ids int64 [n], expected offsets int32 [I, th, tw])."""
    I, tw, th, occupied = OFFSET_CASES[name]
    n_tiles = tw * th
    rng = np.random.default_rng(len(name))
    which = np.repeat([b for b, _ in occupied], [c for _, c in occupied])
    keys = tile_keys(which, _normals(rng, which.size), n_tiles)
    keys = keys[stable_order(keys)]
    return keys, offsets_reference(keys, I, tw, th)


def offsets_reference(sorted_keys, I, tw, th):
    """searchsorted on the linearised (image, tile) of the sorted keys."""
    n_tiles = tw * th
    hi = _u64(sorted_keys) >> np.uint64(32)
    tb = np.uint64(bits_for(n_tiles))
    lin = (hi >> tb) * np.uint64(n_tiles) + (hi & ((np.uint64(1) << tb) - np.uint64(1)))
    off = np.searchsorted(lin, np.arange(I * n_tiles, dtype=np.uint64), side="left")
    return torch.from_numpy(off.astype(np.int32)).reshape(I, th, tw)
