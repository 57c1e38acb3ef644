"""GPU: the per-Gaussian chain of the one-wave-per-tile compositing backward (csrc/raster3d_bwd.hip, variant W) at the sizes
where its bookkeeping can go wrong: the four slots of a turn and the partial turn at a batch end, the 64-entry batches, the
quadrant masks, the conversion of a turn's sums into the columns of a gradient row, image edges and options, and the flatten
id that rides through the staged row as the bits of a float.

Every case goes through the public compositing op (rasterize_to_pixels forward, then backward) on tile lists written by hand -
the op takes the lists as inputs, so a list has exactly the entries a case needs - and is compared element by element with the
fp64 backward of the oracle inside the per-element band of tests/_util.py (RASTER_BWD_BAND), nothing wider. Contributors are
small (sigma 0.8 .. 2 px) and moderately opaque, so that no pixel terminates early and the sums stay well conditioned."""
import math

import numpy as np
import pytest
import torch

from _util import RASTER_BWD_BAND

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = ("v_means2d", "v_conics", "v_colors", "v_opacities")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd

    return gsplat_amd


# ---- Gaussians by role ------------------------------------------------------------------------------------------------------
def _conic(sx, sy, theta=0.0):
    """inverse covariance (a, b, c) of a Gaussian with standard deviations sx, sy along axes rotated by theta"""
    c, s = math.cos(theta), math.sin(theta)
    a = c * c / sx ** 2 + s * s / sy ** 2
    b = c * s * (1.0 / sx ** 2 - 1.0 / sy ** 2)
    cc = s * s / sx ** 2 + c * c / sy ** 2
    return (a, b, cc)


class Scene:
    """Rows of Gaussians (means2d, conics, opacities) collected by role, and per-tile lists of row indices."""

    def __init__(self, seed, W=16, H=16):
        self.rng = np.random.RandomState(seed)
        self.W, self.H = W, H
        self.tw, self.th = (W + 15) // 16, (H + 15) // 16
        self.m, self.c, self.o = [], [], []
        self.lists = [[] for _ in range(self.tw * self.th)]

    def _add(self, xy, conic, opac, tile):
        self.m.append(xy), self.c.append(conic), self.o.append(opac)
        self.lists[tile].append(len(self.m) - 1)
        return len(self.m) - 1

    def _origin(self, tile):
        return 16.0 * (tile % self.tw), 16.0 * (tile // self.tw)

    def contributor(self, tile=0, xy=None, sigma=None, opac=None):
        """reaches some pixel of the tile: sigma 0.8 .. 2 px, anywhere in the tile"""
        r = self.rng
        ox, oy = self._origin(tile)
        if xy is None:
            xy = (ox + r.uniform(1.0, 15.0), oy + r.uniform(1.0, 15.0))
        if sigma is None:
            sigma = (r.uniform(0.8, 2.0), r.uniform(0.8, 2.0))
        return self._add(xy, _conic(sigma[0], sigma[1], r.uniform(0, math.pi)), r.uniform(0.15, 0.6) if opac is None else opac, tile)

    def walked_only(self, tile=0):
        """Passes the staging test of its quadrant (the mean lies inside the rectangle of pixel centres) but reaches no pixel:
        sigma 0.13 px on a pixel CORNER, 0.71 px from the nearest centres, where alpha = 0.5 exp(-15)."""
        r = self.rng
        ox, oy = self._origin(tile)
        return self._add((ox + float(r.randint(1, 15)), oy + float(r.randint(1, 15))), (60.0, 0.0, 60.0), 0.5, tile)

    def far(self, tile=0):
        """staged, then culled for every quadrant: 200 px away"""
        return self._add((self.W + 200.0, self.H + 200.0), _conic(1.0, 1.0), 0.5, tile)

    def tensors(self, channels=3, pad_rows=0):
        g = torch.Generator().manual_seed(int(self.rng.randint(1 << 30)))
        n = len(self.m)
        m2 = torch.tensor(self.m, dtype=torch.float32).reshape(n, 2)
        con = torch.tensor(self.c, dtype=torch.float32).reshape(n, 3)
        op = torch.tensor(self.o, dtype=torch.float32).reshape(n)
        col = torch.rand(n, channels, generator=g)
        off, fl, pos = [], [], 0
        for lst in self.lists:
            off.append(pos)
            fl += lst
            pos += len(lst)
        off = torch.tensor(off, dtype=torch.int32).reshape(1, self.th, self.tw)
        fl = torch.tensor(fl, dtype=torch.int32)
        v_rc = torch.randn(1, self.H, self.W, channels, generator=g)
        v_ra = torch.randn(1, self.H, self.W, 1, generator=g)
        return dict(m2=m2, con=con, col=col, op=op, off=off, fl=fl, v_rc=v_rc, v_ra=v_ra, W=self.W, H=self.H)


# ---- one case: GPU forward + backward against the oracle's fp64 backward ------------------------------------------------------
def _gpu(G, t, backgrounds=None, masks=None, with_v_ra=True, absgrad=False, ids=None, n_rows=None):
    """gradients of the public op; `ids` / `n_rows`: the same rows scattered into a larger (padded) Gaussian array"""
    rows = {k: t[k] for k in ("m2", "con", "col", "op")}
    fl = t["fl"]
    if ids is not None:
        big = {k: torch.zeros((n_rows,) + tuple(v.shape[1:]), device=DEV) for k, v in rows.items()}
        big["con"][:, 0] = 1.0
        big["con"][:, 2] = 1.0
        for k, v in rows.items():
            big[k][ids.to(DEV)] = v.to(DEV)
        rows, fl = big, ids[t["fl"].long()].to(torch.int32)
    leaves = [rows[k].to(DEV).clone().requires_grad_(True) for k in ("m2", "con", "col", "op")]
    bg = None if backgrounds is None else backgrounds.to(DEV)
    mk = None if masks is None else masks.to(DEV)
    rc, ra = G.rasterize_to_pixels(leaves[0], leaves[1], leaves[2], leaves[3], t["W"], t["H"], 16, t["off"].to(DEV),
                                   fl.to(DEV), backgrounds=bg, masks=mk, packed=True, absgrad=absgrad)
    loss = (rc * t["v_rc"].to(DEV)).sum()
    if with_v_ra:
        loss = loss + (ra * t["v_ra"].to(DEV)).sum()
    loss.backward()
    out = {k: l.grad.detach() for k, l in zip(KEYS, leaves)}
    if absgrad:
        out["v_means2d_abs"] = leaves[0].absgrad.detach()
    out["render_colors"], out["render_alphas"] = rc.detach(), ra.detach()
    return out


def _oracle(t, backgrounds=None, masks=None, with_v_ra=True, absgrad=False):
    from oracle import oracle as O

    args = (t["m2"], t["con"], t["col"], t["op"], t["W"], t["H"], 16, t["off"], t["fl"])
    rc, ra, li = O.rasterize_to_pixels(*args, backgrounds=backgrounds, masks=masks)
    v_ra = t["v_ra"] if with_v_ra else torch.zeros_like(t["v_ra"])
    ref = O.rasterize_to_pixels_bwd(*args, ra, li, t["v_rc"], v_ra, backgrounds=backgrounds, masks=masks, absgrad=absgrad,
                                    sample_f64=True)
    ref["render_colors"], ref["render_alphas"], ref["last_ids"] = rc, ra, li
    return ref


def _in_band(got, ref, name, keys=KEYS, rows=None):
    """|gpu - fp64| <= atol + rtol |fp64| for EVERY element, with the (rtol, atol) of RASTER_BWD_BAND; prints the worst ratio"""
    worst = {}
    for key in keys:
        rtol, atol = RASTER_BWD_BAND["v_means2d" if key == "v_means2d_abs" else key]
        a = (got[key] if rows is None else got[key][rows.to(got[key].device)]).double().cpu()
        e = torch.as_tensor(ref[key]).double().reshape(a.shape)
        ratio = ((a - e).abs() / (atol + rtol * e.abs())).max().item() if a.numel() else 0.0
        worst[key] = round(ratio, 4)
    print(f"{name}: worst |err| / band = {worst}")
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"{name}: outside the per-element band (ratio > 1): {bad}"


def _run(G, sc, name, channels=3, **opt):
    t = sc.tensors(channels)
    got, ref = _gpu(G, t, **opt), _oracle(t, **opt)
    assert torch.allclose(got["render_alphas"].cpu(), ref["render_alphas"], rtol=1e-4, atol=5e-5), name
    _in_band(got, ref, name, keys=KEYS + (("v_means2d_abs",) if opt.get("absgrad") else ()))
    return t, got, ref


def _contributors_seen(ref, t):
    """rows with a non-zero opacity gradient in the oracle: the Gaussians that reached a pixel"""
    return int((torch.as_tensor(ref["v_opacities"]) != 0).sum())


# ---- slot and turn edges (SLOTS = 4) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_slot_edges(G, n):
    """One tile whose list has n contributing Gaussians: full turns, and a partial turn left open after 1, 2 and 3 slots."""
    sc = Scene(seed=100 + n)
    for _ in range(n):
        sc.contributor()
    t, got, ref = _run(G, sc, f"slots n={n}")
    assert _contributors_seen(ref, t) == n


@pytest.mark.parametrize("channels,absgrad", [(3, False), (4, False), (3, True)])
def test_every_third_entry_contributes(G, channels, absgrad):
    """Entries that are walked without contributing leave the slot where it is: 27 entries, every third one contributes, the
    other two pass staging (mean inside a quadrant's rectangle) and reach no pixel. Also the one run each of the 4-channel
    kernel and of the absgrad kernel, which share the body."""
    sc = Scene(seed=7)
    for i in range(27):
        sc.contributor() if i % 3 == 2 else sc.walked_only()
    t, got, ref = _run(G, sc, f"every third, {channels} channels, absgrad={absgrad}", channels=channels, absgrad=absgrad)
    assert _contributors_seen(ref, t) == 9


# ---- batch edges (BATCH = 64) --------------------------------------------------------------------------------------------------
def _batch_cases():
    for n in (63, 64, 65, 128, 129):
        for last in sorted({0, 63, 64, n - 1}):
            if last < n:
                yield n, last


@pytest.mark.parametrize("n,last", list(_batch_cases()))
def test_batch_edges(G, n, last):
    """A list of n entries whose last contributor is entry `last` (the walk runs back to front from there): entries 0 .. last
    contribute, the ones behind are walked-only or far. Batches of 64 are counted from `last` backwards, so the cases put a
    batch end - and the partial turn it forces - after 1, 2, 3 and 4 filled slots, and leave one-entry batches at either end."""
    sc = Scene(seed=1000 + 7 * n + last)
    for i in range(n):
        if i <= last:
            sc.contributor(opac=sc.rng.uniform(0.05, 0.3))
        else:
            sc.walked_only() if i % 2 else sc.far()
    t, got, ref = _run(G, sc, f"batch n={n} last={last}")
    assert int(ref["last_ids"].max()) == last  # the forward stopped where the case says
    assert _contributors_seen(ref, t) == last + 1


@pytest.mark.parametrize("n", [65, 130])
def test_batch_end_from_every_slot(G, n):
    """Every third entry contributes over more than one batch: the batch ends fall after different numbers of filled slots."""
    sc = Scene(seed=2000 + n)
    for i in range(n):
        sc.contributor(opac=sc.rng.uniform(0.05, 0.3)) if i % 3 == 0 or i == n - 1 else sc.walked_only()
    _run(G, sc, f"every third over batches n={n}")


# ---- quadrant masks ------------------------------------------------------------------------------------------------------------
QUADRANT_CENTRES = [(4.0, 4.0), (12.0, 4.0), (4.0, 12.0), (12.0, 12.0)]


def _quadrant_scene(kind, seed):
    sc = Scene(seed=seed)
    if kind in (0, 1, 2, 3):  # sigma 0.7: alpha >= 1/255 within 2.2 px of the quadrant's centre, 4.5 px from the next quadrant
        sc.contributor(xy=QUADRANT_CENTRES[kind], sigma=(0.7, 0.7), opac=0.5)
    elif kind == "diagonal":  # on the tile centre, along the diagonal: reaches (7.5, 7.5) and (8.5, 8.5), not (8.5, 7.5), (7.5, 8.5)
        sc._add((8.0, 8.0), _conic(2.0, 0.15, math.pi / 4), 0.6, 0)
    elif kind == "antidiagonal":
        sc._add((8.0, 8.0), _conic(2.0, 0.15, -math.pi / 4), 0.6, 0)
    elif kind == "all":
        sc.contributor(xy=(8.2, 7.9), sigma=(2.0, 2.0), opac=0.5)
    elif kind == "none":
        sc.far()
    return sc


@pytest.mark.parametrize("kind", [0, 1, 2, 3, "diagonal", "antidiagonal", "all", "none"])
def test_quadrant_masks(G, kind):
    """A Gaussian that reaches exactly one quadrant (each of the four), two diagonal quadrants, all four, none (culled after
    staging) - alone in the list, and as one entry among contributors of every quadrant."""
    t, got, ref = _run(G, _quadrant_scene(kind, 31), f"quadrant {kind}, alone")
    quads = torch.stack([(ref["last_ids"][0, y:y + 8, x:x + 8] >= 0) & (ref["render_alphas"][0, y:y + 8, x:x + 8, 0] > 0)
                         for y in (0, 8) for x in (0, 8)]).flatten(1).any(1).tolist()
    want = {0: [1, 0, 0, 0], 1: [0, 1, 0, 0], 2: [0, 0, 1, 0], 3: [0, 0, 0, 1], "diagonal": [1, 0, 0, 1],
            "antidiagonal": [0, 1, 1, 0], "all": [1, 1, 1, 1], "none": [0, 0, 0, 0]}[kind]
    assert quads == [bool(w) for w in want], (kind, quads)  # the case reaches the quadrants it is meant to reach
    sc = _quadrant_scene(kind, 32)
    for i in range(6):
        sc.contributor(xy=QUADRANT_CENTRES[i % 4], sigma=(1.2, 0.9), opac=0.3)
    _run(G, sc, f"quadrant {kind}, among others")


# ---- conversion columns --------------------------------------------------------------------------------------------------------
def test_conversion_columns_one_gaussian_per_tile(G):
    """One Gaussian per tile: every gradient row is the output of a single turn, no order of atomics is involved, so two runs
    agree bit for bit and each column (v_means2d x / y, the three conic entries, opacity, each colour) is checked on its own
    against the oracle. Tile 1: opacity 0.999 with the mean exactly on a pixel centre - that pixel has opac exp(-sigma) > 0.99
    and gives no geometry gradient; tile 2: a mean exactly on a pixel centre; tile 3: an anisotropic, rotated footprint."""
    sc = Scene(seed=5, W=64, H=32)
    sc.contributor(tile=0)
    sc._add((16 + 5.5, 9.5), _conic(1.5, 1.1, 0.4), 0.999, 1)
    sc._add((32 + 10.5, 3.5), _conic(1.0, 1.7, 1.1), 0.4, 2)
    sc._add((48 + 7.9, 8.1), _conic(2.0, 0.5, 0.7), 0.5, 3)
    for tile in range(4, 8):
        sc.contributor(tile=tile)
    t = sc.tensors(3)
    a, b, ref = _gpu(G, t), _gpu(G, t), _oracle(t)
    for key in KEYS:
        assert torch.equal(a[key], b[key]), f"{key}: two runs differ although no sum depends on an order"
    assert float(ref["render_alphas"][0, 9, 16 + 5, 0]) == pytest.approx(0.99, abs=1e-6)  # the clamped pixel of tile 1
    _in_band(a, ref, "one Gaussian per tile")
    for key, cols in (("v_means2d", 2), ("v_conics", 3), ("v_colors", 3)):
        for c in range(cols):
            got_c, ref_c = a[key][:, c].cpu().double(), torch.as_tensor(ref[key])[:, c]
            assert (ref_c != 0).all(), (key, c)  # every column of every row carries a value to check
            rtol, atol = RASTER_BWD_BAND[key]
            assert ((got_c - ref_c).abs() <= atol + rtol * ref_c.abs()).all(), (key, c)
    assert (torch.as_tensor(ref["v_opacities"]) != 0).all()


# ---- image edges and options ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", ["plain", "background", "masks", "no_v_alphas", "background+masks"])
def test_image_edges_and_options(G, option):
    """40 x 24 image: partial tiles on the right and at the bottom; with a background, with `masks` skipping a tile, and
    without a cotangent for the alphas."""
    sc = Scene(seed=77, W=40, H=24)
    for tile in range(sc.tw * sc.th):
        for i in range(11):
            sc.contributor(tile=tile) if i % 4 else sc.walked_only(tile=tile)
    opt = {}
    if "background" in option:
        opt["backgrounds"] = torch.tensor([[0.3, 0.6, 0.9]])
    if "masks" in option:
        mk = torch.ones(1, sc.th, sc.tw, dtype=torch.bool)
        mk[0, 1, 1] = False
        opt["masks"] = mk
    if option == "no_v_alphas":
        opt["with_v_ra"] = False
    _run(G, sc, f"40x24 {option}", **opt)


# ---- the flatten id in the staged row -----------------------------------------------------------------------------------------
def test_flatten_ids_above_2_pow_24(G):
    """The id travels through LDS in a float word and must come back bit for bit: ids above 2^24 (not exactly representable
    as float VALUES, odd ones included) and ids whose bits are a denormal (below 2^23). The Gaussian array is padded to just
    over 2^24 rows; the eleven rows in the list are spread over it, the oracle evaluates the same eleven rows compactly."""
    sc = Scene(seed=9)
    for _ in range(11):
        sc.contributor()
    t = sc.tensors(3)
    n_rows = (1 << 24) + 16
    ids = torch.tensor([0, 3, (1 << 23) - 1, 1 << 23, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 3, (1 << 24) + 6,
                        (1 << 24) + 11, (1 << 24) + 15], dtype=torch.int64)
    got, ref = _gpu(G, t, ids=ids, n_rows=n_rows), _oracle(t)
    _in_band(got, ref, "ids above 2^24", rows=ids.to(DEV))
    for key in KEYS:  # and nothing was added anywhere else
        assert int((got[key] != 0).sum()) == int((got[key][ids.to(DEV)] != 0).sum()), key
