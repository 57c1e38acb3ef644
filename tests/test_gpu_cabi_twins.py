"""GPU: C-ABI entry points that share one host body give the same bits for what they have in common.

Each pair below is one kernel behind two (or three) spellings of the entry point; the wider spelling adds an output or fills the
gradient rows itself. Both are called through _cabi.call on the same inputs, outputs NaN-filled first unless the entry's
contract asks for zero-filled ones, and the common outputs must be torch.equal. That is derivable, not hoped for: same kernel,
same arguments, and every route taken here is free of order-dependent float atomics -

  * no pose gradient (v_viewmats NULL);
  * packed rows of B C = 2 images go Gaussian-major through a row map (every output written once); a single image takes the
    row-major route whose stores are plain (EWA: the UNIQUE instantiation) or one atomic add per Gaussian onto a zero (2DGS);
  * compositing: a gradient row receives ONE atomic add per workgroup that holds the Gaussian, onto a zero-filled row. With at
    most two such workgroups the row is 0 + a + b in either order, and IEEE addition is commutative: 3DGS (3 channels, 16 x 16
    tiles, no absgrad: one wave per tile) renders 32 x 16 pixels = two tiles; 2DGS (one wave per HALF tile) renders 16 x 16 = one
    tile, and gets no median cotangent (that one is added once per pixel).

The extra output of the _opac entries is the float32 sum of <= n terms (n = C views, or the <= B C rows of a Gaussian), held to
n * eps_f32 * sum|terms| of the float64 sum. Shapes: N = 257 (one full 256-thread block and one thread), C = 2, about half of
the visible pairs as packed rows.
"""
import math

import pytest
import torch

from _util import make_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, C, TS = 257, 2, 16
EPS = torch.finfo(torch.float32).eps


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.skip("needs a ROCm GPU")
    import gsplat_amd

    return gsplat_amd


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g).to(DEV)


def _call(name, *args):
    from gsplat_amd import _cabi

    _cabi.call(name, *args)


def _assert_sum(got, terms, dim, n, name):
    """`got` = float32 sum of the <= n `terms` along `dim`."""
    want = terms.double().sum(dim)
    bound = n * EPS * terms.double().abs().sum(dim)
    assert bool(((got.double() - want).abs() <= bound).all()), name


@pytest.fixture(scope="module")
def ewa(G):
    """A projected 3DGS scene with cotangents, dense [C, N] and as packed rows (about half of the visible pairs)."""
    W, H = 64, 48
    sc, W, H = make_scene(N=N, C=C, width=W, height=H, seed=11)
    s = {k: v.to(DEV) for k, v in sc.items()}
    radii, _, _, conics, _ = G.fully_fused_projection(s["means"], None, s["quats"], s["scales"], s["viewmats"], s["Ks"], W, H)
    g = torch.Generator().manual_seed(12)
    s.update(W=W, H=H, radii=radii.contiguous(), conics=conics.contiguous(), v_means2d=_rand(g, C, N, 2), v_depths=_rand(g, C, N),
             v_conics=_rand(g, C, N, 3), v_view=_rand(g, C, N))
    visible = (radii > 0).all(-1)
    assert C * N // 4 < int(visible.sum()) < C * N  # both kinds of pair are present
    s["keep"] = visible & (torch.rand(C, N, generator=g).to(DEV) < 0.5)
    return s


def _packed(s, cams):
    """Rows of the kept pairs of the first `cams` cameras, image-major: ids and the per-row slices of the dense tensors."""
    keep = s["keep"][:cams]
    cam, gid = keep.nonzero(as_tuple=True)
    rows = {k: s[k][:cams][keep].contiguous() for k in ("conics", "v_means2d", "v_depths", "v_conics", "v_view")}
    assert 0 < gid.numel() < cams * N
    return torch.zeros_like(cam), cam.contiguous(), gid.contiguous(), rows


def _ewa_head(s, cams):
    return (s["means"], None, s["quats"], s["scales"], s["viewmats"][:cams].contiguous(), s["Ks"][:cams].contiguous(), 1, cams, N,
            s["W"], s["H"], 0.3, 0)


def test_project_ewa_bwd_and_opac(G, ewa):
    s = ewa
    head = _ewa_head(s, C) + (s["radii"], s["conics"], None, s["v_means2d"], 2, s["v_depths"], s["v_conics"], 3, None)
    a = [_nan(N, 3), _nan(N, 4), _nan(N, 3)]
    b = [_nan(N, 3), _nan(N, 4), _nan(N, 3)]
    v_op = _nan(N)
    _call("gsx_project_ewa_bwd", *head, a[0], None, a[1], a[2], None)
    _call("gsx_project_ewa_bwd_opac", *head, s["v_view"], 1, b[0], None, b[1], b[2], None, v_op)
    for x, y, nm in zip(a, b, ("v_means", "v_quats", "v_scales")):
        assert torch.isfinite(x).all() and torch.equal(x, y), nm
    assert float(a[0].abs().max()) > 0
    _assert_sum(v_op, s["v_view"], 0, C, "v_opacities")


@pytest.mark.parametrize("cams", [2, 1], ids=["row-map", "single-image"])
def test_project_ewa_packed_bwd_and_opac(G, ewa, cams):
    s = ewa
    bid, cid, gid, r = _packed(s, cams)
    nnz = gid.numel()
    row_map = None
    fill = torch.zeros  # row-major route: into zero-filled outputs
    if cams > 1:
        row_map = torch.empty(cams * N, device=DEV, dtype=torch.int32)
        _call("gsx_packed_row_map", bid, cid, gid, nnz, 1, cams, N, row_map)
        fill = lambda *shape, device: _nan(*shape)  # noqa: E731  Gaussian-major: every output row written once
    head = _ewa_head(s, cams) + (nnz, bid, cid, gid, r["conics"], None, r["v_means2d"], 2, r["v_depths"], r["v_conics"], 3, None)
    a = [fill(N, w, device=DEV) for w in (3, 4, 3)]
    b = [fill(N, w, device=DEV) for w in (3, 4, 3)]
    v_op = fill(N, 1, device=DEV).reshape(N)
    _call("gsx_project_ewa_packed_bwd", *head, row_map, a[0], None, a[1], a[2], None)
    _call("gsx_project_ewa_packed_bwd_opac", *head, r["v_view"], 1, row_map, b[0], None, b[1], b[2], None, v_op)
    for x, y, nm in zip(a, b, ("v_means", "v_quats", "v_scales")):
        assert torch.isfinite(x).all() and torch.equal(x, y), nm
    assert float(a[0].abs().max()) > 0
    terms = torch.zeros(cams, N, device=DEV)
    terms[cid, gid] = r["v_view"]  # a Gaussian has at most one row per image
    _assert_sum(v_op, terms, 0, cams, "v_opacities")
    without_rows = ~s["keep"][:cams].any(0)
    assert bool(without_rows.any()) and bool((v_op[without_rows] == 0).all())


def test_project_ewa_opac_without_views_or_rows_is_zero(G, ewa):
    """The branches no CPU test can reach: no views (dense) / no rows (packed) -> v_opacities is set to +0, nothing else is read."""
    s = ewa
    v_op = _nan(N)
    _call("gsx_project_ewa_bwd_opac", *_ewa_head(s, C)[:7], 0, N, s["W"], s["H"], 0.3, 0, *([None] * 4), 2, None, None, 3, None,
          None, 1, *([None] * 5), v_op)
    assert torch.equal(v_op, torch.zeros(N, device=DEV)) and not bool(torch.signbit(v_op).any())
    v_op = _nan(N)
    _call("gsx_project_ewa_packed_bwd_opac", *_ewa_head(s, C), 0, *([None] * 6), 2, None, None, 3, None, None, 1, *([None] * 6), v_op)
    assert torch.equal(v_op, torch.zeros(N, device=DEV)) and not bool(torch.signbit(v_op).any())


@pytest.fixture(scope="module")
def surfels(G):
    W, H = 64, 48
    sc, W, H = make_scene(N=N, C=C, width=W, height=H, seed=13)
    s = {k: v.to(DEV) for k, v in sc.items()}
    radii, _, _, M, _ = G.fully_fused_projection_2dgs(s["means"], s["quats"], s["scales"], s["viewmats"], s["Ks"], W, H)
    g = torch.Generator().manual_seed(14)
    s.update(radii=radii.contiguous(), M=M.reshape(C, N, 9).contiguous(), v_means2d=_rand(g, C, N, 2), v_depths=_rand(g, C, N),
             v_M=_rand(g, C, N, 9), v_normals=_rand(g, C, N, 3), v_view=_rand(g, C, N))
    visible = (radii > 0).all(-1)
    assert C * N // 4 < int(visible.sum()) < C * N
    s["keep"] = visible & (torch.rand(C, N, generator=g).to(DEV) < 0.5)
    return s


def test_project_2dgs_bwd_and_opac(G, surfels):
    s = surfels
    head = (s["means"], s["quats"], s["scales"], s["viewmats"], s["Ks"], 1, C, N, s["radii"], s["M"], s["v_means2d"], s["v_depths"],
            s["v_M"], s["v_normals"], 0, 0)
    a = [_nan(N, 3), _nan(N, 4), _nan(N, 3)]
    b = [_nan(N, 3), _nan(N, 4), _nan(N, 3)]
    v_op = _nan(N)
    _call("gsx_project_2dgs_bwd", *head, a[0], a[1], a[2], None)
    _call("gsx_project_2dgs_bwd_opac", *head, s["v_view"], 1, b[0], b[1], b[2], None, v_op)
    for x, y, nm in zip(a, b, ("v_means", "v_quats", "v_scales")):
        assert torch.isfinite(x).all() and torch.equal(x, y), nm
    assert float(a[0].abs().max()) > 0
    _assert_sum(v_op, s["v_view"], 0, C, "v_opacities")


def test_project_2dgs_packed_bwd_and_rows(G, surfels):
    """One image: a Gaussian has at most one row, so the dense gradient is 0 + its row (exact) and zero elsewhere."""
    s = surfels
    keep = s["keep"][:1]
    cid, gid = keep.nonzero(as_tuple=True)
    nnz = gid.numel()
    assert 0 < nnz < N
    r = {k: s[k][:1][keep].contiguous() for k in ("M", "v_means2d", "v_depths", "v_M", "v_normals")}
    head = (s["means"], s["quats"], s["scales"], s["viewmats"][:1].contiguous(), s["Ks"][:1].contiguous(), 1, 1, N, nnz,
            torch.zeros_like(cid), cid.contiguous(), gid.contiguous(), r["M"], r["v_means2d"], r["v_depths"], r["v_M"], r["v_normals"], 0)
    dense = [torch.zeros(N, w, device=DEV) for w in (3, 4, 3)]  # the contract: accumulated into zero-filled outputs
    rows = [_nan(nnz, w) for w in (3, 4, 3)]
    _call("gsx_project_2dgs_packed_bwd", *head, *dense, None)
    _call("gsx_project_2dgs_packed_bwd_rows", *head, *rows, None)
    for d, x, nm in zip(dense, rows, ("v_means", "v_quats", "v_scales")):
        assert torch.isfinite(x).all() and torch.equal(d[gid], x), nm
        rest = torch.ones(N, dtype=torch.bool, device=DEV)
        rest[gid] = False
        assert bool((d[rest] == 0).all()), nm
    assert float(rows[0].abs().max()) > 0


def _tiles(G, m2, radii, depths, W, H):
    tw, th = math.ceil(W / TS), math.ceil(H / TS)
    _, ids, fl = G.isect_tiles(m2, radii, depths, TS, tw, th)
    return tw, th, G.isect_offset_encode(ids, C, tw, th), fl


def test_raster3d_bwd_ws_fill(G):
    W, H, D = 32, 16, 3
    sc, W, H = make_scene(N=N, C=C, width=W, height=H, seed=15)
    s = {k: v.to(DEV) for k, v in sc.items()}
    radii, m2, depths, conics, _ = G.fully_fused_projection(s["means"], None, s["quats"], s["scales"], s["viewmats"], s["Ks"], W, H)
    op = s["opacities"][None].expand(C, -1).contiguous()
    tw, th, off, fl = _tiles(G, m2, radii, depths, W, H)
    assert (tw, th) == (2, 1) and fl.numel() > N // 2
    g = torch.Generator().manual_seed(16)
    colors = torch.rand(C, N, D, generator=g).to(DEV)
    _, ra, _, last = torch.ops.gsplat.rasterize_to_pixels_3dgs(m2, conics, colors, op, None, None, W, H, TS, off, fl, False, False)
    v_rc, v_ra = _rand(g, C, H, W, D), _rand(g, C, H, W, 1)
    R, stride = C * N, 6 + D
    head = (m2, conics, colors, op, None, None, off, fl, ra, last, v_rc, v_ra, C, fl.numel(), D, W, H, TS, tw, th, 0)
    from gsplat_amd import _cabi

    ws = torch.empty(_cabi._lib.gsx_raster3d_bwd_workspace_bytes(C, tw, th), device=DEV, dtype=torch.uint8)
    plain, with_ws, filled = torch.zeros(R, stride, device=DEV), torch.zeros(R, stride, device=DEV), _nan(R, stride)
    _call("gsx_raster3d_bwd", *head, plain, stride)
    _call("gsx_raster3d_bwd_ws", *head, with_ws, stride, -1, 1, ws, ws.numel())
    _call("gsx_raster3d_bwd_fill", *head, filled, stride, R, -1, 1, ws, ws.numel())
    assert torch.isfinite(plain).all() and float(plain.abs().max()) > 0
    assert torch.equal(plain, with_ws), "gsx_raster3d_bwd_ws"
    assert torch.equal(plain, filled), "gsx_raster3d_bwd_fill"
    assert bool((plain[fl.unique().long()] != 0).any()) and bool((plain == 0).all(-1).any())  # touched rows, and rows only the fill wrote


def test_raster2d_bwd_ws_fill(G):
    W, H, D = 16, 16, 3
    sc, W, H = make_scene(N=N, C=C, width=W, height=H, seed=17)
    s = {k: v.to(DEV) for k, v in sc.items()}
    radii, m2, depths, M, nrm = G.fully_fused_projection_2dgs(s["means"], s["quats"], s["scales"], s["viewmats"], s["Ks"], W, H)
    op = s["opacities"][None].expand(C, -1).contiguous()
    tw, th, off, fl = _tiles(G, m2, radii, depths, W, H)
    assert (tw, th) == (1, 1) and fl.numel() > N // 2
    g = torch.Generator().manual_seed(18)
    colors = torch.rand(C, N, D, generator=g).to(DEV)
    fwd = torch.ops.gsplat.rasterize_to_pixels_2dgs(m2, M, colors, op, nrm, torch.zeros_like(m2), None, None, W, H, TS, off, fl, False,
                                                    False, False)
    rc, ra, _, _, _, _, last, median = fwd
    v_rc, v_ra, v_rn = _rand(g, C, H, W, D), _rand(g, C, H, W, 1), _rand(g, C, H, W, 3)
    R, stride = C * N, 17 + D
    head = (m2, M.contiguous(), colors, op, nrm, None, None, off, fl, rc, ra, last, median, v_rc, v_ra, v_rn, None, None, C, fl.numel(),
            D, W, H, TS, tw, th, 0)
    from gsplat_amd import _cabi

    ws = torch.empty(_cabi._lib.gsx_raster3d_bwd_workspace_bytes(C, tw, th), device=DEV, dtype=torch.uint8)
    plain, with_ws, filled = torch.zeros(R, stride, device=DEV), torch.zeros(R, stride, device=DEV), _nan(R, stride)
    _call("gsx_raster2d_bwd", *head, plain, stride)
    _call("gsx_raster2d_bwd_ws", *head, with_ws, stride, ws, ws.numel())
    _call("gsx_raster2d_bwd_fill", *head, filled, stride, R, ws, ws.numel())
    assert torch.isfinite(plain).all() and float(plain.abs().max()) > 0
    assert torch.equal(plain, with_ws), "gsx_raster2d_bwd_ws"
    assert torch.equal(plain, filled), "gsx_raster2d_bwd_fill"
    assert bool((plain == 0).all(-1).any())  # rows only the fill wrote
