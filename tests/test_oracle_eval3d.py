"""CPU: oracle/eval3d.py (from-world compositing of 3DGUT) against the golden vectors of the reference's own torch
implementation (oracle/pin_eval3d_against_reference.py -> tests/golden/eval3d_ref.npz): images, last sample ids and the
gradients of all five inputs; and the widened statement (`from_world`: hit distance, normals, sample counts, gradients of the
rays and the backgrounds) against oracle/pin_eval3d_extras_against_reference.py -> tests/golden/eval3d_extras_ref.npz. The
per-element float64 use of the same statement is tests/_world_cases.py."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "eval3d_ref.npz")))


@pytest.mark.parametrize("name", ["a", "b"])
def test_eval3d_oracle_matches_reference(gold, name):
    from oracle import eval3d as E

    N, C, W, H, ts = (int(v) for v in gold[f"{name}.shape"])
    t = lambda k: torch.from_numpy(gold[f"{name}.{k}"])  # noqa: E731
    leaves = {k: t(k).clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "colors")}
    bg = t("backgrounds") if f"{name}.backgrounds" in gold else None
    ren, alp, last = E.rasterize_to_pixels_eval3d(leaves["means"], leaves["quats"], leaves["scales"], leaves["colors"],
                                                  leaves["opacities"], t("rays"), W, H, ts, t("isect_offsets"),
                                                  t("flatten_ids"), backgrounds=bg)
    assert ren.shape == (C, H, W, 3) and alp.shape == (C, H, W, 1) and last.dtype == torch.int32
    torch.testing.assert_close(ren, t("ref.render"), rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(alp, t("ref.alpha"), rtol=1e-5, atol=2e-5)
    assert float((last == t("ref.last_ids")).float().mean()) > 0.999
    ((ren * t("v_render")).sum() + (alp * t("v_alpha")).sum()).backward()
    for k, leaf in leaves.items():
        ref = t(f"ref.v_{k}")
        assert float((leaf.grad - ref).abs().max()) <= 2e-4 * float(ref.abs().max()), k


def _replay(gold, name, dtype=torch.float32):
    from oracle import eval3d as E

    sh = [int(v) for v in gold[f"{name}.shape"]]
    (N, C, W, H, ts), D = sh[:5], (sh[5] if len(sh) > 5 else 3)
    hit, nrm = (bool(sh[6]), bool(sh[7])) if len(sh) > 5 else (False, False)
    t = lambda k: torch.from_numpy(gold[f"{name}.{k}"])  # noqa: E731
    f = lambda k: t(k).to(dtype)  # noqa: E731
    leaves = {k: f(k).clone().requires_grad_(True) for k in ("means", "quats", "scales", "opacities", "colors", "rays")}
    if f"{name}.backgrounds" in gold:
        leaves["backgrounds"] = f("backgrounds").clone().requires_grad_(True)
    r = E.from_world(leaves["means"], leaves["quats"], leaves["scales"], leaves["colors"], leaves["opacities"], leaves["rays"], W, H,
                     ts, t("isect_offsets"), t("flatten_ids"), backgrounds=leaves.get("backgrounds"), use_hit_distance=hit,
                     return_normals=nrm)
    assert r.renders.shape == (C, H, W, D) and r.renders.dtype == dtype and (r.normals is not None) == nrm
    loss = (r.renders * f("v_render")).sum() + (r.alphas * f("v_alpha")).sum()
    if nrm:
        loss = loss + (r.normals * f("v_normals")).sum()
    loss.backward()
    return r, leaves, t


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", ["a", "b", "hit", "normals", "both"])
def test_widened_statement_reproduces_the_fixtures(gold, name, dtype):
    """`from_world` in float32 (the kernel's contract) and in float64 (the per-element reference of tests/_world_cases.py) on
    both golden files: images, normals, last ids, sample counts and the gradients of every input, rays and backgrounds included.
    The fixtures are the reference's float32 results: 2e-5 absolute on the images (hit distances reach ~8), 2e-4 of the largest
    element on the gradients, as the existing test above."""
    g = gold if name in ("a", "b") else dict(np.load(os.path.join(ROOT, "tests", "golden", "eval3d_extras_ref.npz")))
    r, leaves, t = _replay(g, name, dtype)
    torch.testing.assert_close(r.renders.float(), t("ref.render"), rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(r.alphas.float(), t("ref.alpha"), rtol=1e-5, atol=2e-5)
    assert float((r.last_ids == t("ref.last_ids")).float().mean()) > 0.999
    assert bool(((r.sample_counts > 0) == (r.last_ids >= 0)).all())
    if f"{name}.ref.sample_counts" in g:
        assert float((r.sample_counts == t("ref.sample_counts")).float().mean()) > 0.999
    if r.normals is not None:
        torch.testing.assert_close(r.normals.float(), t("ref.normals"), rtol=1e-5, atol=2e-5)
    for k, leaf in leaves.items():
        if f"{name}.ref.v_{k}" in g:
            ref = t(f"ref.v_{k}")
            assert float((leaf.grad.float() - ref).abs().max()) <= 2e-4 * float(ref.abs().max()), k


def test_widened_statement_masks_zero_rays_and_batches(gold):
    """What no fixture holds, as properties of the statement: a masked tile shows its background (or 0), alpha 0, no sample;
    a zero ray likewise; two batches of Gaussians are the two single-batch renders; detail=True returns the intermediates."""
    from oracle import eval3d as E

    t = lambda k: torch.from_numpy(gold[f"a.{k}"])  # noqa: E731
    N, C, W, H, ts = (int(v) for v in gold["a.shape"])
    masks = torch.ones(t("isect_offsets").shape, dtype=torch.bool)
    masks[0, 0, 1] = masks[1, 1, 2] = False
    rays = t("rays").clone()
    rays[0, 20, 5, 3:] = 0.0
    args = (t("colors"), t("opacities"), rays, W, H, ts, t("isect_offsets"), t("flatten_ids"))
    r = E.from_world(t("means"), t("quats"), t("scales"), *args, backgrounds=t("backgrounds"), masks=masks, detail=True)
    off = r.renders[0, :ts, ts:2 * ts]
    assert torch.equal(off, t("backgrounds")[0].expand_as(off)) and float(r.alphas[0, :ts, ts:2 * ts].abs().max()) == 0.0
    assert bool((r.last_ids[0, :ts, ts:2 * ts] == -1).all()) and int(r.sample_counts[1, ts:, 2 * ts:].sum()) == 0
    assert torch.equal(r.renders[0, 20, 5], t("backgrounds")[0]) and int(r.last_ids[0, 20, 5]) == -1
    assert int(r.sample_counts[0, 20, 6]) > 0
    assert r.alpha.shape == r.rows.shape and r.M.shape == r.rows.shape + (3, 3) and bool((r.keep <= r.walked).all())
    r0 = E.from_world(t("means"), t("quats"), t("scales"), *args, masks=masks)
    assert float(r0.renders[0, :ts, ts:2 * ts].abs().max()) == 0.0
    # B = 2 batches with C = 1 camera each: image 1 sees the second batch
    m2 = torch.stack([t("means"), t("means") + 0.05])
    rb = E.from_world(m2, t("quats").expand(2, -1, -1), t("scales").expand(2, -1, -1), *args)
    r1 = E.from_world(m2[1], t("quats"), t("scales"), *args)
    r00 = E.from_world(m2[0], t("quats"), t("scales"), *args)
    assert torch.equal(rb.renders[1], r1.renders[1]) and torch.equal(rb.renders[0], r00.renders[0])
    assert not torch.equal(rb.renders[1], r00.renders[1])


def test_pinhole_rays_are_unit_and_hit_the_pixel_centres(gold):
    from oracle import eval3d as E

    N, C, W, H, ts = (int(v) for v in gold["a.shape"])
    viewmats, Ks = torch.from_numpy(gold["a.viewmats"]), torch.from_numpy(gold["a.Ks"])
    rays = E.pinhole_rays(viewmats, Ks, W, H)
    torch.testing.assert_close(rays, torch.from_numpy(gold["a.rays"]))
    torch.testing.assert_close(rays[..., 3:].norm(dim=-1), torch.ones(C, H, W), rtol=0, atol=1e-6)
    # a point one unit along the ray of pixel (x, y) projects back to (x + 0.5, y + 0.5)
    p = rays[..., :3] + rays[..., 3:]
    pc = torch.einsum("cij,chwj->chwi", viewmats[:, :3, :3], p) + viewmats[:, None, None, :3, 3]
    u = pc[..., 0] / pc[..., 2] * Ks[:, 0, 0, None, None] + Ks[:, 0, 2, None, None]
    v = pc[..., 1] / pc[..., 2] * Ks[:, 1, 1, None, None] + Ks[:, 1, 2, None, None]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    assert float((u - (xs + 0.5)).abs().max()) < 1e-3 and float((v - (ys + 0.5)).abs().max()) < 1e-3
