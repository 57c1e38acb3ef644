"""GPU: the L1 K-means kernels (csrc/kmeans.hip) behind gsplat_amd.compression.kmeans_l1 / kmeans_assign_l1 / _KMeans.

The assignment is DEFINED as one float32 accumulator per (row, centroid) pair, ascending d, lowest index among the minima, so
labels and distances are compared bit for bit with that composition evaluated in torch on the same device
(tests/_kmeans_cases.py sequential_f32). The update adds in a fixed order of its own, so its means are held to the float64
mean: an any-order float32 sum of n values is within (n - 1) u sum|x_i| of the exact one and the division adds u |mean|, i.e.
the mean is within n u mean_i|x_i| with u = 2^-24 and the mean of |x| taken per entry over the cluster's rows. Every test asserts
the fused predicate first, so none can pass through the torch path."""
import numpy as np
import pytest
import torch

import _kmeans_cases as kc
from gsplat_amd.compression import png_compression as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def assign(x, c):
    assert C._kmeans_fused_ok(x) and C._kmeans_fused_ok(c), "the fused kernels were not taken"
    labels, best = C.kmeans_assign_l1(x, c, return_distance=True)
    assert labels.dtype == torch.int64 and best.dtype == torch.float32 and labels.shape == best.shape == (x.shape[0],)
    return labels, best


@pytest.mark.parametrize("n,k,d", kc.ASSIGN_CASES)
def test_assign_is_the_sequential_composition_bit_for_bit(n, k, d):
    x, c = (t.to(DEV) for t in kc.assign_case(n, k, d))
    labels, best = assign(x, c)
    ref_labels, ref_best = kc.sequential_f32(x, c)
    assert torch.equal(best, ref_best), f"{int((best != ref_best).sum())} distances differ"
    assert torch.equal(labels, ref_labels), f"{int((labels != ref_labels).sum())} labels differ"
    assert torch.equal(C.kmeans_assign_l1(x, c), labels)  # without the distances: the same labels
    if d == 45:  # against float64
        excess, chosen = kc.excess_over_f64_minimum(x, c, labels)
        tol = kc.tolerance(d, chosen)
        print(f"largest excess over the float64 minimum: {float((excess / tol.clamp_min(1e-300)).max()):.3f} of the tolerance")
        assert bool((excess <= tol).all())


def test_assign_no_rows():
    x, c = torch.zeros(0, 45, device=DEV), torch.randn(5, 45, device=DEV)
    labels, best = assign(x, c)
    assert labels.numel() == 0 and best.numel() == 0


@pytest.mark.parametrize("d", [9, 45])
def test_ties_go_to_the_lowest_index(d):
    x, c = (t.to(DEV) for t in kc.assign_case(257, 65, d))
    twice = torch.cat([c, c])
    labels, best = assign(x, twice)
    assert bool((labels < 65).all()) and torch.equal(labels, assign(x, c)[0]) and torch.equal(best, assign(x, c)[1])
    same = c[:1].expand(300, d).contiguous()
    labels, _ = assign(x, same)
    assert bool((labels == 0).all())
    pick = torch.arange(65, device=DEV).repeat(3)  # rows that ARE centroid rows
    labels, best = assign(twice[pick + 65].contiguous(), twice)
    assert bool((best == 0).all()) and torch.equal(labels, pick)


def test_non_finite_rows_get_a_label_in_range_and_disturb_nobody():
    x, c = (t.to(DEV) for t in kc.assign_case(257, 65, 45))
    clean, clean_best = assign(x, c)
    y = x.clone()
    y[70, 44], y[200, 0] = float("nan"), float("inf")
    labels, best = assign(y, c)
    assert bool(((labels >= 0) & (labels < 65)).all())
    keep = torch.ones(257, dtype=torch.bool, device=DEV)
    keep[[70, 200]] = False
    assert torch.equal(labels[keep], clean[keep]) and torch.equal(best[keep], clean_best[keep])
    # all centroids non-finite: still in range
    bad = c.clone()
    bad[:, 3] = float("nan")
    labels, _ = assign(x, bad)
    assert bool(((labels >= 0) & (labels < 65)).all())


def _update_labels(kind, x, c):
    n, k = x.shape[0], c.shape[0]
    if kind == "assigned":
        return assign(x, c)[0]
    if kind == "one cluster":
        return torch.zeros(n, dtype=torch.int64, device=DEV)
    g = torch.Generator().manual_seed(17)  # two thirds of the clusters empty, cluster 3 large, the last cluster used
    lab = torch.randint(0, k // 3, (n,), generator=g) * 3
    lab[1000:2500] = 3
    lab[-1] = k - 1
    return lab.to(DEV)


@pytest.mark.parametrize("kind", ["assigned", "one cluster", "empty clusters"])
@pytest.mark.parametrize("d", [9, 45])
def test_update(d, kind):
    n, k = 4099, 257
    g = torch.Generator().manual_seed(100 + d)
    x = torch.randn(n, d, generator=g).to(DEV)
    c = x[torch.randperm(n, generator=g)[:k].to(DEV)].clone()
    assert C._kmeans_fused_ok(x) and C._kmeans_fused_ok(c)
    labels = _update_labels(kind, x, c)
    new, counts, shift = C._update_fused(x, labels.to(torch.int32), c)
    ref_counts = torch.bincount(labels, minlength=k)
    assert counts.dtype == torch.int32 and torch.equal(counts.to(torch.int64), ref_counts)
    empty = ref_counts == 0
    assert kind != "empty clusters" or int(empty.sum()) > k // 2
    assert kind != "one cluster" or int(empty.sum()) == k - 1
    assert torch.equal(new[empty], c[empty])
    sums = torch.zeros(k, d, dtype=torch.float64, device=DEV).index_add_(0, labels, x.double())
    sums_abs = torch.zeros(k, d, dtype=torch.float64, device=DEV).index_add_(0, labels, x.double().abs())
    nk = ref_counts.clamp_min(1).double()[:, None]
    err = (new.double() - sums / nk).abs()[~empty]
    tol = (nk * kc.U * (sums_abs / nk))[~empty]
    print(f"largest mean error: {float((err / tol.clamp_min(1e-300)).max()):.3f} of the tolerance")
    assert bool((err <= tol).all())
    assert shift.shape == (1,) and torch.equal(shift[0], (new - c).abs().max())
    again = C._update_fused(x, labels.to(torch.int32), c)
    assert torch.equal(again[0], new) and torch.equal(again[1], counts) and torch.equal(again[2], shift)


def test_kmeans_l1_recovers_separated_blobs_and_repeats_bit_for_bit():
    sigma = 0.05
    x, blob, centres = kc.blobs(n=4096, d=45, n_blobs=32, n_clusters=48, sigma=sigma, seed=3, init_seed=1)
    x, blob, centres = x.to(DEV), blob.to(DEV), centres.to(DEV)
    assert C._kmeans_fused_ok(x)
    cents, lab = C.kmeans_l1(x, 48, n_iters=25, seed=1)
    assert cents.shape == (48, 45) and lab.shape == (4096,) and lab.dtype == torch.int64
    assert bool(((lab >= 0) & (lab < 48)).all())
    for k in range(48):
        # the mean of n >= 1 rows of one blob (an emptied cluster keeps such a mean): the mean absolute deviation from the blob's
        # centre per coordinate is ~ 0.8 sigma / sqrt(n), below sigma
        dev = (cents[k][None] - centres).abs().mean(dim=1)
        home = int(dev.argmin())
        assert float(dev[home]) <= sigma, f"centroid {k}: {float(dev[home]):.4f}"
        # a centroid of its own in every blob at the start and blobs far apart: no cluster is ever mixed (kc.blobs)
        assert bool((blob[lab == k] == home).all()), f"cluster {k}"
    assert torch.equal(C.kmeans_assign_l1(x, cents), lab)  # the labels are those of the returned centroids
    cents2, lab2 = C.kmeans_l1(x, 48, n_iters=25, seed=1)
    assert torch.equal(cents, cents2) and torch.equal(lab, lab2)


def test_codec_round_trip_on_the_gpu(tmp_path):
    g = torch.Generator().manual_seed(23)
    shN = torch.randn(1024, 15, 3, generator=g).to(DEV)
    assert C._kmeans_fused_ok(shN.reshape(1024, -1))
    meta = C._KMeans.compress(str(tmp_path), "shN", shN, n_clusters=64, verbose=False)
    back = C._KMeans.decompress(str(tmp_path), "shN", meta)
    blob = np.load(str(tmp_path / "shN.npz"))
    assert blob["labels"].dtype == np.uint16 and blob["labels"].shape == (1024,) and int(blob["labels"].max()) < 64
    assert blob["centroids"].shape == (64, 45) and int(blob["centroids"].max()) <= 63
    cents = torch.from_numpy(blob["centroids"] / 63)
    mins, maxs = torch.tensor(meta["mins"]), torch.tensor(meta["maxs"])
    expect = (cents * (maxs - mins) + mins)[torch.from_numpy(blob["labels"].astype(np.int64))].reshape(1024, 15, 3).float()
    assert back.shape == shN.shape and torch.equal(back, expect)
