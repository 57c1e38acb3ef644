"""Shared by tests/test_kmeans.py and tests/test_gpu_kmeans.py: seeded inputs for the L1 K-means kernels (csrc/kmeans.hip), the
sequential float32 composition that DEFINES their result, and a float64 brute force. Every generator runs on the CPU."""
import torch

# the smallest shapes that reach every edge of the assignment kernel (64 rows per workgroup, centroid tiles of 64, four
# coordinates per LDS read): below one row tile and no multiple of it; one centroid, a tile boundary, many tiles; odd D, D not a
# multiple of 4, the cap
NS = (1, 63, 257, 1000)
KS = (1, 2, 65, 1031, 4099)
DS = (1, 9, 45, 72, 128)
ASSIGN_CASES = [(n, k, d) for d in DS for k in KS for n in NS]

U = 2.0 ** -24  # unit roundoff of float32


def assign_case(n, k, d):
    """(x [n, d], centroids [k, d]), standard normal, float32, seeded by the shape."""
    g = torch.Generator().manual_seed(1_000_003 * n + 1_009 * k + d)
    return torch.randn(n, d, generator=g), torch.randn(k, d, generator=g)


def lowest_argmin(dist):
    """(min over dim 1, the LOWEST index that attains it)."""
    best = dist.min(dim=1).values
    cols = torch.arange(dist.shape[1], device=dist.device).expand_as(dist)
    return best, torch.where(dist == best[:, None], cols, torch.full_like(cols, dist.shape[1])).min(dim=1).values


def sequential_f32(x, c):
    """The definition: one float32 accumulator per pair, acc = acc + |x[i, d] - c[j, d]| for ascending d, then the lowest-index
    argmin. Returns (labels int64 [N], best float32 [N]); runs on x's device."""
    assert x.dtype == torch.float32 and c.dtype == torch.float32
    acc = torch.zeros((x.shape[0], c.shape[0]), dtype=torch.float32, device=x.device)
    for d in range(x.shape[1]):
        acc = acc + (x[:, d, None] - c[None, :, d]).abs()
    best, labels = lowest_argmin(acc)
    return labels, best


def distances_f64(x, c):
    """[N, K] float64 L1 distances of the float32 inputs (accumulated per coordinate: no [N, K, D] tensor)."""
    x, c = x.double(), c.double()
    acc = torch.zeros((x.shape[0], c.shape[0]), dtype=torch.float64, device=x.device)
    for d in range(x.shape[1]):
        acc += (x[:, d, None] - c[None, :, d]).abs()
    return acc


def excess_over_f64_minimum(x, c, labels):
    """(float64 distance of the chosen centroid - float64 minimum, float64 distance of the chosen centroid), per row."""
    d64 = distances_f64(x, c)
    chosen = d64.gather(1, labels[:, None])[:, 0]
    return chosen - d64.min(dim=1).values, chosen


def tolerance(d, chosen):
    """2 (D + 1) 2^-24 dist. A computed distance is the exact one times (1 + t), |t| <= (D + 1) u to first order: D once-rounded
    differences summed by D - 1 rounded additions in any order. A centroid c preferred over the true minimiser m has
    fl(dist_c) <= fl(dist_m), so dist_c (1 - e) <= dist_m (1 + e) with e = (D + 1) u, i.e. dist_c - dist_m <= e (dist_c + dist_m)
    <= 2 e dist_c: `dist` is the float64 distance of the chosen centroid."""
    return 2.0 * (d + 1) * U * chosen


def blobs(n=4096, d=45, n_blobs=32, n_clusters=48, sigma=0.05, seed=3, init_seed=1):
    """The separated-blob construction of tests/test_compression.py (centres 10 randn, rows = centre + sigma randn), with one
    addition that turns "pure clusters" from luck into a theorem: the rows kmeans_l1 draws as initial centroids with `init_seed`
    (the first `n_clusters` entries of a seeded CPU randperm) are dealt to the blobs round robin, so every blob starts with a
    centroid of its own. The blobs lie ~ 10 sqrt(2 d) apart and are sigma wide, so from the first assignment on every row goes to
    a centroid inside its blob, every cluster is pure, and stays so. Returns (x, blob of each row, centres)."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(n_blobs, d, generator=g) * 10
    blob = torch.randint(0, n_blobs, (n,), generator=g)
    first = torch.randperm(n, generator=torch.Generator().manual_seed(init_seed))[:n_clusters]
    blob[first] = torch.arange(n_clusters) % n_blobs
    x = centres[blob] + sigma * torch.randn(n, d, generator=g)
    return x, blob, centres
