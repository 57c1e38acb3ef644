// gsplat_amd — exact k-nearest-neighbour search over a point cloud (gsx_knn_bin / gsx_knn_search), the kernel behind
// gsplat_amd.init_utils.knn / knn_scale_init (the reference: gsplat/init_utils.py:145 knn_scale_init, a chunked cdist + topk,
// and examples/utils.py:156 knn, scikit-learn on the host).
//
// Algorithm (all float32, one uniform grid, nothing read back by the host):
//   gsx_knn_bin     1. knn_bbox_kernel    256 workgroups: min / max / sum / sum of squares (double) / count of the FINITE points
//                   2. knn_grid_kernel    one lane: box = bounding box intersected with mean +- 3 sigma per axis (a handful of far
//                                         outliers must not decide the cell size; points outside the box fall into the border
//                                         cells), grid dims with at most M = M(N) cells, M a power of two near N / 2
//                   3. knn_keys_kernel    key[i] = cell(i) << 32 | i; a non-finite point gets the cell kNoCell (sorts last)
//   (the caller sorts the keys; they are distinct, so any correct sort gives the same order)
//   gsx_knn_search  4. knn_gather_kernel  sorted[j] = (x, y, z, index) of the j-th key; cell_start[c] = lower bound of c << 32
//                                         among the sorted keys, a binary search of 32 fixed steps, for every c in [0, M]
//                   5. knn_walk_kernel    one lane per query IN SORTED ORDER (the lanes of a wave sit in the same or adjacent
//                                         cells, so their loads coincide): cubic rings of cells outward, the K best squared
//                                         distances and indices in registers. A cell row along x is one contiguous range of
//                                         `sorted`. After ring r the query stops if its K-th best distance is no larger than
//                                         its distance to the nearest face of the (2r+1)^3 block that still has cells behind
//                                         it, or if no face has. A query still open after ring `ring_cap` is appended to the
//                                         deferred list (integer atomic on a counter in the workspace).
//                   6. knn_deferred_kernel  a fixed number of workgroups loops over the deferred list; one workgroup per
//                                         query scans all finite points, 256 best-lists merged pairwise through LDS.
//
// Exactness. d2 = (dx dx + dy dy) + dz dz from coordinate differences (unit built with -ffp-contract=off: the walk and the
// deferred scan give the same bits, and d2 is symmetric in its two points). The K smallest d2 of a row are a unique multiset,
// so the returned distances do not depend on the grid, on the sort, on which path served the row, or on the input order.
// The stop test is conservative: with t(p) = fl(fl(p - bmin) * scale) (monotone in p, the same expression that binned p), a
// point in a cell beyond the face m has t >= m (or < m on the low side), so its coordinate differs from the query's by at
// least (|m - t(q)| - 2^-22 (1024 + |t(q)|)) cells; the test subtracts 1e-3 + 1e-6 |t(q)| cells and shortens the cell by 1e-6.
//
// Termination, bounded by construction - no trip count is a data value:
//   - bbox: grid-stride over N. grid: loops over 256 partials, 3 axes, 4 passes. keys / gather: one element per lane.
//   - cell_start: exactly 32 halvings of [0, N]. Every entry is <= N by construction.
//   - walk: r runs over [0, ring_cap] (host argument, <= 1024); per ring (2r+1)^2 rows; per row one or two ranges
//     [cell_start[a], cell_start[b]) with both ends clamped to N, so at most N trips. Nothing waits on another lane.
//   - deferred: count = min(counter, N) (each query appends at most once); workgroup b takes entries b, b + G, ...: at most
//     N / G + 1 trips of N / 256 + 1 points, 8 merge steps of KP elements.
//   Non-finite points (any coordinate NaN or +-Inf) are left out of the box and carry kNoCell: they are in no cell range and
//   `n_finite = cell_start[M]` ends the deferred scan before them, so they are in nobody's neighbour set; their own rows are
//   NaN with index -1. A finite point whose distance overflows float32 is never closer than "no neighbour" (inf, index -1).
//   A degenerate box (zero or non-representable extent on an axis) gives that axis one cell; all axes degenerate = one cell,
//   which ring 0 scans completely and the "no face has cells behind it" rule closes.
#include "common.hpp"

#include <math.h>

namespace gsx {

constexpr int kKnnPartials        = 256;  // workgroups of the bounding-box pass
constexpr int kKnnPartialWidth    = 16;   // doubles per partial: min[3] max[3] sum[3] sumsq[3] count, padded
constexpr int kKnnAxisCap         = 1024; // cells per axis (keeps the rounding of t below the 1e-3 cell of the stop test)
constexpr uint32_t kKnnNoCell     = 0x7FFFFFFFu;
constexpr int kKnnDeferredBlocks  = 1024;
constexpr uint32_t kKnnMaxCells   = 1u << 24;
constexpr uint32_t kKnnMaxRingCap = 1024;

struct KnnHeader { // the first 64 bytes of the workspace
    float bmin[3], scale[3], h[3];
    int32_t dims[3];
    uint32_t n_deferred;
    uint32_t n_cells;
    uint32_t pad[2];
};
static_assert(sizeof(KnnHeader) == 64, "KnnHeader layout");

struct KnnLayout {
    uint32_t M; // cell_start has M + 1 entries
    size_t partials, cell_start, sorted, deferred, total;
};

static KnnLayout knn_layout(int64_t N)
{
    KnnLayout L;
    uint32_t M = 1;
    while ((int64_t)M * 4 <= N && M < kKnnMaxCells) M <<= 1; // the power of two in (N / 4, N / 2]
    L.M          = M;
    auto up      = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.partials   = 256;
    L.cell_start = L.partials + up((size_t)kKnnPartials * kKnnPartialWidth * sizeof(double));
    L.sorted     = L.cell_start + up(((size_t)M + 1) * sizeof(uint32_t));
    L.deferred   = L.sorted + up((size_t)N * sizeof(float4));
    L.total      = L.deferred + up((size_t)N * sizeof(uint32_t));
    return L;
}

__device__ __forceinline__ bool knn_finite3(float a, float b, float c)
{
    return fabsf(a) <= 3.402823466e38f && fabsf(b) <= 3.402823466e38f && fabsf(c) <= 3.402823466e38f; // false for NaN
}

__global__ void __launch_bounds__(256) knn_bbox_kernel(const float *__restrict__ x, uint32_t N, double *__restrict__ partials)
{
    __shared__ double s_red[256];
    double v[13];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        v[a]     = INFINITY;
        v[3 + a] = -INFINITY;
        v[6 + a] = 0.0;
        v[9 + a] = 0.0;
    }
    v[12] = 0.0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < N; i += (uint32_t)kKnnPartials * 256u) {
        const float p[3] = {x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2]};
        if (!knn_finite3(p[0], p[1], p[2])) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double d = (double)p[a];
            v[a]           = fmin(v[a], d);
            v[3 + a]       = fmax(v[3 + a], d);
            v[6 + a] += d;
            v[9 + a] += d * d;
        }
        v[12] += 1.0;
    }
    // 13 tree reductions in a fixed order (the work is negligible next to the search)
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        s_red[threadIdx.x] = v[k];
        __syncthreads();
        for (uint32_t s = 128; s >= 1; s >>= 1) {
            if (threadIdx.x < s) {
                const double a = s_red[threadIdx.x], b = s_red[threadIdx.x + s];
                s_red[threadIdx.x] = k < 3 ? fmin(a, b) : (k < 6 ? fmax(a, b) : a + b);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) partials[(size_t)blockIdx.x * kKnnPartialWidth + k] = s_red[0];
        __syncthreads();
    }
}

__global__ void knn_grid_kernel(const double *__restrict__ partials, uint32_t M, KnnHeader *__restrict__ hdr)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double v[13];
    for (int k = 0; k < 13; ++k) v[k] = k < 3 ? (double)INFINITY : (k < 6 ? -(double)INFINITY : 0.0);
    for (int b = 0; b < kKnnPartials; ++b)
        for (int k = 0; k < 13; ++k) {
            const double p = partials[(size_t)b * kKnnPartialWidth + k];
            v[k]           = k < 3 ? fmin(v[k], p) : (k < 6 ? fmax(v[k], p) : v[k] + p);
        }
    float lo[3] = {0.f, 0.f, 0.f}, e[3] = {0.f, 0.f, 0.f};
    bool active[3] = {false, false, false};
    if (v[12] > 0.0) {
        for (int a = 0; a < 3; ++a) {
            const double mean = v[6 + a] / v[12];
            const double sd   = sqrt(fmax(v[9 + a] / v[12] - mean * mean, 0.0));
            const float l     = (float)fmax(v[a], mean - 3.0 * sd);
            const float u     = (float)fmin(v[3 + a], mean + 3.0 * sd);
            lo[a]             = l;
            e[a]              = u - l;
            active[a]         = e[a] > 1e-30f && e[a] < 1e30f; // false for NaN too
        }
    }
    // cell edge hh such that the active extents hold M cells; an axis thinner than one cell leaves the count (4 passes: each
    // of the first three can retire an axis, the last one settles hh)
    double hh = 0.0;
    for (int pass = 0; pass < 4; ++pass) {
        int d      = 0;
        double vol = 1.0;
        for (int a = 0; a < 3; ++a)
            if (active[a]) {
                ++d;
                vol *= (double)e[a];
            }
        if (d == 0) break;
        hh = pow(vol / (double)M, 1.0 / (double)d);
        for (int a = 0; a < 3; ++a)
            if (active[a] && !((double)e[a] >= hh)) active[a] = false;
    }
    int32_t dims[3];
    uint64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        dims[a] = 1;
        if (active[a] && hh > 0.0) {
            const double q = floor((double)e[a] / hh);
            dims[a]        = q >= (double)kKnnAxisCap ? kKnnAxisCap : (q >= 1.0 ? (int32_t)q : 1);
        }
        cells *= (uint64_t)dims[a];
    }
    if (cells > (uint64_t)M) { // cannot happen (prod floor(e / hh) <= M); the table size must hold whatever happens
        dims[0] = dims[1] = dims[2] = 1;
        cells                      = 1;
    }
    for (int a = 0; a < 3; ++a) {
        const bool on = dims[a] > 1;
        hdr->bmin[a]  = lo[a];
        hdr->scale[a] = on ? (float)dims[a] / e[a] : 0.f;
        hdr->h[a]     = on ? e[a] / (float)dims[a] : 0.f;
        hdr->dims[a]  = dims[a];
    }
    hdr->n_deferred = 0;
    hdr->n_cells    = (uint32_t)cells;
    hdr->pad[0] = hdr->pad[1] = 0;
}

// cell coordinate along one axis; `t` is the value the stop test of the walk uses
__device__ __forceinline__ int knn_axis_cell(float p, float bmin, float scale, int dim, float &t)
{
    t = (p - bmin) * scale;
    return (int)fminf(fmaxf(t, 0.f), (float)(dim - 1)); // fmaxf(NaN, 0) = 0
}

__global__ void __launch_bounds__(256)
    knn_keys_kernel(const float *__restrict__ x, uint32_t N, const KnnHeader *__restrict__ hdr, int64_t *__restrict__ keys)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const float p[3] = {x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2]};
    uint32_t cell    = kKnnNoCell;
    if (knn_finite3(p[0], p[1], p[2])) {
        float t;
        const int cx = knn_axis_cell(p[0], hdr->bmin[0], hdr->scale[0], hdr->dims[0], t);
        const int cy = knn_axis_cell(p[1], hdr->bmin[1], hdr->scale[1], hdr->dims[1], t);
        const int cz = knn_axis_cell(p[2], hdr->bmin[2], hdr->scale[2], hdr->dims[2], t);
        cell         = (uint32_t)((cz * hdr->dims[1] + cy) * hdr->dims[0] + cx);
    }
    keys[i] = (int64_t)(((uint64_t)cell << 32) | (uint64_t)i);
}

__global__ void __launch_bounds__(256)
    knn_gather_kernel(const float *__restrict__ x, const int64_t *__restrict__ keys, uint32_t N, uint32_t M,
                      float4 *__restrict__ sorted, uint32_t *__restrict__ cell_start)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < N) {
        uint32_t src = (uint32_t)((uint64_t)keys[i] & 0xFFFFFFFFull);
        if (src >= N) src = N - 1; // keys that are not ours must not turn into an address
        sorted[i] = make_float4(x[3 * (size_t)src], x[3 * (size_t)src + 1], x[3 * (size_t)src + 2], __uint_as_float(src));
    }
    if (i <= M) {
        const int64_t target = (int64_t)((uint64_t)i << 32);
        uint32_t lo = 0, hi = N;
        for (int it = 0; it < 32; ++it)
            if (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (keys[mid] < target) lo = mid + 1;
                else hi = mid;
            }
        cell_start[i] = lo;
    }
}

template <int KP>
__device__ __forceinline__ void knn_insert(float (&bd)[KP], uint32_t (&bi)[KP], float d, uint32_t id)
{
    if (d < bd[KP - 1]) {
#pragma unroll
        for (int j = KP - 1; j > 0; --j) {
            const bool up   = d < bd[j - 1];
            const bool here = !up && d < bd[j];
            bi[j]           = up ? bi[j - 1] : (here ? id : bi[j]);
            bd[j]           = up ? bd[j - 1] : (here ? d : bd[j]);
        }
        if (d < bd[0]) {
            bd[0] = d;
            bi[0] = id;
        }
    }
}

__device__ __forceinline__ float knn_d2(const float4 &q, const float4 &p)
{
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return (dx * dx + dy * dy) + dz * dz;
}

template <int KP>
__device__ __forceinline__ void knn_scan(const float4 *__restrict__ sorted, uint32_t a, uint32_t b, uint32_t N, const float4 &q,
                                         float (&bd)[KP], uint32_t (&bi)[KP])
{
    b = b < N ? b : N;
    for (uint32_t j = a; j < b; ++j) {
        const float4 p = sorted[j];
        knn_insert<KP>(bd, bi, knn_d2(q, p), __float_as_uint(p.w));
    }
}

template <int KP>
__device__ __forceinline__ void knn_write_row(float *__restrict__ dist, int64_t *__restrict__ idx, uint32_t row, uint32_t K,
                                              const float (&bd)[KP], const uint32_t (&bi)[KP])
{
#pragma unroll
    for (int j = 0; j < KP; ++j)
        if ((uint32_t)j < K) {
            dist[(size_t)row * K + j] = sqrtf(bd[j]);
            if (idx) idx[(size_t)row * K + j] = bi[j] == 0xFFFFFFFFu ? (int64_t)-1 : (int64_t)bi[j];
        }
}

template <int KP>
__global__ void __launch_bounds__(64)
    knn_walk_kernel(const float4 *__restrict__ sorted, const int64_t *__restrict__ keys, const uint32_t *__restrict__ cell_start,
                    KnnHeader *__restrict__ hdr, uint32_t *__restrict__ deferred, uint32_t N, uint32_t K, uint32_t ring_cap,
                    float *__restrict__ dist, int64_t *__restrict__ idx)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= N) return;
    const float4 q      = sorted[i];
    const uint32_t self = __float_as_uint(q.w);
    const uint32_t cell = (uint32_t)((uint64_t)keys[i] >> 32);
    const int DX = hdr->dims[0], DY = hdr->dims[1], DZ = hdr->dims[2];
    if (cell >= (uint32_t)(DX * DY * DZ)) { // a non-finite point (kKnnNoCell)
        for (uint32_t j = 0; j < K; ++j) {
            dist[(size_t)self * K + j] = __uint_as_float(0x7FC00000u);
            if (idx) idx[(size_t)self * K + j] = -1;
        }
        return;
    }
    const int c[3]   = {(int)(cell % (uint32_t)DX), (int)((cell / (uint32_t)DX) % (uint32_t)DY), (int)(cell / (uint32_t)(DX * DY))};
    const int D[3]   = {DX, DY, DZ};
    const float qv[3] = {q.x, q.y, q.z};
    float t[3], h[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        (void)knn_axis_cell(qv[a], hdr->bmin[a], hdr->scale[a], D[a], t[a]);
        h[a] = hdr->h[a] * (1.0f - 1e-6f);
    }
    float bd[KP];
    uint32_t bi[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        bd[j] = INFINITY;
        bi[j] = 0xFFFFFFFFu;
    }
    bool done = false;
    for (uint32_t r = 0; r <= ring_cap && !done; ++r) {
        const int R = (int)r;
        for (int dz = -R; dz <= R; ++dz) {
            const int z = c[2] + dz;
            if (z < 0 || z >= DZ) continue;
            for (int dy = -R; dy <= R; ++dy) {
                const int y = c[1] + dy;
                if (y < 0 || y >= DY) continue;
                const uint32_t row = (uint32_t)((z * DY + y) * DX);
                if (dz == -R || dz == R || dy == -R || dy == R) { // a face of the shell: the whole x range, one contiguous range
                    const int x0 = max(c[0] - R, 0), x1 = min(c[0] + R, DX - 1);
                    knn_scan<KP>(sorted, cell_start[row + (uint32_t)x0], cell_start[row + (uint32_t)x1 + 1u], N, q, bd, bi);
                } else { // inside the shell: its two end cells (R > 0 here)
                    if (c[0] - R >= 0) {
                        const uint32_t cc = row + (uint32_t)(c[0] - R);
                        knn_scan<KP>(sorted, cell_start[cc], cell_start[cc + 1u], N, q, bd, bi);
                    }
                    if (c[0] + R < DX) {
                        const uint32_t cc = row + (uint32_t)(c[0] + R);
                        knn_scan<KP>(sorted, cell_start[cc], cell_start[cc + 1u], N, q, bd, bi);
                    }
                }
            }
        }
        // the nearest face of the (2R+1)^3 block that still has cells behind it
        float bound = INFINITY;
        bool open   = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float slack = 1e-3f + 1e-6f * fabsf(t[a]);
            if (c[a] - R > 0) {
                bound = fminf(bound, fmaxf(((t[a] - (float)(c[a] - R)) - slack) * h[a], 0.f));
                open  = true;
            }
            if (c[a] + R + 1 < D[a]) {
                bound = fminf(bound, fmaxf((((float)(c[a] + R + 1) - t[a]) - slack) * h[a], 0.f));
                open  = true;
            }
        }
        done = !open || bd[KP - 1] <= bound * bound; // false while bound is NaN: such a query ends up deferred
    }
    if (!done) {
        const uint32_t slot = atomicAdd(&hdr->n_deferred, 1u);
        if (slot < N) deferred[slot] = i;
        return;
    }
    knn_write_row<KP>(dist, idx, self, K, bd, bi);
}

template <int KP>
__global__ void __launch_bounds__(256)
    knn_deferred_kernel(const float4 *__restrict__ sorted, const uint32_t *__restrict__ cell_start, uint32_t M,
                        const KnnHeader *__restrict__ hdr, const uint32_t *__restrict__ deferred, uint32_t N, uint32_t K,
                        float *__restrict__ dist, int64_t *__restrict__ idx)
{
    __shared__ float s_d[256 * KP];
    __shared__ uint32_t s_i[256 * KP];
    const uint32_t t   = threadIdx.x;
    const uint32_t cnt = min(hdr->n_deferred, N);
    const uint32_t nf  = min(cell_start[M], N); // the finite points come first in `sorted`
    for (uint32_t qi = blockIdx.x; qi < cnt; qi += (uint32_t)kKnnDeferredBlocks) {
        const uint32_t qpos = min(deferred[qi], N - 1u);
        const float4 q      = sorted[qpos];
        float bd[KP];
        uint32_t bi[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            bd[j] = INFINITY;
            bi[j] = 0xFFFFFFFFu;
        }
        for (uint32_t j = t; j < nf; j += 256u) {
            const float4 p = sorted[j];
            knn_insert<KP>(bd, bi, knn_d2(q, p), __float_as_uint(p.w));
        }
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            s_d[t * KP + j] = bd[j];
            s_i[t * KP + j] = bi[j];
        }
        // pairwise merge of sorted lists: lane t reads lists t and t + s and writes list t, which no other lane reads in this step
        for (uint32_t s = 128; s >= 1; s >>= 1) {
            __syncthreads();
            if (t < s) {
                uint32_t ia = t * KP, ib = (t + s) * KP; // offsets consumed sum to j <= KP - 1: neither list is overrun
#pragma unroll
                for (int j = 0; j < KP; ++j) {
                    const float a = s_d[ia], b = s_d[ib];
                    const bool ta = a <= b;
                    bd[j]         = ta ? a : b;
                    bi[j]         = ta ? s_i[ia] : s_i[ib];
                    ia += ta ? 1u : 0u;
                    ib += ta ? 0u : 1u;
                }
#pragma unroll
                for (int j = 0; j < KP; ++j) {
                    s_d[t * KP + j] = bd[j];
                    s_i[t * KP + j] = bi[j];
                }
            }
        }
        if (t == 0) knn_write_row<KP>(dist, idx, __float_as_uint(q.w), K, bd, bi);
        __syncthreads(); // the lists are rewritten by the next query
    }
}

template <int KP>
static void knn_launch(const float4 *sorted, const int64_t *keys, uint32_t *cell_start, uint32_t M, KnnHeader *hdr,
                       uint32_t *deferred, uint32_t N, uint32_t K, uint32_t ring_cap, float *dist, int64_t *idx, hipStream_t s)
{
    knn_walk_kernel<KP><<<dim3((uint32_t)ceil_div((int64_t)N, 64)), dim3(64), 0, s>>>(sorted, keys, cell_start, hdr, deferred, N,
                                                                                      K, ring_cap, dist, idx);
    knn_deferred_kernel<KP><<<dim3(kKnnDeferredBlocks), dim3(256), 0, s>>>(sorted, cell_start, M, hdr, deferred, N, K, dist, idx);
}

} // namespace gsx

using namespace gsx;

extern "C" int64_t gsx_knn_workspace_bytes(int64_t N, uint32_t K)
{
    (void)K; // the best-lists live in registers and LDS
    if (N <= 0 || N >= 0x7FFFFFFF) return 0;
    return (int64_t)knn_layout(N).total;
}

extern "C" int gsx_knn_bin(const float *x, int64_t N, void *workspace, int64_t *keys, void *stream)
{
    GSX_REQUIRE(N > 0 && N < 0x7FFFFFFF, "gsx_knn_bin: N = %lld outside (0, 2^31 - 1)", (long long)N);
    GSX_REQUIRE(x && workspace && keys, "gsx_knn_bin: null pointer");
    GSX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "gsx_knn_bin: workspace must be 256-byte aligned");
    const KnnLayout L = knn_layout(N);
    hipStream_t s     = (hipStream_t)stream;
    char *w           = static_cast<char *>(workspace);
    KnnHeader *hdr    = reinterpret_cast<KnnHeader *>(w);
    double *partials  = reinterpret_cast<double *>(w + L.partials);
    knn_bbox_kernel<<<dim3(kKnnPartials), dim3(256), 0, s>>>(x, (uint32_t)N, partials);
    knn_grid_kernel<<<dim3(1), dim3(64), 0, s>>>(partials, L.M, hdr);
    knn_keys_kernel<<<dim3((uint32_t)ceil_div(N, 256)), dim3(256), 0, s>>>(x, (uint32_t)N, hdr, keys);
    return check_launch("knn_bin");
}

extern "C" int gsx_knn_search(const float *x, const int64_t *sorted_keys, int64_t N, uint32_t K, uint32_t ring_cap,
                              void *workspace, float *dist, int64_t *idx, void *stream)
{
    GSX_REQUIRE(N > 0 && N < 0x7FFFFFFF, "gsx_knn_search: N = %lld outside (0, 2^31 - 1)", (long long)N);
    GSX_REQUIRE(K >= 1 && K <= 16 && (int64_t)K <= N, "gsx_knn_search: K = %u outside [1, min(16, N)]", K);
    GSX_REQUIRE(ring_cap <= kKnnMaxRingCap, "gsx_knn_search: ring_cap = %u above %u", ring_cap, kKnnMaxRingCap);
    GSX_REQUIRE(x && sorted_keys && workspace && dist, "gsx_knn_search: null pointer");
    GSX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "gsx_knn_search: workspace must be 256-byte aligned");
    const KnnLayout L    = knn_layout(N);
    hipStream_t s        = (hipStream_t)stream;
    char *w              = static_cast<char *>(workspace);
    KnnHeader *hdr       = reinterpret_cast<KnnHeader *>(w);
    uint32_t *cell_start = reinterpret_cast<uint32_t *>(w + L.cell_start);
    float4 *sorted       = reinterpret_cast<float4 *>(w + L.sorted);
    uint32_t *deferred   = reinterpret_cast<uint32_t *>(w + L.deferred);
    const uint32_t n     = (uint32_t)N;
    const int64_t work   = N > (int64_t)L.M + 1 ? N : (int64_t)L.M + 1;
    knn_gather_kernel<<<dim3((uint32_t)ceil_div(work, 256)), dim3(256), 0, s>>>(x, sorted_keys, n, L.M, sorted, cell_start);
    if (K == 1) knn_launch<1>(sorted, sorted_keys, cell_start, L.M, hdr, deferred, n, K, ring_cap, dist, idx, s);
    else if (K <= 4) knn_launch<4>(sorted, sorted_keys, cell_start, L.M, hdr, deferred, n, K, ring_cap, dist, idx, s);
    else if (K <= 8) knn_launch<8>(sorted, sorted_keys, cell_start, L.M, hdr, deferred, n, K, ring_cap, dist, idx, s);
    else knn_launch<16>(sorted, sorted_keys, cell_start, L.M, hdr, deferred, n, K, ring_cap, dist, idx, s);
    return check_launch("knn_search");
}
