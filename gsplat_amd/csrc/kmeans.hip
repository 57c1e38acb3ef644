// gsplat_amd — Lloyd's iteration with Manhattan-distance assignment (gsx_kmeans_assign_l1 / gsx_kmeans_update), the kernels
// behind gsplat_amd.compression.kmeans_l1: the SH codebook of PngCompression (the reference asks torchpq's KMeans with
// distance="manhattan" for it, gsplat/compression/png_compression.py:348-351).
//
// The distance of a pair is DEFINED, not merely approximated: one float32 accumulator that starts at 0 and takes
// acc = acc + |x[i, d] - c[j, d]| for d = 0 .. D - 1 in ascending order; the label of a row is the lowest j among the minimal
// distances. No multiply is involved (the unit is built with -ffp-contract=off all the same), a pair's value does not depend on
// where its row or its centroid falls in a tile, and the padded coordinates add |0 - 0| = +0 to a non-negative (or NaN)
// accumulator, which leaves its bits alone. So the labels and distances are the ones a plain loop over d gives, bit for bit.
//
// gsx_kmeans_assign_l1   kmeans_assign_kernel: a workgroup of 256 lanes owns kRowTile = 64 rows (staged once in LDS) and sweeps
//                        all K centroids in tiles of kCenTile = 64 staged through LDS. Both images have a row stride of S floats,
//                        S = 4 * (ceil(D / 4) | 1): D padded to whole 16-byte slots, and an ODD number of slots per row, so the
//                        16 lanes of one ds_read_b128 lane group, which read 16 different rows at the same column, hit 16
//                        different slots. Lane (wave w, lane l): rows (l % 16) + 16 i, centroids 4 (4 w + l / 16) + jj of the
//                        tile, i, jj < 4: a 4 x 4 micro-tile of independent accumulators fed by 4 + 4 128-bit LDS reads per
//                        four coordinates (128 VALU instructions: a subtract and an add with |.| on its source per term). After
//                        a tile every lane folds its 16 distances into its four running (best, label) pairs with a strict <,
//                        centroids ascending; after the sweep the 16 lanes that hold the same row are merged through LDS,
//                        smaller distance first, then smaller label. No row-by-centroid matrix exists anywhere.
//                        A distance that is NaN or +inf is never below the running best: a row all of whose distances are such
//                        (a NaN or infinite coordinate) gets label 0 and best = +inf.
// gsx_kmeans_update      sorted_keys = label << 32 | row ascending, so a cluster is one contiguous range of it.
//                        1. kmeans_bounds_kernel   start[k] = lower bound of k << 32, 32 fixed halvings, k in [0, K]; shift = 0.
//                        2. kmeans_runs_kernel     a half-wave per RUN of kRun = 32 consecutive sorted positions (runs are cut at
//                                                  multiples of 32 whatever the labels are) adds the rows of each label it meets,
//                                                  in sorted order, lane l holding coordinates l, l + 32, l + 64, l + 96. The sum
//                                                  of a label that touches the first position of the run goes to the run's
//                                                  partial slot 0, one that touches only the last position to slot 1, and a
//                                                  label strictly inside the run - a whole cluster - to centroids_out[label].
//                        3. kmeans_finish_kernel   a workgroup per cluster: eight half-waves add the cluster's run partials
//                                                  g, g + 8, g + 16, ... each, the eight sums are added in the order 0 .. 7,
//                                                  divided by the count; an empty cluster copies centroids_in. max |new - old|
//                                                  goes through an LDS integer max and one integer atomicMax on the bits of the
//                                                  (non-negative) float: no float atomics, a fixed order of additions, so the
//                                                  result is bit-equal between runs. All N rows in one cluster are N / 32 runs
//                                                  summed by N / 32 half-waves and N / 256 additions deep in the last kernel.
//
// Termination: every loop runs over a host argument (K tiles, D / 4 steps, 32 positions, 32 halvings, partial count <= N / 32 + 1)
// and every index that comes out of `sorted_keys` is clamped (row < N) or checked (label < K) before it becomes an address.
#include "common.hpp"

#include <math.h>

namespace gsx {

constexpr int kRowTile   = 64;
constexpr int kCenTile   = 64;
constexpr int kKmThreads = 256;
constexpr int kKmMaxD    = 128;
constexpr int kRun       = 32;

static inline uint32_t kmeans_stride(uint32_t D) { return 4u * (((D + 3u) / 4u) | 1u); }

// rows [row0, row0 + 64) of src [n_rows, D] -> tile [64][S], zero beyond D and beyond n_rows. Element e = trow * DP + col of the
// padded tile is taken by lane e % 256, which starts at (trow, col) = (lane / DP, lane % DP) and advances by 256 = q * DP + r without a division.
__device__ __forceinline__ void kmeans_stage(const float *__restrict__ src, int64_t row0, int64_t n_rows, uint32_t D, uint32_t DP,
                                             uint32_t S, uint32_t q, uint32_t r, uint32_t trow, uint32_t col, float *__restrict__ tile)
{
#pragma unroll 4
    for (uint32_t e = threadIdx.x; e < (uint32_t)kRowTile * DP; e += kKmThreads) {
        const int64_t row = row0 + trow;
        float v           = 0.f;
        if (col < D && row < n_rows) v = src[(size_t)row * D + col];
        tile[trow * S + col] = v;
        col += r;
        trow += q;
        if (col >= DP) {
            col -= DP;
            ++trow;
        }
    }
}

__global__ void __launch_bounds__(kKmThreads)
    kmeans_assign_kernel(const float *__restrict__ x, int64_t N, uint32_t D, const float *__restrict__ cen, int64_t K, uint32_t DP,
                         uint32_t S, uint32_t q, uint32_t r, int32_t *__restrict__ labels, float *__restrict__ best_out)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    float *s_x = s_mem;                // [64][S]; columns DP .. S - 1 are never read
    float *s_c = s_mem + kRowTile * S; // [64][S], reused for the merge of the running bests
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t rg = lane & 15u, cg = wave * 4u + (lane >> 4);
    const int64_t row0 = (int64_t)blockIdx.x * kRowTile;

    const uint32_t trow0 = threadIdx.x / DP, col0 = threadIdx.x % DP;
    kmeans_stage(x, row0, N, D, DP, S, q, r, trow0, col0, s_x);

    float best[4];
    int32_t lab[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        best[i] = INFINITY;
        lab[i]  = 0;
    }
    const float *px = s_x + rg * S;
    const float *pc = s_c + cg * 4u * S;
    for (int64_t c0 = 0; c0 < K; c0 += kCenTile) {
        __syncthreads(); // the previous tile has been read (first trip: nothing to wait for but s_x)
        kmeans_stage(cen, c0, K, D, DP, S, q, r, trow0, col0, s_c);
        __syncthreads();
        float acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
#pragma unroll 2
        for (uint32_t d = 0; d < DP; d += 4) {
            v4f xv[4], cv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) xv[i] = *reinterpret_cast<const v4f *>(px + (uint32_t)i * 16u * S + d);
#pragma unroll
            for (int j = 0; j < 4; ++j) cv[j] = *reinterpret_cast<const v4f *>(pc + (uint32_t)j * S + d);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] + fabsf(xv[i][e] - cv[j][e]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t cj = c0 + cg * 4u + j;
            if (cj < K) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (acc[i][j] < best[i]) {
                        best[i] = acc[i][j];
                        lab[i]  = (int32_t)cj;
                    }
            }
        }
    }
    // merge the 16 lanes that hold a row: s_best[cg][row], s_lab[cg][row]
    __syncthreads();
    float *s_best  = s_c;
    int32_t *s_lab = reinterpret_cast<int32_t *>(s_c + 16 * kRowTile);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        s_best[cg * kRowTile + rg + 16u * i] = best[i];
        s_lab[cg * kRowTile + rg + 16u * i]  = lab[i];
    }
    __syncthreads();
    if (threadIdx.x < kRowTile) {
        const int64_t row = row0 + threadIdx.x;
        float b           = s_best[threadIdx.x];
        int32_t l         = s_lab[threadIdx.x];
        for (int g = 1; g < 16; ++g) {
            const float bg   = s_best[g * kRowTile + threadIdx.x];
            const int32_t lg = s_lab[g * kRowTile + threadIdx.x];
            if (bg < b || (bg == b && lg < l)) {
                b = bg;
                l = lg;
            }
        }
        if (row < N) {
            labels[row] = l;
            if (best_out) best_out[row] = b;
        }
    }
}

struct KmeansLayout {
    size_t bounds, partials, total;
    int64_t n_runs;
};

static KmeansLayout kmeans_layout(int64_t N, uint32_t D, int64_t K)
{
    KmeansLayout L;
    auto up    = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.n_runs   = ceil_div(N, kRun);
    L.bounds   = 0;
    L.partials = up(((size_t)K + 1) * sizeof(int32_t));
    L.total    = L.partials + up((size_t)L.n_runs * 2 * D * sizeof(float));
    return L;
}

__global__ void __launch_bounds__(256)
    kmeans_bounds_kernel(const int64_t *__restrict__ keys, uint32_t N, int64_t K, int32_t *__restrict__ start, uint32_t *__restrict__ shift_bits)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k == 0) *shift_bits = 0u;
    if (k > K) return;
    const int64_t target = (int64_t)((uint64_t)k << 32);
    uint32_t lo = 0, hi = N;
    for (int it = 0; it < 32; ++it)
        if (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < target) lo = mid + 1;
            else hi = mid;
        }
    start[k] = (int32_t)lo;
}

__global__ void __launch_bounds__(256)
    kmeans_runs_kernel(const float *__restrict__ x, const int64_t *__restrict__ keys, uint32_t N, uint32_t D, int64_t K,
                       int64_t n_runs, float *__restrict__ partials, float *__restrict__ cen_out)
{
    const uint32_t l  = threadIdx.x & 31u;
    const int64_t run = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (run >= n_runs) return;
    const uint32_t p0 = (uint32_t)run * kRun, p1 = min(p0 + (uint32_t)kRun, N);
    float acc[4]      = {0.f, 0.f, 0.f, 0.f};
    uint32_t cur      = 0;
    bool first        = true; // the open segment holds position p0
    auto flush        = [&](bool last) {
        float *dst = nullptr;
        if (first) dst = partials + ((size_t)run * 2) * D;
        else if (last) dst = partials + ((size_t)run * 2 + 1) * D;
        else if ((int64_t)cur < K) dst = cen_out + (size_t)cur * D;
        if (dst) {
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u)
                if (l + 32u * u < D) dst[l + 32u * u] = acc[u];
        }
    };
    for (uint32_t p = p0; p < p1; ++p) {
        const uint64_t key = (uint64_t)keys[p];
        const uint32_t lb  = (uint32_t)(key >> 32);
        uint32_t row       = (uint32_t)(key & 0xFFFFFFFFull);
        if (row >= N) row = N - 1; // keys that are not ours must not turn into an address
        if (p > p0 && lb != cur) {
            flush(false);
            first = false;
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) acc[u] = 0.f;
        }
        cur = lb;
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u)
            if (l + 32u * u < D) acc[u] = acc[u] + x[(size_t)row * D + l + 32u * u];
    }
    flush(true);
}

__global__ void __launch_bounds__(256)
    kmeans_finish_kernel(const int32_t *__restrict__ start, const float *__restrict__ partials, uint32_t N, uint32_t D, int64_t n_runs,
                         const float *__restrict__ cen_in, float *__restrict__ cen_out, int32_t *__restrict__ counts,
                         uint32_t *__restrict__ shift_bits)
{
    __shared__ float s_sum[8][kKmMaxD];
    __shared__ uint32_t s_max;
    const int64_t k  = blockIdx.x;
    const uint32_t l = threadIdx.x & 31u, g = threadIdx.x >> 5;
    uint32_t a0 = (uint32_t)start[k], a1 = (uint32_t)start[k + 1];
    a0               = min(a0, N);
    a1               = min(max(a1, a0), N);
    const uint32_t n = a1 - a0;
    if (threadIdx.x == 0) {
        counts[k] = (int32_t)n;
        s_max     = 0u;
    }
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    if (n > 0) { // uniform over the workgroup
        const uint32_t ra = a0 / kRun, rb = (a1 - 1u) / kRun;
        const bool at_edge  = a0 == ra * kRun;
        const bool interior = ra == rb && !at_edge && a1 != min((ra + 1u) * kRun, N);
        if (interior) {
            if (g == 0)
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u)
                    if (l + 32u * u < D) sum[u] = cen_out[(size_t)k * D + l + 32u * u]; // the whole sum, left by kmeans_runs_kernel
        } else {
            const uint32_t m = rb - ra + 1u;
            for (uint32_t i = g; i < m; i += 8u) {
                const uint32_t slot = (i == 0 && !at_edge) ? 1u : 0u;
                const float *src    = partials + ((size_t)(ra + i) * 2 + slot) * D;
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u)
                    if (l + 32u * u < D) sum[u] = sum[u] + src[l + 32u * u];
            }
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) s_sum[g][l + 32u * u] = sum[u];
            __syncthreads();
            if (g == 0)
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) {
                    float t = s_sum[0][l + 32u * u];
                    for (int h = 1; h < 8; ++h) t = t + s_sum[h][l + 32u * u];
                    sum[u] = t;
                }
        }
    }
    __syncthreads(); // s_max = 0 is visible
    if (g == 0) {
        uint32_t mx = 0u;
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u)
            if (l + 32u * u < D) {
                const size_t at = (size_t)k * D + l + 32u * u;
                const float old = cen_in[at];
                const float nw  = n > 0 ? sum[u] / (float)n : old;
                cen_out[at]     = nw;
                mx              = max(mx, __float_as_uint(fabsf(nw - old))); // non-negative floats order like their bits; NaN on top
            }
        if (mx) atomicMax(&s_max, mx);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_max > __atomic_load_n(shift_bits, __ATOMIC_RELAXED)) atomicMax(shift_bits, s_max); // the load only filters
}

} // namespace gsx

using namespace gsx;

extern "C" int gsx_kmeans_assign_l1(const float *x, int64_t N, uint32_t D, const float *centroids, int64_t K, int32_t *labels,
                                    float *best, void *stream)
{
    GSX_REQUIRE(N >= 0 && N < 0x7FFFFFFFll, "gsx_kmeans_assign_l1: N = %lld outside [0, 2^31 - 1)", (long long)N);
    GSX_REQUIRE(D >= 1 && D <= (uint32_t)kKmMaxD, "gsx_kmeans_assign_l1: D = %u outside [1, %d]", D, kKmMaxD);
    GSX_REQUIRE(K >= 1 && K < 0x7FFFFFFFll, "gsx_kmeans_assign_l1: K = %lld outside [1, 2^31 - 1)", (long long)K);
    if (N == 0) return GSX_OK;
    GSX_REQUIRE(x && centroids && labels, "gsx_kmeans_assign_l1: null pointer");
    const uint32_t DP = (D + 3u) & ~3u, S = kmeans_stride(D);
    // two images of 64 rows; the merge of the running bests reuses the centroid image and needs 16 * 64 * (4 + 4) bytes of it
    const size_t image = (size_t)kCenTile * S * sizeof(float), merge = (size_t)16 * kRowTile * (sizeof(float) + sizeof(int32_t));
    const size_t need  = (size_t)kRowTile * S * sizeof(float) + (image > merge ? image : merge);
    static PerDeviceOnce once;
    if (once.first())
        (void)hipFuncSetAttribute((const void *)kmeans_assign_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
    kmeans_assign_kernel<<<dim3((uint32_t)ceil_div(N, kRowTile)), dim3(kKmThreads), need, (hipStream_t)stream>>>(
        x, N, D, centroids, K, DP, S, (uint32_t)kKmThreads / DP, (uint32_t)kKmThreads % DP, labels, best);
    return check_launch("kmeans_assign_l1");
}

extern "C" int64_t gsx_kmeans_workspace_bytes(int64_t N, uint32_t D, int64_t K)
{
    if (N <= 0 || N >= 0x7FFFFFFFll || D < 1 || D > (uint32_t)kKmMaxD || K < 1 || K >= 0x7FFFFFFFll) return 0;
    return (int64_t)kmeans_layout(N, D, K).total;
}

extern "C" int gsx_kmeans_update(const float *x, int64_t N, uint32_t D, const int32_t *labels, const int64_t *sorted_keys, int64_t K,
                                 const float *centroids_in, float *centroids_out, int32_t *counts, float *shift, void *workspace,
                                 void *stream)
{
    (void)labels; // the sorted keys carry them
    GSX_REQUIRE(N > 0 && N < 0x7FFFFFFFll, "gsx_kmeans_update: N = %lld outside (0, 2^31 - 1)", (long long)N);
    GSX_REQUIRE(D >= 1 && D <= (uint32_t)kKmMaxD, "gsx_kmeans_update: D = %u outside [1, %d]", D, kKmMaxD);
    GSX_REQUIRE(K >= 1 && K < 0x7FFFFFFFll, "gsx_kmeans_update: K = %lld outside [1, 2^31 - 1)", (long long)K);
    GSX_REQUIRE(x && sorted_keys && centroids_in && centroids_out && counts && shift && workspace, "gsx_kmeans_update: null pointer");
    GSX_REQUIRE(centroids_in != centroids_out, "gsx_kmeans_update: centroids_out must not be centroids_in");
    GSX_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0, "gsx_kmeans_update: workspace must be 256-byte aligned");
    const KmeansLayout L = kmeans_layout(N, D, K);
    hipStream_t s        = (hipStream_t)stream;
    char *w              = static_cast<char *>(workspace);
    int32_t *start       = reinterpret_cast<int32_t *>(w + L.bounds);
    float *partials      = reinterpret_cast<float *>(w + L.partials);
    uint32_t *shift_bits = reinterpret_cast<uint32_t *>(shift);
    kmeans_bounds_kernel<<<dim3((uint32_t)ceil_div(K + 1, 256)), dim3(256), 0, s>>>(sorted_keys, (uint32_t)N, K, start, shift_bits);
    kmeans_runs_kernel<<<dim3((uint32_t)ceil_div(L.n_runs, 8)), dim3(256), 0, s>>>(x, sorted_keys, (uint32_t)N, D, K, L.n_runs, partials,
                                                                                  centroids_out);
    kmeans_finish_kernel<<<dim3((uint32_t)K), dim3(256), 0, s>>>(start, partials, (uint32_t)N, D, L.n_runs, centroids_in, centroids_out,
                                                                counts, shift_bits);
    return check_launch("kmeans_update");
}
