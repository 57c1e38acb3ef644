// gsplat_amd — the native grid sort of gsplat_amd.compression.sort (plas_sort): gsx_plas_blur and gsx_plas_step, the two halves
// of one step of the block-assignment sort that orders the splats on PngCompression's parameter grid (the reference imports the
// third-party `plas` package for it, gsplat/compression/sort.py:22-64). The torch functions of sort.py define both results.
//
// gsx_plas_blur   target = box mean of width 2 r + 1 along W, then along H, reflect borders without edge repeat. Two launches of
//                 plas_box_kernel, the first into the workspace. A line of a pass (a grid row for the W pass, a grid column for
//                 the H pass) is cut into segments of S outputs; a lane owns one segment of one channel: it adds the 2 r + 1 taps
//                 of the segment's first window, then slides: sum = sum + (incoming - outgoing). Lanes are numbered channel
//                 first (the W pass: the C floats of a cell, then segments, then rows) resp. along the W * C floats of a grid
//                 row (the H pass), so the H pass reads and writes whole contiguous rows and the W pass 4 C-byte runs that the
//                 next slide steps find in the cache. Cost per output: (2 r + 1) / S + 2 loads, against 2 r + 1 for a tap loop;
//                 a prefix sum would be O(1) but its differences cancel (a prefix over W values carries W u max|x| of error
//                 into a window of 3). S = min(max(32, (2 r + 1) / 8), (max(H, W) + 3) / 2): the first window is 2 r rounded
//                 additions, every slide two, so a mean is off by at most (2 r + 2 (S - 1)) u max|x| <= (max(H, W) + 2 r + 1) u
//                 max|x| per pass.
// gsx_plas_step   plas_step_kernel: the 16 lanes of a DPP row own one group of four cells, a workgroup of 256 lanes 16 groups. The
//                 cells come from the integer definition of sort.py:plas_groups restated in uint32 arithmetic (step_hash is
//                 computed on the host with the same functions); the 16 lanes compute them alike. Lane k holds channels k and
//                 k + 16 of the four rows and the four targets: a load instruction of the wave reads 4 C-byte runs of four
//                 groups' rows instead of one float each of 64 rows (a lane-per-group form of this kernel spent its time
//                 there: 0.51 ms a step at 1000 x 1000 x 14 against 0.10 ms). The lane's share of cost[i][j] is
//                 (x_i[k] - t_j[k])^2 + (x_i[k + 16] - t_j[k + 16])^2 (no fused multiply-add: the unit is built with
//                 -ffp-contract=off), and row16_sum adds the 16 shares in a fixed butterfly that leaves the same bits in
//                 every lane of the row. Then the 24 totals ((cost[p0][0] + cost[p1][1]) + cost[p2][2]) + cost[p3][3] in
//                 lexicographic order with a strict <, so the identity wins ties and a NaN total never wins. Only when the
//                 chosen permutation is not the identity does the lane write its channels back permuted - from registers, all
//                 reads of the group are behind it - and lanes 0..3 move the four index entries. Groups are disjoint: no other
//                 row of lanes touches those cells. improvement and total: one lane per group speaks; wave_sum, the four wave
//                 sums of a workgroup added in order by thread 0 into partials[2 wg], partials[2 wg + 1];
//                 plas_finish_kernel (one workgroup) has lane k add partials k, k + 256, ... in ascending order, then the
//                 same fixed wave / workgroup order. No float atomics: two runs give the same bits.
//
// Bounds: every lane index is checked against the number of segments resp. groups, a group's cells lie inside complete blocks
// (oy + nby * b <= H, ox + nbx * b <= W by construction), reflect() maps [-(n - 1), 2 (n - 1)] into [0, n) and r <= n - 1 is
// required, and the loops run over host arguments.
#include "common.hpp"

namespace gsx {

constexpr int kPlasThreads = 256;
constexpr int kPlasMaxC    = 32;
constexpr int kPlasGroupLanes  = 16;                             // the lanes that own a group: one DPP row, two channels per lane
constexpr int kPlasGroupsPerWg = kPlasThreads / kPlasGroupLanes;
static_assert(kPlasMaxC <= 2 * kPlasGroupLanes, "a lane holds two channels");

__host__ __device__ __forceinline__ uint32_t plas_mix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    return x ^ (x >> 16);
}

static inline uint32_t plas_step_hash(uint32_t seed, uint32_t t) { return plas_mix32(plas_mix32(seed) + t); }

__host__ __device__ __forceinline__ int64_t plas_reflect(int64_t i, int64_t n)
{
    if (i < 0) i = -i;
    if (i >= n) i = 2 * (n - 1) - i;
    return i;
}

// One pass of the box mean, the work of one lane. An element is src[outer * outer_stride + a * axis_stride + inner], a in [0, len)
// along the pass, inner in [0, n_inner) contiguous. Lane = (outer, segment, inner), inner fastest; lane < outer count * n_seg *
// n_inner is the caller's check.
__host__ __device__ __forceinline__ void plas_box_lane(const float *__restrict__ src, float *__restrict__ dst, int64_t lane, int64_t n_inner,
                                                       int64_t n_seg, int64_t len, int64_t axis_stride, int64_t outer_stride, int64_t r,
                                                       int64_t S)
{
    const int64_t inner = lane % n_inner, rest = lane / n_inner;
    const int64_t seg = rest % n_seg, outer = rest / n_seg;
    const float *s    = src + outer * outer_stride + inner;
    float *d          = dst + outer * outer_stride + inner;
    const int64_t a0 = seg * S, a1 = a0 + S < len ? a0 + S : len;
    const float width = (float)(2 * r + 1);
    float sum         = 0.f;
#pragma unroll 4
    for (int64_t k = a0 - r; k <= a0 + r; ++k) sum = sum + s[plas_reflect(k, len) * axis_stride];
    d[a0 * axis_stride] = sum / width;
#pragma unroll 4
    for (int64_t a = a0 + 1; a < a1; ++a) {
        const float in  = s[plas_reflect(a + r, len) * axis_stride];
        const float out = s[plas_reflect(a - 1 - r, len) * axis_stride];
        sum             = sum + (in - out);
        d[a * axis_stride] = sum / width;
    }
}

__global__ void __launch_bounds__(kPlasThreads)
    plas_box_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n_lanes, int64_t n_inner, int64_t n_seg, int64_t len,
                    int64_t axis_stride, int64_t outer_stride, int64_t r, int64_t S)
{
    const int64_t lane = (int64_t)blockIdx.x * kPlasThreads + threadIdx.x;
    if (lane < n_lanes) plas_box_lane(src, dst, lane, n_inner, n_seg, len, axis_stride, outer_stride, r, S);
}

// the cell of slot `x` of a block: three rounds of multiply by an odd key, xorshift, add a key on m = 2 log2(b) bits
__host__ __device__ __forceinline__ uint32_t plas_slot_cell(uint32_t x, const uint32_t (&mul)[3], const uint32_t (&add)[3], uint32_t mask,
                                                   uint32_t shift)
{
#pragma unroll
    for (int rnd = 0; rnd < 3; ++rnd) {
        x = (x * mul[rnd]) & mask;
        x ^= x >> shift;
        x = (x + add[rnd]) & mask;
    }
    return x;
}

// the four cells of group `gid` of a step (sort.py: plas_groups): block gid / (b * b / 4), its slots 4 g .. 4 g + 3
__host__ __device__ __forceinline__ void plas_group_cells(int64_t gid, uint32_t W, uint32_t log2b, uint32_t oy, uint32_t ox, uint32_t nbx,
                                                          uint32_t step_hash, size_t (&cell)[4])
{
    const uint32_t m = 2u * log2b, mask = (1u << m) - 1u, shift = m / 2u > 1u ? m / 2u : 1u, b = 1u << log2b;
    const uint32_t bid = (uint32_t)(gid >> (m - 2u)), g = (uint32_t)gid & ((1u << (m - 2u)) - 1u);
    const uint32_t kb = plas_mix32(step_hash + (bid + 1u) * 0x9E3779B9u);
    uint32_t mul[3], add[3];
#pragma unroll
    for (uint32_t rnd = 0; rnd < 3; ++rnd) {
        mul[rnd] = (plas_mix32(kb + 2u * rnd + 1u) | 1u) & mask;
        add[rnd] = plas_mix32(kb + 2u * rnd + 2u) & mask;
    }
    const uint32_t y0 = oy + (bid / nbx) * b, x0 = ox + (bid % nbx) * b;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t local = plas_slot_cell(4u * g + j, mul, add, mask, shift);
        cell[j]              = (size_t)(y0 + (local >> log2b)) * W + x0 + (local & (b - 1u));
    }
}

struct PlasPerm {
    int p[4];
};
// the 24 permutations of (0, 1, 2, 3) in lexicographic order (q is a compile-time constant wherever this is called: the loop over
// it is unrolled)
__host__ __device__ __forceinline__ constexpr PlasPerm plas_perm(int q)
{
    constexpr PlasPerm perms[24] = {{{0, 1, 2, 3}}, {{0, 1, 3, 2}}, {{0, 2, 1, 3}}, {{0, 2, 3, 1}}, {{0, 3, 1, 2}}, {{0, 3, 2, 1}},
                                    {{1, 0, 2, 3}}, {{1, 0, 3, 2}}, {{1, 2, 0, 3}}, {{1, 2, 3, 0}}, {{1, 3, 0, 2}}, {{1, 3, 2, 0}},
                                    {{2, 0, 1, 3}}, {{2, 0, 3, 1}}, {{2, 1, 0, 3}}, {{2, 1, 3, 0}}, {{2, 3, 0, 1}}, {{2, 3, 1, 0}},
                                    {{3, 0, 1, 2}}, {{3, 0, 2, 1}}, {{3, 1, 0, 2}}, {{3, 1, 2, 0}}, {{3, 2, 0, 1}}, {{3, 2, 1, 0}}};
    return perms[q];
}

template <typename T>
__host__ __device__ __forceinline__ T plas_pick(uint32_t which, T v0, T v1, T v2, T v3)
{
    return which == 0 ? v0 : (which == 1 ? v1 : (which == 2 ? v2 : v3));
}

// sum over the workgroup in a fixed order; the result is valid in thread 0. s_wave: kPlasThreads / 64 floats.
__device__ __forceinline__ float plas_block_sum(float v, float *s_wave)
{
    v = wave_sum(v);
    __syncthreads(); // s_wave may still be read from the previous use
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    float tot = s_wave[0];
#pragma unroll
    for (int w = 1; w < kPlasThreads / 64; ++w) tot = tot + s_wave[w];
    return tot;
}

// One step: the 16 lanes of a DPP row own one group, lane k its channels k and k + 16.
__global__ void __launch_bounds__(kPlasThreads)
    plas_step_kernel(float *__restrict__ grid, const float *__restrict__ target, int32_t *__restrict__ index, uint32_t W, uint32_t C,
                     uint32_t log2b, uint32_t oy, uint32_t ox, uint32_t nbx, uint32_t step_hash, int64_t G, float *__restrict__ partials)
{
    __shared__ float s_wave[kPlasThreads / 64];
    const uint32_t k  = threadIdx.x & (uint32_t)(kPlasGroupLanes - 1);
    const int64_t gid = (int64_t)blockIdx.x * kPlasGroupsPerWg + (threadIdx.x / kPlasGroupLanes);
    const bool live   = gid < G; // the same in the 16 lanes of a row
    size_t cell[4]    = {0, 0, 0, 0};
    if (live) plas_group_cells(gid, W, log2b, oy, ox, nbx, step_hash, cell);
    float x[2][4], cost[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) cost[i][j] = 0.f;
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {
        const uint32_t c = k + (uint32_t)kPlasGroupLanes * half;
        float tg[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[half][i] = 0.f;
            tg[i]      = 0.f;
        }
        if (live && c < C) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[half][i] = grid[cell[i] * C + c];
                tg[i]      = target[cell[i] * C + c];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = x[half][i] - tg[j];
                cost[i][j]    = cost[i][j] + d * d; // a channel this lane does not hold adds (0 - 0)^2 = +0
            }
    }
    // every lane of the row ends up with the same 16 sums: the butterfly adds the same two values in both lanes of a pair
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) cost[i][j] = row16_sum(cost[i][j]);
    constexpr uint32_t kIdentity = 0u | (1u << 2) | (2u << 4) | (3u << 6); // two bits per position: the row that moves there
    const float identity         = ((cost[0][0] + cost[1][1]) + cost[2][2]) + cost[3][3];
    float best                   = identity;
    uint32_t code                = kIdentity;
#pragma unroll
    for (int q = 1; q < 24; ++q) {
        const PlasPerm pm = plas_perm(q);
        const float tot   = ((cost[pm.p[0]][0] + cost[pm.p[1]][1]) + cost[pm.p[2]][2]) + cost[pm.p[3]][3];
        if (tot < best) {
            best = tot;
            code = (uint32_t)pm.p[0] | ((uint32_t)pm.p[1] << 2) | ((uint32_t)pm.p[2] << 4) | ((uint32_t)pm.p[3] << 6);
        }
    }
    if (live && code != kIdentity) {
        const uint32_t p0 = code & 3u, p1 = (code >> 2) & 3u, p2 = (code >> 4) & 3u, p3 = (code >> 6) & 3u;
#pragma unroll
        for (uint32_t half = 0; half < 2; ++half) {
            const uint32_t c = k + (uint32_t)kPlasGroupLanes * half;
            if (c < C) { // the four values of the channel were read above, before anything is written
                grid[cell[0] * C + c] = plas_pick(p0, x[half][0], x[half][1], x[half][2], x[half][3]);
                grid[cell[1] * C + c] = plas_pick(p1, x[half][0], x[half][1], x[half][2], x[half][3]);
                grid[cell[2] * C + c] = plas_pick(p2, x[half][0], x[half][1], x[half][2], x[half][3]);
                grid[cell[3] * C + c] = plas_pick(p3, x[half][0], x[half][1], x[half][2], x[half][3]);
            }
        }
        if (k < 4u) { // lane j moves index entry p[j] to cell j: the four loads are one instruction, ahead of the store
            const uint32_t from = plas_pick(k, p0, p1, p2, p3);
            const int32_t moved = index[plas_pick(from, cell[0], cell[1], cell[2], cell[3])];
            index[plas_pick(k, cell[0], cell[1], cell[2], cell[3])] = moved;
        }
    }
    const bool counts          = live && k == 0u; // one lane speaks for the group
    const float wg_improvement = plas_block_sum(counts ? identity - best : 0.f, s_wave);
    const float wg_total       = plas_block_sum(counts ? identity : 0.f, s_wave);
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x]     = wg_improvement;
        partials[2 * (size_t)blockIdx.x + 1] = wg_total;
    }
}

__global__ void __launch_bounds__(kPlasThreads) plas_finish_kernel(const float *__restrict__ partials, int64_t n_partials, float *__restrict__ result)
{
    __shared__ float s_wave[kPlasThreads / 64];
    float improvement = 0.f, total = 0.f;
    for (int64_t k = threadIdx.x; k < n_partials; k += kPlasThreads) {
        improvement = improvement + partials[2 * k];
        total       = total + partials[2 * k + 1];
    }
    improvement = plas_block_sum(improvement, s_wave);
    total       = plas_block_sum(total, s_wave);
    if (threadIdx.x == 0) {
        result[0] = improvement;
        result[1] = total;
    }
}

static bool plas_shape_ok(int64_t H, int64_t W, uint32_t C)
{
    return H >= 1 && W >= 1 && H < 0x7FFFFFFFll && W < 0x7FFFFFFFll && H * W < 0x80000000ll && C >= 1 && C <= (uint32_t)kPlasMaxC;
}

} // namespace gsx

using namespace gsx;

extern "C" int64_t gsx_plas_workspace_bytes(int64_t H, int64_t W, uint32_t C)
{
    if (!plas_shape_ok(H, W, C)) return 0;
    return H * W * (int64_t)C * (int64_t)sizeof(float);
}

extern "C" int64_t gsx_plas_partials_floats(int64_t H, int64_t W)
{
    if (!plas_shape_ok(H, W, 1)) return 0;
    const int64_t wgs = ceil_div(H * W / 4, kPlasGroupsPerWg);
    return 2 * (wgs > 1 ? wgs : 1);
}

extern "C" int gsx_plas_blur(const float *grid, int64_t H, int64_t W, uint32_t C, int64_t r, float *target, void *workspace, void *stream)
{
    GSX_REQUIRE(plas_shape_ok(H, W, C), "gsx_plas_blur: H = %lld, W = %lld, C = %u outside H W < 2^31, 1 <= C <= %d", (long long)H,
                (long long)W, C, kPlasMaxC);
    GSX_REQUIRE(r >= 1 && r <= (H < W ? H : W) - 1, "gsx_plas_blur: r = %lld outside [1, min(H, W) - 1]", (long long)r);
    GSX_REQUIRE(grid && target && workspace, "gsx_plas_blur: null pointer");
    GSX_REQUIRE(grid != target && (const void *)grid != workspace && (void *)target != workspace, "gsx_plas_blur: buffers must not alias");
    float *mid        = static_cast<float *>(workspace);
    hipStream_t s     = (hipStream_t)stream;
    const int64_t big = H > W ? H : W;
    int64_t S         = (2 * r + 1) / 8 > 32 ? (2 * r + 1) / 8 : 32;
    if (S > (big + 3) / 2) S = (big + 3) / 2;
    {   // along W: lines are grid rows, the C floats of a cell are the contiguous inner index
        const int64_t n_seg = ceil_div(W, S), n_lanes = H * n_seg * C;
        plas_box_kernel<<<dim3((uint32_t)ceil_div(n_lanes, kPlasThreads)), dim3(kPlasThreads), 0, s>>>(grid, mid, n_lanes, C, n_seg, W, C,
                                                                                                    W * C, r, S);
    }
    {   // along H: one "outer" slab, the W * C floats of a grid row are the contiguous inner index
        const int64_t n_seg = ceil_div(H, S), n_lanes = n_seg * W * C;
        plas_box_kernel<<<dim3((uint32_t)ceil_div(n_lanes, kPlasThreads)), dim3(kPlasThreads), 0, s>>>(mid, target, n_lanes, W * C, n_seg,
                                                                                                    H, W * C, 0, r, S);
    }
    return check_launch("plas_blur");
}

extern "C" int gsx_plas_step(float *grid, const float *target, int32_t *index, int64_t H, int64_t W, uint32_t C, uint32_t b,
                             uint32_t seed, uint32_t t, float *partials, float *result, void *stream)
{
    GSX_REQUIRE(plas_shape_ok(H, W, C), "gsx_plas_step: H = %lld, W = %lld, C = %u outside H W < 2^31, 1 <= C <= %d", (long long)H,
                (long long)W, C, kPlasMaxC);
    GSX_REQUIRE(b >= 2 && (b & (b - 1u)) == 0 && b <= 32768u, "gsx_plas_step: b = %u is not a power of two in [2, 32768]", b);
    GSX_REQUIRE(grid && target && index && partials && result, "gsx_plas_step: null pointer");
    GSX_REQUIRE(grid != target, "gsx_plas_step: target must not be grid");
    uint32_t log2b = 0;
    while ((1u << log2b) < b) ++log2b;
    const uint32_t h  = plas_step_hash(seed, t);
    const uint32_t oy = h & (b - 1u), ox = (h >> 16) & (b - 1u);
    const int64_t nby = H > (int64_t)oy ? (H - oy) / b : 0, nbx = W > (int64_t)ox ? (W - ox) / b : 0;
    const int64_t G   = nby * nbx * ((int64_t)b * b / 4); // <= H W / 4
    hipStream_t s     = (hipStream_t)stream;
    const int64_t wgs = ceil_div(G, kPlasGroupsPerWg);   // <= gsx_plas_partials_floats(H, W) / 2
    if (wgs > 0)
        plas_step_kernel<<<dim3((uint32_t)wgs), dim3(kPlasThreads), 0, s>>>(grid, target, index, (uint32_t)W, C, log2b, oy, ox,
                                                                          (uint32_t)nbx, h, G, partials);
    plas_finish_kernel<<<dim3(1), dim3(kPlasThreads), 0, s>>>(partials, wgs, result);
    return check_launch("plas_step");
}
