// HexPlane feature field of the dynamic-scene trainer (examples/dynamic_surgical_trainer.py; semantics restated from
// gsplat/contrib/dynamic/hexplane.py: HexPlaneField with grid_dimensions 2, four input coordinates, 32 channels per plane).
// C-ABI: gsx_hexplane_scale_cells / _pack / _unpack / _fwd / _bwd.
//
// A point (x, y, z, t) samples, per scale, the six planes xy, xz, xt, yz, yt, zt bilinearly (align_corners = true, border
// padding, as grid_sample does) and multiplies the six 32-channel samples element-wise; the scales are concatenated.
// x, y, z are first mapped to [-1, 1] by (v - aabb[0]) * (2 / (aabb[1] - aabb[0])) - 1, t is taken as it is. For plane (a, b)
// coordinate a runs along W = res[a] and coordinate b along H = res[b]; index u = ((c + 1) / 2) * (size - 1), clamped to
// [0, size - 1].
//
// Layout: the parameters stay [1, 32, H, W] (channel-major: the 32 channels of a cell are H * W floats apart). The kernels work
// on a channel-last arena [cells of all planes of all scales][32]: a cell is one 128-byte line, the two x-neighbours of a
// bilinear footprint are 256 contiguous bytes. hexplane_layout_kernel<true> fills a scale's part of the arena from its six
// planes (a 64-cell x 32-channel tile through LDS, both sides coalesced); <false> writes the six gradient tensors from the
// gradient arena, every element.
//
// Corners: i0 = min(floor(u), size - 2) and f = u - i0, so both corners i0 and i0 + 1 are inside the plane for every u in
// [0, size - 1]; at u = size - 1 the weights are (0, 1), the values grid_sample gives with its zero-weight corner at `size`
// left out. The clamps are on the float index (fmax first: a NaN becomes 0) and once more on the integer, so a load address
// cannot leave the plane for any bit pattern of the coordinates. Non-finite coordinates therefore give finite border samples:
// a NaN or -inf index samples cell 0 of its axis, +inf the last cell (for x, y, z that is the index after the normalisation,
// which flips the sign with aabb[0] = +bounds), and they pass no gradient.
//
// Forward: eight lanes per point, each with a float4 of channels: a corner is one 128-byte load per point, the output row
// of a scale one 128-byte store. 32 points per workgroup of four waves; only features [N, S * 32] is written.
//
// Backward (recomputes the samples): one wave per point and trip; lane = (x corner, channel), so that every load and every
// atomic instruction of the wave is the 256 contiguous bytes of the two x-neighbours of one plane row. The halves are joined by
// one lane swap. dI_p = v_feature * prod_{q != p} I_q by prefix and suffix products (no division: planes may hold zeros).
// Plane gradients are float atomic adds (global_atomic_add_f32, no return) into the channel-last gradient arena, which the
// entry point zeroes on the stream: 12 instructions of 256 bytes per point and scale. Their sums depend on arrival order, so the
// plane gradients of two runs may differ in the last bits. v_xyzt sums, per lane, its channel's share over planes and scales
// (zero where the index was clamped: the test is 0 < u < size - 1 on the unclamped index), chained through (size - 1) / 2 and,
// for x, y, z, 2 / (aabb[1] - aabb[0]); the 64 lanes are added by wave_sum4_scatter, a fixed order: two runs give the same
// bits, as they do for features. A persistent grid of kHpBwdBlocks workgroups; wave w of the grid takes points w, w + waves, ...
#include "common.hpp"

namespace gsx {

constexpr int kHpC         = 32;   // channels per plane
constexpr int kHpMaxScales = 4;
constexpr int kHpMinRes = 2, kHpMaxRes = 2048;
constexpr int kHpThreads   = 256;
constexpr int kHpFwdPoints = kHpThreads / 8; // forward: eight lanes per point
constexpr int kHpBwdWaves  = kHpThreads / kWave;
// The grid A/B of profiles/hexplane.json (tools/hexplane_bench.py --grid-lib): the backward runs at the chip's float-atomic rate,
// 2048 and 4096 workgroups measure the same and 512 half a percent slower.
#ifndef GSX_HEXPLANE_BWD_BLOCKS
#define GSX_HEXPLANE_BWD_BLOCKS 2048
#endif
constexpr int kHpBwdBlocks = GSX_HEXPLANE_BWD_BLOCKS; // persistent backward grid: 8192 waves, one point each per trip
constexpr int kHpTile      = 64;             // cells per workgroup of the layout kernels

// The layout A/B of profiles/hexplane.json (tools/hexplane_bench.py --ab-lib): a library built with
// -DGSX_HEXPLANE_CHANNEL_MAJOR=1 keeps every plane's part of the arena as the parameter lies in memory, [32][cells], so the
// sampling kernels read and add as they would on the parameters in place: a channel per lane, every lane of a load or an atomic
// instruction on a cache line of its own (the forward gathers its float4 from four lines). Not a product configuration.
#ifndef GSX_HEXPLANE_CHANNEL_MAJOR
#define GSX_HEXPLANE_CHANNEL_MAJOR 0
#endif
constexpr bool kHpChannelMajor = GSX_HEXPLANE_CHANNEL_MAJOR != 0;

// float index of channel ch of cell `cell` of the plane of `cells` cells that starts at arena cell `base`
__device__ __forceinline__ size_t hp_at(uint32_t base, size_t cells, size_t cell, int ch)
{
    return kHpChannelMajor ? (size_t)base * kHpC + (size_t)ch * cells + cell : ((size_t)base + cell) * kHpC + ch;
}

// plane p = (kHpA[p], kHpB[p]): itertools.combinations(range(4), 2)
__device__ __host__ constexpr int hp_a(int p) { return p < 3 ? 0 : (p < 5 ? 1 : 2); }
__device__ __host__ constexpr int hp_b(int p) { return p < 3 ? p + 1 : (p < 5 ? p - 1 : 3); }

struct HpScale {
    int res[4];       // x, y, z, t
    uint32_t base[6]; // first arena cell of each plane
};

struct HpArgs {
    const float *xyzt;  // [N, 4] contiguous
    const float *aabb;  // [2, 3]
    const float *arena; // [cells][32], 16-byte aligned
    int64_t N;
    int S;
    HpScale sc[kHpMaxScales];
    float *features;         // fwd: [N, S * 32], 16-byte aligned
    const float *v_features; // bwd: [N, S * 32]
    float *v_xyzt;           // bwd: [N, 4] or null
    float *v_arena;          // bwd: [cells][32], zeroed, or null
};

struct HpPlanes {
    float *plane[6];      // [32][cells[p]]
    uint32_t cells[6];
    uint32_t base[6];     // first arena cell of the plane, relative to the scale's part
    uint32_t tile0[7];    // first workgroup of each plane; tile0[6] = grid size
};

struct HpAxis {
    int i0;  // lower corner, in [0, size - 2]
    float f; // weight of the upper corner
    float m; // d index / d coordinate where the index is not clamped, else 0
};

__device__ __forceinline__ HpAxis hp_axis(float c, int size)
{
    const float top = (float)(size - 1);
    const float u   = ((c + 1.0f) * 0.5f) * top;
    const float uc  = fminf(fmaxf(u, 0.0f), top); // fmax first: NaN -> 0
    HpAxis r;
    r.i0 = max(min((int)uc, size - 2), 0);
    r.f  = uc - (float)r.i0;
    r.m  = (u > 0.0f && u < top) ? 0.5f * top : 0.0f;
    return r;
}

// one rounding per operation, in the order the contract states
__device__ __forceinline__ float hp_normalize(float v, float a0, float k)
{
#pragma clang fp contract(off)
    return (v - a0) * k - 1.0f;
}

__device__ __forceinline__ void hp_coords(const HpArgs &a, int64_t n, float c[4], float k[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float a0 = a.aabb[i], a1 = a.aabb[3 + i];
        k[i] = 2.0f / (a1 - a0);
        c[i] = hp_normalize(a.xyzt[n * 4 + i], a0, k[i]);
    }
    c[3] = a.xyzt[n * 4 + 3];
}

__global__ void __launch_bounds__(kHpThreads) hexplane_fwd_kernel(HpArgs a)
{
    const int sub   = (int)threadIdx.x & 7;
    const int64_t n = (int64_t)blockIdx.x * kHpFwdPoints + ((int)threadIdx.x >> 3);
    if (n >= a.N) return;
    float c[4], k[3];
    hp_coords(a, n, c, k);
    const v4f *arena = reinterpret_cast<const v4f *>(a.arena);
    v4f *out         = reinterpret_cast<v4f *>(a.features) + n * (a.S * (kHpC / 4)) + sub;
    for (int s = 0; s < a.S; ++s) {
        const HpScale &sc = a.sc[s];
        HpAxis ax[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) ax[i] = hp_axis(c[i], sc.res[i]);
        v4f prod = {1.0f, 1.0f, 1.0f, 1.0f};
#pragma unroll
        for (int p = 0; p < 6; ++p) {
            const HpAxis &X = ax[hp_a(p)], &Y = ax[hp_b(p)];
            const size_t W = (size_t)sc.res[hp_a(p)], cell = (size_t)Y.i0 * W + (size_t)X.i0;
            v4f v00, v01, v10, v11;
            if constexpr (kHpChannelMajor) {
                const size_t cells = W * (size_t)sc.res[hp_b(p)];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float *q = a.arena + hp_at(sc.base[p], cells, cell, 4 * sub + j);
                    v00[j] = q[0]; v01[j] = q[1]; v10[j] = q[W]; v11[j] = q[W + 1];
                }
            } else {
                const v4f *q = arena + ((size_t)sc.base[p] + cell) * (kHpC / 4) + sub;
                v00 = q[0]; v01 = q[kHpC / 4]; v10 = q[W * (kHpC / 4)]; v11 = q[W * (kHpC / 4) + kHpC / 4];
            }
            const float gx = 1.0f - X.f, gy = 1.0f - Y.f;
            v4f I = v00 * (gx * gy);
            I += v01 * (X.f * gy);
            I += v10 * (gx * Y.f);
            I += v11 * (X.f * Y.f);
            prod *= I;
        }
        out[s * (kHpC / 4)] = prod;
    }
}

// low half + high half, in every lane
__device__ __forceinline__ float hp_join_halves(float x)
{
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

__global__ void __launch_bounds__(kHpThreads) hexplane_bwd_kernel(HpArgs a)
{
    const int lane = lane_id(), ch = lane & (kHpC - 1);
    const bool hi  = lane >= kHpC; // the x corner of this lane
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int F    = a.S * kHpC;
    for (int64_t n = (int64_t)blockIdx.x * kHpBwdWaves + wave; n < a.N; n += (int64_t)gridDim.x * kHpBwdWaves) {
        float c[4], k[3];
        hp_coords(a, n, c, k);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int s = 0; s < a.S; ++s) {
            const HpScale &sc = a.sc[s];
            HpAxis ax[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) ax[i] = hp_axis(c[i], sc.res[i]);
            const float g = a.v_features[n * F + s * kHpC + ch];
            float wx[6], col[6], dy[6], I[6];
            size_t at[6], up[6]; // the lane's element in the lower row, and the distance to the upper one
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                const HpAxis &X = ax[hp_a(p)], &Y = ax[hp_b(p)];
                const size_t W = (size_t)sc.res[hp_a(p)];
                at[p] = hp_at(sc.base[p], W * (size_t)sc.res[hp_b(p)], (size_t)Y.i0 * W + (size_t)X.i0 + (hi ? 1 : 0), ch);
                up[p] = kHpChannelMajor ? W : W * kHpC;
                const float v0 = a.arena[at[p]], v1 = a.arena[at[p] + up[p]];
                wx[p]  = hi ? X.f : 1.0f - X.f;
                col[p] = (1.0f - Y.f) * v0 + Y.f * v1;
                dy[p]  = v1 - v0;
                I[p]   = hp_join_halves(wx[p] * col[p]);
            }
            float pre[6], suf = 1.0f; // pre[p] = g * I_0 .. I_{p-1}
            pre[0] = g;
#pragma unroll
            for (int p = 1; p < 6; ++p) pre[p] = pre[p - 1] * I[p - 1];
#pragma unroll
            for (int p = 5; p >= 0; --p) {
                const float dI = pre[p] * suf;
                suf *= I[p];
                const HpAxis &X = ax[hp_a(p)], &Y = ax[hp_b(p)];
                if (a.v_arena) {
                    const float w = dI * wx[p];
                    atomic_add_f32(a.v_arena + at[p], w * (1.0f - Y.f));
                    atomic_add_f32(a.v_arena + at[p] + up[p], w * Y.f);
                }
                acc[hp_a(p)] += X.m * (dI * (hi ? col[p] : -col[p]));
                acc[hp_b(p)] += Y.m * (dI * (wx[p] * dy[p]));
            }
        }
        if (a.v_xyzt) {
            const float r = wave_sum4_scatter(acc[0] * k[0], acc[1] * k[1], acc[2] * k[2], acc[3]);
            if ((lane & 15) == 0) a.v_xyzt[n * 4 + (lane >> 4)] = r;
        }
    }
}

// PACK: arena[(base[p] + cell) * 32 + c] = plane[p][c * cells[p] + cell]; else the other way round, every plane element written.
template <bool PACK>
__global__ void __launch_bounds__(kHpThreads) hexplane_layout_kernel(HpPlanes pl, float *arena)
{
    __shared__ float s_t[kHpC][kHpTile + 1];
    int p = 0;
    while (p < 5 && blockIdx.x >= pl.tile0[p + 1]) ++p;
    const uint32_t cell0 = (blockIdx.x - pl.tile0[p]) * kHpTile, cells = pl.cells[p];
    float *plane = pl.plane[p];
    float *rows  = arena + hp_at(pl.base[p], cells, cell0, 0); // the tile's first element in the arena
    const size_t cs = kHpChannelMajor ? 1 : kHpC, hs = kHpChannelMajor ? cells : 1; // its cell and channel strides
    const int t  = (int)threadIdx.x;
#pragma unroll
    for (int i = 0; i < kHpC * kHpTile / kHpThreads; ++i) {
        if (PACK) {
            const int c = i * (kHpThreads / kHpTile) + (t >> 6), j = t & (kHpTile - 1);
            if (cell0 + j < cells) s_t[c][j] = plane[(size_t)c * cells + cell0 + j];
        } else {
            const int j = i * (kHpThreads / kHpC) + (t >> 5), c = t & (kHpC - 1);
            if (cell0 + j < cells) s_t[c][j] = rows[(size_t)j * cs + (size_t)c * hs];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kHpC * kHpTile / kHpThreads; ++i) {
        if (PACK) {
            const int j = i * (kHpThreads / kHpC) + (t >> 5), c = t & (kHpC - 1);
            if (cell0 + j < cells) rows[(size_t)j * cs + (size_t)c * hs] = s_t[c][j];
        } else {
            const int c = i * (kHpThreads / kHpTile) + (t >> 6), j = t & (kHpTile - 1);
            if (cell0 + j < cells) plane[(size_t)c * cells + cell0 + j] = s_t[c][j];
        }
    }
}

} // namespace gsx

using namespace gsx;

// The planes of one scale, in order, from `first`; returns the number of cells (0: a resolution out of range).
static int64_t hp_scale(HpScale &sc, int64_t rx, int64_t ry, int64_t rz, int64_t rt, int64_t first)
{
    const int64_t res[4] = {rx, ry, rz, rt};
    int64_t cells = 0;
    for (int i = 0; i < 4; ++i) {
        if (res[i] < kHpMinRes || res[i] > kHpMaxRes) return 0;
        sc.res[i] = (int)res[i];
    }
    for (int p = 0; p < 6; ++p) {
        sc.base[p] = (uint32_t)(first + cells);
        cells += res[hp_a(p)] * res[hp_b(p)];
    }
    return cells;
}

extern "C" int64_t gsx_hexplane_scale_cells(uint32_t rx, uint32_t ry, uint32_t rz, uint32_t rt)
{
    HpScale sc;
    return hp_scale(sc, rx, ry, rz, rt, 0);
}

template <bool PACK>
static int hp_layout(const char *who, float *const planes[6], uint32_t rx, uint32_t ry, uint32_t rz, uint32_t rt, float *arena,
                     void *stream)
{
    HpScale sc;
    GSX_REQUIRE(hp_scale(sc, rx, ry, rz, rt, 0) > 0, "%s: resolution (%u, %u, %u, %u) outside [%d, %d]", who, rx, ry, rz, rt,
                kHpMinRes, kHpMaxRes);
    GSX_REQUIRE(arena, "%s: null argument", who);
    HpPlanes pl;
    pl.tile0[0] = 0;
    for (int p = 0; p < 6; ++p) {
        GSX_REQUIRE(planes[p], "%s: null argument", who);
        pl.plane[p]     = planes[p];
        pl.cells[p]     = (uint32_t)(sc.res[hp_a(p)] * sc.res[hp_b(p)]);
        pl.base[p]      = sc.base[p];
        pl.tile0[p + 1] = pl.tile0[p] + (uint32_t)ceil_div(pl.cells[p], kHpTile);
    }
    hexplane_layout_kernel<PACK><<<dim3(pl.tile0[6]), kHpThreads, 0, (hipStream_t)stream>>>(pl, arena);
    return check_launch(who);
}

extern "C" int gsx_hexplane_pack(const float *xy, const float *xz, const float *xt, const float *yz, const float *yt,
                                 const float *zt, uint32_t rx, uint32_t ry, uint32_t rz, uint32_t rt, float *arena, void *stream)
{
    float *const planes[6] = {const_cast<float *>(xy), const_cast<float *>(xz), const_cast<float *>(xt),
                              const_cast<float *>(yz), const_cast<float *>(yt), const_cast<float *>(zt)};
    return hp_layout<true>("gsx_hexplane_pack", planes, rx, ry, rz, rt, arena, stream);
}

extern "C" int gsx_hexplane_unpack(const float *v_arena, uint32_t rx, uint32_t ry, uint32_t rz, uint32_t rt, float *v_xy,
                                   float *v_xz, float *v_xt, float *v_yz, float *v_yt, float *v_zt, void *stream)
{
    float *const planes[6] = {v_xy, v_xz, v_xt, v_yz, v_yt, v_zt};
    return hp_layout<false>("gsx_hexplane_unpack", planes, rx, ry, rz, rt, const_cast<float *>(v_arena), stream);
}

// Returns the arena's cell count through `cells`.
static int hp_args(const char *who, HpArgs &a, const float *xyzt, int64_t N, const float *aabb, const float *arena,
                   const int32_t *res, uint32_t S, int64_t &cells)
{
    GSX_REQUIRE(xyzt && aabb && arena && res, "%s: null argument", who);
    GSX_REQUIRE(N > 0 && N < (int64_t)1 << 31, "%s: N %lld out of range", who, (long long)N);
    GSX_REQUIRE(S >= 1 && S <= (uint32_t)kHpMaxScales, "%s: %u scales, 1 to %d supported", who, S, kHpMaxScales);
    GSX_REQUIRE(((uintptr_t)arena & 15) == 0, "%s: arena not 16-byte aligned", who);
    cells = 0;
    for (uint32_t s = 0; s < S; ++s) {
        const int32_t *r = res + 4 * s;
        const int64_t c  = hp_scale(a.sc[s], r[0], r[1], r[2], r[3], cells);
        GSX_REQUIRE(c > 0, "%s: resolution (%d, %d, %d, %d) of scale %u outside [%d, %d]", who, r[0], r[1], r[2], r[3], s,
                    kHpMinRes, kHpMaxRes);
        cells += c;
    }
    a.xyzt = xyzt; a.aabb = aabb; a.arena = arena; a.N = N; a.S = (int)S;
    return GSX_OK;
}

extern "C" int gsx_hexplane_fwd(const float *xyzt, int64_t N, const float *aabb, const float *arena, const int32_t *res,
                                uint32_t S, float *features, void *stream)
{
    if (N == 0) return GSX_OK;
    HpArgs a{};
    int64_t cells;
    if (int rc = hp_args("gsx_hexplane_fwd", a, xyzt, N, aabb, arena, res, S, cells)) return rc;
    GSX_REQUIRE(features && ((uintptr_t)features & 15) == 0, "gsx_hexplane_fwd: features null or not 16-byte aligned");
    a.features = features;
    hexplane_fwd_kernel<<<dim3((unsigned)ceil_div(N, kHpFwdPoints)), kHpThreads, 0, (hipStream_t)stream>>>(a);
    return check_launch("hexplane_fwd");
}

extern "C" int gsx_hexplane_bwd(const float *xyzt, int64_t N, const float *aabb, const float *arena, const int32_t *res,
                                uint32_t S, const float *v_features, float *v_xyzt, float *v_arena, void *stream)
{
    if (N == 0) return GSX_OK;
    HpArgs a{};
    int64_t cells;
    if (int rc = hp_args("gsx_hexplane_bwd", a, xyzt, N, aabb, arena, res, S, cells)) return rc;
    GSX_REQUIRE(v_features, "gsx_hexplane_bwd: null argument");
    if (!v_xyzt && !v_arena) return GSX_OK;
    a.v_features = v_features; a.v_xyzt = v_xyzt; a.v_arena = v_arena;
    if (v_arena && hipMemsetAsync(v_arena, 0, (size_t)cells * kHpC * sizeof(float), (hipStream_t)stream) != hipSuccess) {
        set_last_error("gsx_hexplane_bwd: cannot zero the gradient arena");
        return GSX_ERR_ARG;
    }
    const int64_t blocks = ceil_div(N, kHpBwdWaves);
    hexplane_bwd_kernel<<<dim3((unsigned)(blocks < kHpBwdBlocks ? blocks : kHpBwdBlocks)), kHpThreads, 0, (hipStream_t)stream>>>(a);
    return check_launch("hexplane_bwd");
}
