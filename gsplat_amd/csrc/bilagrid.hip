// Bilateral-grid appearance model of the training step (examples/simple_trainer.py:571-577, 766-776, 981-984 with
// post_processing="bilateral_grid"; semantics restated from examples/lib_bilagrid.py:110-295 and gsplat/losses.py:642-667).
// C-ABI: gsx_bilagrid_slice_fwd / gsx_bilagrid_slice_bwd / gsx_tv_fwd / gsx_tv_bwd.
//
// A pixel of colour rgb at image position (u, v) in [0, 1]^2 samples a grid [12, L, Hg, Wg] of 3 x 4 affine matrices trilinearly
// at (ix, iy, iz) = (u (Wg - 1), v (Hg - 1), gray (L - 1)), gray = 0.299 r + 0.587 g + 0.114 b, each index clamped to its axis
// (F.grid_sample, align_corners=True, padding_mode="border": a clamped index passes no gradient), and leaves
// rgb_out = A[:, :3] rgb + A[:, 3].
//
// Forward: one thread per pixel, 8 corners x 12 channels read through L1 (a grid is 96 KiB), nothing but rgb_out is written
// unless the matrices are asked for.
//
// Backward: every pixel adds 8 corners x 12 channels to a grid of L Hg Wg 12 floats - thousands of contributions per element.
// With pixel-centre coordinates (no xy tensor) the sum is taken on chip: one workgroup owns the pixels whose (floor ix, floor iy)
// is ONE grid cell (or a band of rows of it), so it touches 2 x 2 x L corners = 48 L floats. Those accumulators live in LDS,
// replicated R = 32 times with the replica as the fastest index: lane l adds into replica l % 32, at dword (accumulator * 32 +
// l % 32). The intent: neighbouring pixels share their corners, so unreplicated a wave's lanes would pile onto a few addresses;
// replicated, the 32 lanes that a 4-byte LDS operation services together ({0-31}, {32-63}) hit 32 different dwords whose
// addresses differ modulo 32 and modulo 64 dwords whichever corner each lane hits, and lanes l and l + 32, which share a
// replica, are serviced in different passes. That reasoning rests on the LDS tables of the microarchitecture notes, which are
// given for ds_read / ds_write, not for ds_add_f32; no bank-conflict counter was read. What was measured is the whole kernel
// against the global-atomic scatter below (profiles/bilagrid.json). At the end the workgroup adds the
// replicas and sends one global atomic per non-zero accumulator. A pixel belongs to the workgroup whose cell its own float
// arithmetic names; the pixel rectangle scanned per cell is that cell's exact rectangle widened by two pixels, which covers the
// rounding of a pixel's float index for every image side the entry point admits (< 2^22, where that error is below a pixel).
// The cell's 48 L grid values are staged in LDS as well. v_rgb (through the affine product and through the guidance iz) is
// written by the same pass, every element.
// With an xy tensor the corners of a workgroup's pixels are arbitrary: that case is the SIMPLER accumulation, one global
// atomicAdd per (pixel, corner, channel), as is a guidance dimension too large for 64 KiB of LDS (L > 170: 48 L staged values
// plus at least one replica of 48 L sums).
// v_grids or v_rgb may be null: that gradient is not wanted, and its sums / its stores are skipped.
//
// Total variation: sum over the three spatial axes of mean squared forward differences, per-workgroup partial sums added by one
// workgroup in a fixed order in double (no float atomics; the shape of gsx_photometric_fwd's reduction).
#include "common.hpp"

namespace gsx {

constexpr int kBgThreads = 256;
constexpr int kBgCell = 48; // floats per guidance level of one cell: 2 x 2 corners x 12 channels

struct BgArgs {
    const float *grids;   // [N, 12, L, Hg, Wg]
    int32_t N, L, Hg, Wg;
    const float *rgb;     // [I, H, W, 3] through srgb
    int64_t srgb[4];
    const float *xy;      // [I, H, W, 2] through sxy, or null = pixel centres ((x + 0.5) / W, (y + 0.5) / H)
    int64_t sxy[4];
    const int64_t *idx;   // [I] grid of each image
    int32_t I, H, W;
    float *rgb_out;       // fwd: [I, H, W, 3] contiguous
    float *mats;          // fwd: [I, H, W, 12] contiguous or null
    const float *v_out;   // bwd: [I, H, W, 3] through sv
    int64_t sv[4];
    float *v_rgb;         // bwd: [I, H, W, 3] contiguous, or null
    float *v_grids;       // bwd: [N, 12, L, Hg, Wg], accumulated into, or null
    int32_t ncx, ncy, splits, replicas; // bwd, cell-owner kernel
};

// continuous index along one axis of `size` cells for a coordinate n in [-1, 1], as grid_sample takes it
struct BgAxis {
    int i0;   // floor of the clamped index
    float f;  // fraction
    float gm; // d index / d coordinate-in-[0, 1]: size - 1, or 0 where the index was clamped
};

__device__ __forceinline__ BgAxis bg_axis(float n, int size)
{
    const float m = (float)(size - 1);
    float t = ((n + 1.0f) * 0.5f) * m;
    BgAxis a;
    a.gm = m;
    if (!(t > 0.0f)) { t = 0.0f; a.gm = 0.0f; } // also NaN: stays inside the grid
    else if (t >= m) { t = m; a.gm = 0.0f; }
    const float fl = floorf(t);
    a.i0 = (int)fl;
    a.f = t - fl;
    return a;
}

struct BgPixel {
    float r, g, b;
    BgAxis ax, ay, az;
};

template <bool HAS_XY>
__device__ __forceinline__ BgPixel bg_pixel(const BgArgs &a, int i, int y, int x)
{
    BgPixel p;
    const float *c = a.rgb + i * a.srgb[0] + y * a.srgb[1] + x * a.srgb[2];
    p.r = c[0]; p.g = c[a.srgb[3]]; p.b = c[2 * a.srgb[3]];
    float u, v;
    if constexpr (HAS_XY) {
        const float *q = a.xy + i * a.sxy[0] + y * a.sxy[1] + x * a.sxy[2];
        u = q[0]; v = q[a.sxy[3]];
    } else {
        u = ((float)x + 0.5f) / (float)a.W;
        v = ((float)y + 0.5f) / (float)a.H;
    }
    const float gray = p.r * 0.299f + p.g * 0.587f + p.b * 0.114f;
    p.ax = bg_axis((u - 0.5f) * 2.0f, a.Wg);
    p.ay = bg_axis((v - 0.5f) * 2.0f, a.Hg);
    p.az = bg_axis(gray * 2.0f - 1.0f, a.L);
    return p;
}

// grid values and gradient sums as the backward sees them: straight in global memory ...
struct BgGlobalGrid {
    const float *g; // this image's grid
    float *vg;      // its gradient
    int64_t chan, sz, sy; // strides of (channel, z, y)
    __device__ __forceinline__ int64_t at(int z, int y, int x) const { return z * sz + y * sy + x; }
    __device__ __forceinline__ float load(int64_t o, int c) const { return g[o + c * chan]; }
    __device__ __forceinline__ void add(int64_t o, int c, float v) const
    {
        if (vg) atomic_add_f32(vg + o + c * chan, v); // uniform: null = the grids' gradient is not wanted
    }
};

// ... or one cell's 2 x 2 x L corners in LDS (values: [z][yc][xc][12]; sums: the same index times R + replica)
struct BgCellGrid {
    const float *g;
    float *acc;
    int cx, cy, R, rep;
    __device__ __forceinline__ int at(int z, int y, int x) const { return ((z * 2 + (y - cy)) * 2 + (x - cx)) * 12; }
    __device__ __forceinline__ float load(int o, int c) const { return g[o + c]; }
    __device__ __forceinline__ void add(int o, int c, float v) const
    {
        if (acc) atomicAdd(acc + (o + c) * R + rep, v); // uniform: null = the grids' gradient is not wanted
    }
};

// One pixel of the backward: adds its share of v_grids through G and returns v_rgb in (vr, vg, vb).
template <class G>
__device__ __forceinline__ void bg_pixel_bwd(const BgArgs &a, const BgPixel &p, const G &grid, float o0, float o1, float o2,
                                             float &vr, float &vg, float &vb)
{
    // d L / d A[i][j]
    const float vo[3] = {o0, o1, o2};
    const float in[4] = {p.r, p.g, p.b, 1.0f};
    float vA[12];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) vA[i * 4 + j] = vo[i] * in[j];
    float A[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) A[c] = 0.0f;
    float giz = 0.0f; // d L / d iz
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        const int z = p.az.i0 + dz;
        if (z >= a.L) continue;
        const float wz = dz ? p.az.f : 1.0f - p.az.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = p.ay.i0 + dy;
            if (y >= a.Hg) continue;
            const float wy = dy ? p.ay.f : 1.0f - p.ay.f;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int x = p.ax.i0 + dx;
                if (x >= a.Wg) continue;
                const float wxy = (dx ? p.ax.f : 1.0f - p.ax.f) * wy, w = wxy * wz;
                const auto o = grid.at(z, y, x);
                float dot = 0.0f;
#pragma unroll
                for (int c = 0; c < 12; ++c) {
                    const float gv = grid.load(o, c);
                    A[c] += w * gv;
                    dot += gv * vA[c];
                    grid.add(o, c, w * vA[c]);
                }
                giz += (dz ? wxy : -wxy) * dot;
            }
        }
    }
    const float dgray = giz * p.az.gm; // iz = gray (L - 1) where not clamped
    vr = A[0] * o0 + A[4] * o1 + A[8] * o2 + dgray * 0.299f;
    vg = A[1] * o0 + A[5] * o1 + A[9] * o2 + dgray * 0.587f;
    vb = A[2] * o0 + A[6] * o1 + A[10] * o2 + dgray * 0.114f;
}

template <bool HAS_XY>
__global__ void __launch_bounds__(kBgThreads) bilagrid_fwd_kernel(const BgArgs a)
{
    const int64_t n = (int64_t)a.I * a.H * a.W, q = (int64_t)blockIdx.x * kBgThreads + threadIdx.x;
    if (q >= n) return;
    const int x = (int)(q % a.W), y = (int)((q / a.W) % a.H), i = (int)(q / ((int64_t)a.W * a.H));
    const int64_t gi = a.idx[i];
    float A[12];
    if (gi < 0 || gi >= a.N) { // no such grid: a result nobody can mistake for one, and no read outside the tensor
#pragma unroll
        for (int c = 0; c < 12; ++c) A[c] = __builtin_nanf("");
        if (a.mats)
#pragma unroll
            for (int c = 0; c < 12; ++c) a.mats[q * 12 + c] = A[c];
        a.rgb_out[q * 3] = a.rgb_out[q * 3 + 1] = a.rgb_out[q * 3 + 2] = A[0];
        return;
    }
    const BgPixel p = bg_pixel<HAS_XY>(a, i, y, x);
    const int64_t sy = a.Wg, sz = (int64_t)a.Hg * a.Wg, chan = sz * a.L;
    const float *g = a.grids + gi * 12 * chan;
#pragma unroll
    for (int c = 0; c < 12; ++c) A[c] = 0.0f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz) {
        const int zz = p.az.i0 + dz;
        if (zz >= a.L) continue;
        const float wz = dz ? p.az.f : 1.0f - p.az.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int yy = p.ay.i0 + dy;
            if (yy >= a.Hg) continue;
            const float wy = dy ? p.ay.f : 1.0f - p.ay.f;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int xx = p.ax.i0 + dx;
                if (xx >= a.Wg) continue;
                const float w = (dx ? p.ax.f : 1.0f - p.ax.f) * wy * wz;
                const float *gc = g + zz * sz + yy * sy + xx;
#pragma unroll
                for (int c = 0; c < 12; ++c) A[c] += w * gc[c * chan];
            }
        }
    }
    if (a.mats)
#pragma unroll
        for (int c = 0; c < 12; ++c) a.mats[q * 12 + c] = A[c];
    a.rgb_out[q * 3 + 0] = A[0] * p.r + A[1] * p.g + A[2] * p.b + A[3];
    a.rgb_out[q * 3 + 1] = A[4] * p.r + A[5] * p.g + A[6] * p.b + A[7];
    a.rgb_out[q * 3 + 2] = A[8] * p.r + A[9] * p.g + A[10] * p.b + A[11];
}

// The simpler accumulation: one thread per pixel, one global atomic per (corner, channel).
template <bool HAS_XY>
__global__ void __launch_bounds__(kBgThreads) bilagrid_bwd_scatter_kernel(const BgArgs a)
{
    const int64_t n = (int64_t)a.I * a.H * a.W, q = (int64_t)blockIdx.x * kBgThreads + threadIdx.x;
    if (q >= n) return;
    const int x = (int)(q % a.W), y = (int)((q / a.W) % a.H), i = (int)(q / ((int64_t)a.W * a.H));
    const int64_t gi = a.idx[i];
    float vr = 0.0f, vg = 0.0f, vb = 0.0f;
    if (gi >= 0 && gi < a.N) {
        const BgPixel p = bg_pixel<HAS_XY>(a, i, y, x);
        BgGlobalGrid grid;
        grid.sy = a.Wg; grid.sz = (int64_t)a.Hg * a.Wg; grid.chan = grid.sz * a.L;
        grid.g = a.grids + gi * 12 * grid.chan;
        grid.vg = a.v_grids ? a.v_grids + gi * 12 * grid.chan : nullptr;
        const float *vo = a.v_out + i * a.sv[0] + y * a.sv[1] + x * a.sv[2];
        bg_pixel_bwd(a, p, grid, vo[0], vo[a.sv[3]], vo[2 * a.sv[3]], vr, vg, vb);
    }
    if (a.v_rgb) { a.v_rgb[q * 3] = vr; a.v_rgb[q * 3 + 1] = vg; a.v_rgb[q * 3 + 2] = vb; }
}

// The pixel range [lo, hi) that certainly holds every pixel centre whose index along an axis of `ncell` cells floors to
// `cell`: the exact range, two pixels wider on each side (the float index of a pixel is off by far less than that).
__device__ __forceinline__ void bg_cell_range(int cell, int ncell, int npix, int &lo, int &hi)
{
    lo = cell == 0 ? 0 : max(0, (int)(((int64_t)cell * npix) / ncell) - 2);
    hi = cell == ncell - 1 ? npix : min(npix, (int)(((int64_t)(cell + 1) * npix + ncell - 1) / ncell) + 2);
}

// Pixel-centre coordinates: blockIdx.x = ((image * ncy + cy) * ncx + cx) * splits + split.
__global__ void __launch_bounds__(kBgThreads) bilagrid_bwd_cell_kernel(const BgArgs a)
{
    extern __shared__ float s_bg[];
    const int R = a.replicas, nacc = a.L * kBgCell;
    float *s_grid = s_bg, *s_acc = s_bg + nacc;
    int b = blockIdx.x;
    const int split = b % a.splits; b /= a.splits;
    const int cx = b % a.ncx; b /= a.ncx;
    const int cy = b % a.ncy;
    const int i = b / a.ncy;
    int xlo, xhi, ylo, yhi;
    bg_cell_range(cx, a.ncx, a.W, xlo, xhi);
    bg_cell_range(cy, a.ncy, a.H, ylo, yhi);
    const int rows = (yhi - ylo + a.splits - 1) / a.splits;
    ylo += split * rows;
    yhi = min(yhi, ylo + rows);
    const int rw = xhi - xlo, npix = rw * max(yhi - ylo, 0);
    const int64_t gi = a.idx[i];
    const bool valid = gi >= 0 && gi < a.N; // workgroup-uniform
    const int64_t sy = a.Wg, sz = (int64_t)a.Hg * a.Wg, chan = sz * a.L;
    if (valid) {
        const float *g = a.grids + gi * 12 * chan;
        for (int k = threadIdx.x; k < nacc; k += kBgThreads) {
            const int c = k % 12, xc = (k / 12) % 2, yc = (k / 24) % 2, z = k / kBgCell;
            const int gx = cx + xc, gy = cy + yc;
            s_grid[k] = gx < a.Wg && gy < a.Hg ? g[c * chan + z * sz + gy * sy + gx] : 0.0f;
        }
        if (a.v_grids)
            for (int k = threadIdx.x; k < nacc * R; k += kBgThreads) s_acc[k] = 0.0f;
    }
    __syncthreads();
    BgCellGrid grid;
    grid.g = s_grid; grid.acc = a.v_grids ? s_acc : nullptr; grid.cx = cx; grid.cy = cy; grid.R = R; grid.rep = (int)threadIdx.x & (R - 1);
    for (int q = threadIdx.x; q < npix; q += kBgThreads) {
        const int x = xlo + q % rw, y = ylo + q / rw;
        float vr = 0.0f, vg = 0.0f, vb = 0.0f;
        const int64_t o = (((int64_t)i * a.H + y) * a.W + x) * 3;
        if (valid) {
            const BgPixel p = bg_pixel<false>(a, i, y, x);
            if (min(p.ax.i0, a.ncx - 1) != cx || min(p.ay.i0, a.ncy - 1) != cy) continue; // a neighbouring cell's pixel
            const float *vo = a.v_out + i * a.sv[0] + y * a.sv[1] + x * a.sv[2];
            bg_pixel_bwd(a, p, grid, vo[0], vo[a.sv[3]], vo[2 * a.sv[3]], vr, vg, vb);
        } else {
            // no grid, no gradient; the pixel still has exactly one owner: the cell its coordinates name
            const BgPixel p = bg_pixel<false>(a, i, y, x);
            if (min(p.ax.i0, a.ncx - 1) != cx || min(p.ay.i0, a.ncy - 1) != cy) continue;
        }
        if (a.v_rgb) { a.v_rgb[o] = vr; a.v_rgb[o + 1] = vg; a.v_rgb[o + 2] = vb; }
    }
    if (!valid || !a.v_grids) return;
    __syncthreads();
    float *vgr = a.v_grids + gi * 12 * chan;
    for (int k = threadIdx.x; k < nacc; k += kBgThreads) {
        float t = 0.0f;
        for (int r = 0; r < R; ++r) t += s_acc[k * R + ((r + k) & (R - 1))]; // rotated: neighbouring lanes start at different replicas
        const int c = k % 12, xc = (k / 12) % 2, yc = (k / 24) % 2, z = k / kBgCell;
        const int gx = cx + xc, gy = cy + yc;
        if (t != 0.0f && gx < a.Wg && gy < a.Hg) atomic_add_f32(vgr + c * chan + z * sz + gy * sy + gx, t);
    }
}

// ---- total variation of x [B, C, D1, D2, D3] ---------------------------------------------------------------------------
struct TvArgs {
    const float *x;
    int32_t C, D1, D2, D3;
    int64_t n;       // B C D1 D2 D3
    float w1, w2, w3; // 1 / (B * element count of the differenced tensor without its batch axis), per axis
};

constexpr int kTvThreads = 256, kTvPerThread = 4, kTvMaxBlocks = 2048;

__global__ void __launch_bounds__(kTvThreads) tv_partial_kernel(const TvArgs a, float *partial)
{
    __shared__ float s_red[kTvThreads / kWave];
    const int64_t s2 = a.D3, s1 = (int64_t)a.D2 * a.D3;
    float acc = 0.0f;
    for (int64_t e = (int64_t)blockIdx.x * kTvThreads + threadIdx.x; e < a.n; e += (int64_t)gridDim.x * kTvThreads) {
        const int i3 = (int)(e % a.D3), i2 = (int)((e / s2) % a.D2), i1 = (int)((e / s1) % a.D1);
        const float v = a.x[e];
        if (i1 + 1 < a.D1) { const float d = a.x[e + s1] - v; acc += a.w1 * d * d; }
        if (i2 + 1 < a.D2) { const float d = a.x[e + s2] - v; acc += a.w2 * d * d; }
        if (i3 + 1 < a.D3) { const float d = a.x[e + 1] - v; acc += a.w3 * d * d; }
    }
    acc = wave_sum(acc);
    if (lane_id() == 0) s_red[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int w = 0; w < kTvThreads / kWave; ++w) t += s_red[w];
        partial[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(kTvThreads) tv_finish_kernel(const float *partial, int n_blocks, float *out)
{
    __shared__ double s[kTvThreads];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += kTvThreads) acc += (double)partial[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int o = kTvThreads / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)s[0];
}

__global__ void __launch_bounds__(kTvThreads) tv_bwd_kernel(const TvArgs a, const float *grad, float *v_x)
{
    const int64_t e = (int64_t)blockIdx.x * kTvThreads + threadIdx.x;
    if (e >= a.n) return;
    const int64_t s2 = a.D3, s1 = (int64_t)a.D2 * a.D3;
    const int i3 = (int)(e % a.D3), i2 = (int)((e / s2) % a.D2), i1 = (int)((e / s1) % a.D1);
    const float v = a.x[e];
    float t = 0.0f;
    if (i1 > 0) t += a.w1 * (v - a.x[e - s1]);
    if (i1 + 1 < a.D1) t -= a.w1 * (a.x[e + s1] - v);
    if (i2 > 0) t += a.w2 * (v - a.x[e - s2]);
    if (i2 + 1 < a.D2) t -= a.w2 * (a.x[e + s2] - v);
    if (i3 > 0) t += a.w3 * (v - a.x[e - 1]);
    if (i3 + 1 < a.D3) t -= a.w3 * (a.x[e + 1] - v);
    v_x[e] = 2.0f * grad[0] * t;
}

} // namespace gsx

using namespace gsx;

static int bilagrid_args(const char *who, BgArgs &a, const float *grids, uint32_t N, uint32_t L, uint32_t Hg, uint32_t Wg,
                         const float *rgb, const int64_t *strides_rgb, const float *xy, const int64_t *strides_xy,
                         const int64_t *grid_idx, uint32_t I, uint32_t H, uint32_t W)
{
    GSX_REQUIRE(grids && rgb && strides_rgb && grid_idx, "%s: null argument", who);
    GSX_REQUIRE(!xy || strides_xy, "%s: xy needs its strides", who);
    GSX_REQUIRE(N > 0 && L > 0 && Hg > 0 && Wg > 0, "%s: empty grid [%u, 12, %u, %u, %u]", who, N, L, Hg, Wg);
    GSX_REQUIRE((int64_t)N * 12 * L * Hg * Wg < (int64_t)1 << 31 && L < 1u << 20 && Hg < 1u << 20 && Wg < 1u << 20,
                "%s: grid [%u, 12, %u, %u, %u] too large", who, N, L, Hg, Wg);
    GSX_REQUIRE((int64_t)I * H * W < (int64_t)1 << 31, "%s: more than 2^31 pixels", who);
    // the cell-owner backward widens each cell's pixel rectangle by two pixels for the rounding of (x + 0.5) / W * (Wg - 1)
    GSX_REQUIRE(H < 1u << 22 && W < 1u << 22, "%s: image side beyond 2^22 (%u x %u)", who, H, W);
    a.grids = grids; a.N = (int32_t)N; a.L = (int32_t)L; a.Hg = (int32_t)Hg; a.Wg = (int32_t)Wg;
    a.rgb = rgb; a.xy = xy; a.idx = grid_idx; a.I = (int32_t)I; a.H = (int32_t)H; a.W = (int32_t)W;
    for (int k = 0; k < 4; ++k) { a.srgb[k] = strides_rgb[k]; a.sxy[k] = xy ? strides_xy[k] : 0; }
    return GSX_OK;
}

extern "C" int gsx_bilagrid_slice_fwd(const float *grids, uint32_t N, uint32_t L, uint32_t Hg, uint32_t Wg, const float *rgb,
                                      const int64_t *strides_rgb, const float *xy, const int64_t *strides_xy,
                                      const int64_t *grid_idx, uint32_t I, uint32_t H, uint32_t W, float *rgb_out,
                                      float *affine_mats, void *stream)
{
    if ((int64_t)I * H * W == 0) return GSX_OK;
    BgArgs a{};
    if (int rc = bilagrid_args("gsx_bilagrid_slice_fwd", a, grids, N, L, Hg, Wg, rgb, strides_rgb, xy, strides_xy, grid_idx, I, H, W))
        return rc;
    GSX_REQUIRE(rgb_out, "gsx_bilagrid_slice_fwd: null argument");
    a.rgb_out = rgb_out; a.mats = affine_mats;
    const dim3 grid((unsigned)ceil_div((int64_t)I * H * W, kBgThreads));
    if (xy) bilagrid_fwd_kernel<true><<<grid, kBgThreads, 0, (hipStream_t)stream>>>(a);
    else bilagrid_fwd_kernel<false><<<grid, kBgThreads, 0, (hipStream_t)stream>>>(a);
    return check_launch("bilagrid_slice_fwd");
}

extern "C" int gsx_bilagrid_slice_bwd(const float *grids, uint32_t N, uint32_t L, uint32_t Hg, uint32_t Wg, const float *rgb,
                                      const int64_t *strides_rgb, const float *xy, const int64_t *strides_xy,
                                      const int64_t *grid_idx, uint32_t I, uint32_t H, uint32_t W, const float *v_rgb_out,
                                      const int64_t *strides_v, float *v_rgb, float *v_grids, void *stream)
{
    if ((int64_t)I * H * W == 0) return GSX_OK;
    BgArgs a{};
    if (int rc = bilagrid_args("gsx_bilagrid_slice_bwd", a, grids, N, L, Hg, Wg, rgb, strides_rgb, xy, strides_xy, grid_idx, I, H, W))
        return rc;
    GSX_REQUIRE(v_rgb_out && strides_v, "gsx_bilagrid_slice_bwd: null argument");
    if (!v_rgb && !v_grids) return GSX_OK;
    a.v_out = v_rgb_out; a.v_rgb = v_rgb; a.v_grids = v_grids;
    for (int k = 0; k < 4; ++k) a.sv[k] = strides_v[k];
    // replicas of the cell's accumulators: the most (a power of two, at most 32) that fit 64 KiB with the staged grid values
    int R = 32;
    while (R >= 1 && (int64_t)L * kBgCell * (R + 1) * 4 > 65536) R >>= 1;
    a.ncx = Wg > 1 ? (int32_t)Wg - 1 : 1;
    a.ncy = Hg > 1 ? (int32_t)Hg - 1 : 1;
    const int64_t cells = (int64_t)I * a.ncx * a.ncy;
    if (xy || R < 1 || cells * 8 >= (int64_t)1 << 31) {
        const dim3 grid((unsigned)ceil_div((int64_t)I * H * W, kBgThreads));
        if (xy) bilagrid_bwd_scatter_kernel<true><<<grid, kBgThreads, 0, (hipStream_t)stream>>>(a);
        else bilagrid_bwd_scatter_kernel<false><<<grid, kBgThreads, 0, (hipStream_t)stream>>>(a);
        return check_launch("bilagrid_slice_bwd (scatter)");
    }
    // bands of rows per cell: about 1024 workgroups for the 256 CUs where the cells allow it, at least ~4 rows each, at most 8
    // bands (every band pays the zeroing and the flush of its replicas). A choice by reasoning; other values were not timed.
    int64_t splits = ceil_div(1024, cells);
    const int64_t cell_rows = ceil_div(H, a.ncy);
    if (splits > ceil_div(cell_rows, 4)) splits = ceil_div(cell_rows, 4);
    if (splits < 1) splits = 1;
    if (splits > 8) splits = 8;
    a.splits = (int32_t)splits; a.replicas = R;
    const size_t lds = (size_t)L * kBgCell * (R + 1) * 4;
    bilagrid_bwd_cell_kernel<<<dim3((unsigned)(cells * splits)), kBgThreads, lds, (hipStream_t)stream>>>(a);
    return check_launch("bilagrid_slice_bwd");
}

static int tv_args(const char *who, TvArgs &a, const float *x, uint32_t B, uint32_t C, uint32_t D1, uint32_t D2, uint32_t D3)
{
    GSX_REQUIRE(x, "%s: null argument", who);
    GSX_REQUIRE(D1 < 1u << 30 && D2 < 1u << 30 && D3 < 1u << 30 && C < 1u << 30, "%s: dimension too large", who);
    a.x = x; a.C = (int32_t)C; a.D1 = (int32_t)D1; a.D2 = (int32_t)D2; a.D3 = (int32_t)D3;
    a.n = (int64_t)B * C * D1 * D2 * D3;
    auto weight = [&](double d1, double d2, double d3) {
        const double count = (double)C * d1 * d2 * d3;
        return (float)(1.0 / ((count > 1.0 ? count : 1.0) * (double)B));
    };
    a.w1 = weight((double)D1 - 1, D2, D3); a.w2 = weight(D1, (double)D2 - 1, D3); a.w3 = weight(D1, D2, (double)D3 - 1);
    return GSX_OK;
}

extern "C" int64_t gsx_tv_blocks(uint32_t B, uint32_t C, uint32_t D1, uint32_t D2, uint32_t D3)
{
    const int64_t n = (int64_t)B * C * D1 * D2 * D3, blocks = ceil_div(n, (int64_t)kTvThreads * kTvPerThread);
    return blocks < 1 ? 1 : (blocks > kTvMaxBlocks ? kTvMaxBlocks : blocks);
}

extern "C" int gsx_tv_fwd(const float *x, uint32_t B, uint32_t C, uint32_t D1, uint32_t D2, uint32_t D3, float *partial_sums,
                          float *loss, void *stream)
{
    GSX_REQUIRE(partial_sums && loss, "gsx_tv_fwd: null argument");
    TvArgs a{};
    if ((int64_t)B * C * D1 * D2 * D3 == 0) {
        tv_finish_kernel<<<1, kTvThreads, 0, (hipStream_t)stream>>>(partial_sums, 0, loss);
        return check_launch("tv_finish");
    }
    if (int rc = tv_args("gsx_tv_fwd", a, x, B, C, D1, D2, D3)) return rc;
    const int blocks = (int)gsx_tv_blocks(B, C, D1, D2, D3);
    tv_partial_kernel<<<blocks, kTvThreads, 0, (hipStream_t)stream>>>(a, partial_sums);
    if (int rc = check_launch("tv_fwd")) return rc;
    tv_finish_kernel<<<1, kTvThreads, 0, (hipStream_t)stream>>>(partial_sums, blocks, loss);
    return check_launch("tv_finish");
}

extern "C" int gsx_tv_bwd(const float *x, uint32_t B, uint32_t C, uint32_t D1, uint32_t D2, uint32_t D3, const float *grad_device,
                          float *v_x, void *stream)
{
    if ((int64_t)B * C * D1 * D2 * D3 == 0) return GSX_OK;
    GSX_REQUIRE(grad_device && v_x, "gsx_tv_bwd: null argument");
    TvArgs a{};
    if (int rc = tv_args("gsx_tv_bwd", a, x, B, C, D1, D2, D3)) return rc;
    tv_bwd_kernel<<<dim3((unsigned)ceil_div(a.n, kTvThreads)), kTvThreads, 0, (hipStream_t)stream>>>(a, grad_device, v_x);
    return check_launch("tv_bwd");
}
