// Deformation network of the dynamic-scene trainer (examples/dynamic_surgical_trainer.py; semantics restated from
// gsplat/contrib/dynamic/deformation.py: DeformNetwork). C-ABI: gsx_deform_fwd / gsx_deform_bwd.
//
// One row is one Gaussian: h = relu(W3 relu(W2 relu(W1 x + b1) + b2) + b3) over its 64 plane features x, 64 hidden units per
// layer, and an 8-wide head d = Wh h + bh = [position 3 | quaternion 4 | opacity 1] that is added to (means, quats, opacities).
// The fused configuration only: float32, 64 features, width 64, three hidden layers. The caller joins the three heads into one
// [8][64] matrix.
//
// The scheme is appearance.hip's (helpers in mlp_tile.hpp): products on v_mfma_f32_32x32x2_f32, a wave owns 32 Gaussians, every
// tile transposed - Gaussian on the lane, unit in the accumulator registers - so each layer's accumulator tile is the next
// layer's B operand without crossing lanes. The features are loaded straight into that layout (lane half h reads the 16-byte
// pieces 8 q + 4 h of its row), so the first layer is the same [64][64] product as the others. The three weight matrices sit in
// LDS as [64][65]; the head (8 outputs) and its transpose are VALU work on the accumulator layout, halves joined by one
// cross-lane add.
//
// Backward (recomputes the forward; nothing of size [N, 64] but v_x is written to memory): per tile, from the head down,
// dZ3 = (Wh^T dOut) where H3 > 0, dZ2 = (W3^T dZ3) where H2 > 0, dZ1 = (W2^T dZ2) where H1 > 0, dX = W1^T dZ1. The weight gradients
// v_W3 = dZ3^T H2, v_W2 = dZ2^T H1, v_W1 = dZ1^T X sum over the Gaussians, the lane index: both operands go through the
// wave-private LDS transposition and the sums stay in 3 x 4 accumulator tiles per wave for the whole kernel (192 registers; at
// most four pairs of tiles are live beside them: X is read again where v_W1 needs it, and once H2 and H1 are staged only their
// > 0 decisions are kept, as one 32-bit mask each). v_b1..3, v_Wh and v_bh are row sums of the staged
// tiles: lane l adds the 32 Gaussians of unit l, in order. A null cotangent counts as zeros. With zero heads dZ3 is exactly
// zero, and so is every sum that it feeds.
// No float atomics: a persistent grid; each wave writes its small sums to a slot of its own, each workgroup adds its four waves'
// weight-gradient tiles in LDS in a fixed order and writes one partial; deform_finish_kernel adds the partials in a fixed order
// (in double). Waves without rows write zeros. Two runs give the same bits.
#include "common.hpp"
#include "mlp_tile.hpp"

namespace gsx {

constexpr int kDfMaxBlocks = 256; // persistent backward grid: one workgroup per CU (the forward fits three)
constexpr int kDfWeights = 3 * 64 * kApLd + 8 * 64 + 3 * 64 + 8; // W1, W2, W3, Wh, b1..3, bh
constexpr int kDfSmall = 3 * 64 + 8 * 64 + 8; // a wave's slot: v_b1 [64] | v_b2 [64] | v_b3 [64] | v_Wh [8][64] | v_bh [8]
constexpr int kDfBig = 3 * 64 * 64;           // a workgroup's partial: v_W1 | v_W2 | v_W3
constexpr int kDfParts = 8;                   // the finish kernel cuts the list of partials into this many runs per element

struct DfArgs {
    const float *x;                     // [N, 64] contiguous, 16-byte aligned
    const float *means, *quats, *opac;  // fwd: [N, 3], [N, 4], [N, 1] contiguous
    const float *W1, *b1, *W2, *b2, *W3, *b3, *Wh, *bh;
    int64_t N, ntiles;
    float *means_out, *quats_out, *opac_out;   // fwd
    const float *v_means, *v_quats, *v_opac;   // bwd: the cotangents, contiguous; each may be null (zeros)
    float *v_x;                                // bwd: [N, 64] or null (not wanted)
    float *part_big;                           // bwd: [blocks][kDfBig]
    float *part_small;                         // bwd: [blocks * 4][kDfSmall]
};

struct DfLds {
    float *W1, *W2, *W3, *Wh, *b, *bh;
};

__device__ __forceinline__ DfLds df_load_weights(const DfArgs &a, float *s)
{
    DfLds w;
    w.W1 = s; w.W2 = w.W1 + 64 * kApLd; w.W3 = w.W2 + 64 * kApLd; w.Wh = w.W3 + 64 * kApLd; w.b = w.Wh + 8 * 64; w.bh = w.b + 3 * 64;
    for (int e = threadIdx.x; e < 64 * 64; e += kApThreads) {
        const int o = (e >> 6) * kApLd + (e & 63);
        w.W1[o] = a.W1[e];
        w.W2[o] = a.W2[e];
        w.W3[o] = a.W3[e];
    }
    for (int e = threadIdx.x; e < 8 * 64; e += kApThreads) w.Wh[e] = a.Wh[e];
    for (int e = threadIdx.x; e < 64; e += kApThreads) { w.b[e] = a.b1[e]; w.b[64 + e] = a.b2[e]; w.b[128 + e] = a.b3[e]; }
    if (threadIdx.x < 8) w.bh[threadIdx.x] = a.bh[threadIdx.x];
    __syncthreads();
    return w;
}

// Top of a tile's work. The weights in LDS do not change between tiles, and left alone the compiler lifts their operand reads out
// of the tile loop: several hundred registers, which it then spills to scratch. Past this point it has to read them again.
__device__ __forceinline__ void df_tile_begin() { asm volatile("" ::: "memory"); }

// X^T of this wave's 32 Gaussians in the accumulator layout: register 4 q + j of lane half h is feature 8 q + 4 h + j (x0) and
// 32 + 8 q + 4 h + j (x1). A row past N is zeros.
__device__ __forceinline__ void df_load_x(const float *x, int64_t n, bool valid, int h, v16f &x0, v16f &x1)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v4f u = {0.0f, 0.0f, 0.0f, 0.0f}, v = u;
        if (valid) {
            u = *reinterpret_cast<const v4f *>(x + n * 64 + 8 * q + 4 * h);
            v = *reinterpret_cast<const v4f *>(x + n * 64 + 32 + 8 * q + 4 * h);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { x0[4 * q + j] = u[j]; x1[4 * q + j] = v[j]; }
    }
}

// Y^T = relu(W X^T + b)
__device__ __forceinline__ void df_layer(const float *s_W, const float *s_b, int g, int h, const v16f &x0, const v16f &x1, v16f &y0,
                                         v16f &y1)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const v4f b0 = *reinterpret_cast<const v4f *>(s_b + 8 * q + 4 * h);
        const v4f b1 = *reinterpret_cast<const v4f *>(s_b + 32 + 8 * q + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) { y0[4 * q + j] = b0[j]; y1[4 * q + j] = b1[j]; }
    }
    ap_mm_acc<kApLd, 1>(s_W, g, h, x0, x1, y0);
    ap_mm_acc<kApLd, 1>(s_W + 32 * kApLd, g, h, x0, x1, y1);
    ap_relu(y0);
    ap_relu(y1);
}

// where a layer's activation is positive: bit r for y0[r], bit 16 + r for y1[r]. One register instead of the two tiles, which
// are needed no longer once they are staged. Built and read by shifts alone, which need no constants held in registers.
__device__ __forceinline__ uint32_t df_positive(const v16f &y0, const v16f &y1)
{
    uint32_t m = 0;
#pragma unroll
    for (int r = 15; r >= 0; --r) m = (m << 1) | (y1[r] > 0.0f ? 1u : 0u);
#pragma unroll
    for (int r = 15; r >= 0; --r) m = (m << 1) | (y0[r] > 0.0f ? 1u : 0u);
    return m;
}

// dX^T = W^T dZ^T, kept where the layer's activation was positive
__device__ __forceinline__ void df_layer_t(const float *s_W, int g, int h, const v16f &z0, const v16f &z1, uint32_t positive,
                                           v16f &d0, v16f &d1)
{
    d0 = ap_zero();
    d1 = ap_zero();
    ap_mm_acc<1, kApLd>(s_W, g, h, z0, z1, d0);
    ap_mm_acc<1, kApLd>(s_W + 32, g, h, z0, z1, d1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        d0[r] = (int32_t)(positive << (31 - r)) < 0 ? d0[r] : 0.0f;
        d1[r] = (int32_t)(positive << (15 - r)) < 0 ? d1[r] : 0.0f;
    }
}

// the sum over the 32 Gaussians of unit `lane` of a staged tile
__device__ __forceinline__ float df_row_sum(const float *sP, int lane)
{
    const float *row = sP + lane * kApSt;
    float t = 0.0f;
#pragma unroll 4
    for (int k = 0; k < kApTile; ++k) t += row[k];
    return t;
}

__global__ void __launch_bounds__(kApThreads) deform_fwd_kernel(const DfArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_w[kDfWeights];
    const DfLds w = df_load_weights(a, s_w);
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), g = lane & 31, h = lane >> 5;
    for (int64_t tile = (int64_t)blockIdx.x * kApWaves + wave; tile < a.ntiles; tile += (int64_t)gridDim.x * kApWaves) {
        const int64_t n = tile * kApTile + g;
        const bool valid = n < a.N;
        df_tile_begin();
        v16f x0, x1, h10, h11, h20, h21;
        df_load_x(a.x, n, valid, h, x0, x1);
        df_layer(w.W1, w.b, g, h, x0, x1, h10, h11);
        df_layer(w.W2, w.b + 64, g, h, h10, h11, h20, h21);
        df_layer(w.W3, w.b + 128, g, h, h20, h21, h10, h11); // H3 in h10 / h11
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            o[k] = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4f w0 = *reinterpret_cast<const v4f *>(w.Wh + k * 64 + 8 * q + 4 * h);
                const v4f w1 = *reinterpret_cast<const v4f *>(w.Wh + k * 64 + 32 + 8 * q + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[k] += w0[j] * h10[4 * q + j] + w1[j] * h11[4 * q + j];
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (o[k] + __shfl_xor(o[k], 32)) + w.bh[k];
        if (valid) {
            if (h == 0) { // the lower half writes the means, the upper one the quaternions and the opacity
                const float *p = a.means + n * 3;
                float *q = a.means_out + n * 3;
                q[0] = p[0] + o[0]; q[1] = p[1] + o[1]; q[2] = p[2] + o[2];
            } else {
                const float *p = a.quats + n * 4;
                float *q = a.quats_out + n * 4;
                q[0] = p[0] + o[3]; q[1] = p[1] + o[4]; q[2] = p[2] + o[5]; q[3] = p[3] + o[6];
                a.opac_out[n] = a.opac[n] + o[7];
            }
        }
    }
}

template <bool WANT_X>
__global__ void __launch_bounds__(kApThreads) deform_bwd_kernel(const DfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_df[];
    const DfLds w = df_load_weights(a, s_df);
    float *s_stage = s_df + kDfWeights;
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), g = lane & 31, h = lane >> 5;
    float *sP = s_stage + wave * kApStage, *sQ = sP + 64 * kApSt;
    v16f accW1[4], accW2[4], accW3[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { accW1[t] = ap_zero(); accW2[t] = ap_zero(); accW3[t] = ap_zero(); }
    // lane l owns unit l of the sums over a tile's Gaussians, which it takes row-wise from the staged [unit][Gaussian] tiles
    // (and lane k < 8 output k of the head's bias)
    float vb1 = 0.0f, vb2 = 0.0f, vb3 = 0.0f, vbh = 0.0f, vWh[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) vWh[k] = 0.0f;

    for (int64_t tile = (int64_t)blockIdx.x * kApWaves + wave; tile < a.ntiles; tile += (int64_t)gridDim.x * kApWaves) {
        const int64_t n = tile * kApTile + g;
        const bool valid = n < a.N;
        df_tile_begin();
        v16f x0, x1, h10, h11, h20, h21, h30, h31;
        df_load_x(a.x, n, valid, h, x0, x1);
        df_layer(w.W1, w.b, g, h, x0, x1, h10, h11);
        df_layer(w.W2, w.b + 64, g, h, h10, h11, h20, h21);
        df_layer(w.W3, w.b + 128, g, h, h20, h21, h30, h31);
        float vo[8]; // a row past N and a missing cotangent contribute nothing to any sum
#pragma unroll
        for (int k = 0; k < 8; ++k) vo[k] = 0.0f;
        if (valid) {
            if (a.v_means) { vo[0] = a.v_means[n * 3]; vo[1] = a.v_means[n * 3 + 1]; vo[2] = a.v_means[n * 3 + 2]; }
            if (a.v_quats) { vo[3] = a.v_quats[n * 4]; vo[4] = a.v_quats[n * 4 + 1]; vo[5] = a.v_quats[n * 4 + 2]; vo[6] = a.v_quats[n * 4 + 3]; }
            if (a.v_opac) vo[7] = a.v_opac[n];
        }
        // the head backwards. v_Wh[k][j] = sum_g dOut[g][k] H3[g][j] and v_bh: from H3 and dOut staged
        ap_stage(sP, h30, h31, g, h);
        if (h == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) sQ[k * kApSt + g] = vo[k];
        }
        wave_lds_sync();
        {
            const float *row = sP + lane * kApSt;
            float ws[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) ws[k] = 0.0f;
#pragma unroll 4
            for (int i = 0; i < kApTile; ++i) {
                const float hv = row[i];
#pragma unroll
                for (int k = 0; k < 8; ++k) ws[k] += sQ[k * kApSt + i] * hv;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) vWh[k] += ws[k];
            vbh += df_row_sum(sQ, lane & 7);
        }
        // dZ3 (into h30 / h31)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v4f d0 = {0.0f, 0.0f, 0.0f, 0.0f}, d1 = d0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const v4f w0 = *reinterpret_cast<const v4f *>(w.Wh + k * 64 + 8 * q + 4 * h);
                const v4f w1 = *reinterpret_cast<const v4f *>(w.Wh + k * 64 + 32 + 8 * q + 4 * h);
                d0 += w0 * vo[k];
                d1 += w1 * vo[k];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                h30[4 * q + j] = h30[4 * q + j] > 0.0f ? d0[j] : 0.0f;
                h31[4 * q + j] = h31[4 * q + j] > 0.0f ? d1[j] : 0.0f;
            }
        }
        wave_lds_sync(); // the row sums above are done
        // v_W3 += dZ3^T H2, v_b3 += the row sums of dZ3^T
        ap_stage(sP, h30, h31, g, h);
        ap_stage(sQ, h20, h21, g, h);
        wave_lds_sync();
        const uint32_t pos2 = df_positive(h20, h21);
        vb3 += df_row_sum(sP, lane);
        ap_outer(sP, sQ, g, h, accW3);
        v16f d20, d21;
        df_layer_t(w.W3, g, h, h30, h31, pos2, d20, d21);
        wave_lds_sync(); // the reads of the v_W3 product are done
        // v_W2 += dZ2^T H1
        ap_stage(sP, d20, d21, g, h);
        ap_stage(sQ, h10, h11, g, h);
        wave_lds_sync();
        const uint32_t pos1 = df_positive(h10, h11);
        vb2 += df_row_sum(sP, lane);
        ap_outer(sP, sQ, g, h, accW2);
        df_layer_t(w.W2, g, h, d20, d21, pos1, h30, h31); // dZ1 in h30 / h31
        wave_lds_sync();
        // v_W1 += dZ1^T X
        ap_stage(sP, h30, h31, g, h);
        df_load_x(a.x, n, valid, h, x0, x1); // read again (a cache hit) rather than held in 32 registers through the tile
        ap_stage(sQ, x0, x1, g, h);
        wave_lds_sync();
        vb1 += df_row_sum(sP, lane);
        ap_outer(sP, sQ, g, h, accW1);
        if constexpr (WANT_X) {
            v16f dx0 = ap_zero(), dx1 = ap_zero();
            ap_mm_acc<1, kApLd>(w.W1, g, h, h30, h31, dx0);
            ap_mm_acc<1, kApLd>(w.W1 + 32, g, h, h30, h31, dx1);
            if (valid) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const v4f u = {dx0[4 * q], dx0[4 * q + 1], dx0[4 * q + 2], dx0[4 * q + 3]};
                    const v4f v = {dx1[4 * q], dx1[4 * q + 1], dx1[4 * q + 2], dx1[4 * q + 3]};
                    *reinterpret_cast<v4f *>(a.v_x + n * 64 + 8 * q + 4 * h) = u;
                    *reinterpret_cast<v4f *>(a.v_x + n * 64 + 32 + 8 * q + 4 * h) = v;
                }
            }
        }
        wave_lds_sync(); // the reads of the v_W1 product are done before the next tile stages
    }
    float *slot = a.part_small + ((int64_t)blockIdx.x * kApWaves + wave) * kDfSmall;
    slot[lane] = vb1;
    slot[64 + lane] = vb2;
    slot[128 + lane] = vb3;
#pragma unroll
    for (int k = 0; k < 8; ++k) slot[192 + k * 64 + lane] = vWh[k];
    if (lane < 8) slot[192 + 512 + lane] = vbh;
    float *big = a.part_big + (int64_t)blockIdx.x * kDfBig;
    ap_reduce_big(s_stage, accW1, wave, g, h, big);
    ap_reduce_big(s_stage, accW2, wave, g, h, big + 64 * 64);
    ap_reduce_big(s_stage, accW3, wave, g, h, big + 2 * 64 * 64);
}

// Sums of the partials in a fixed order: element e < kDfBig of (v_W1 | v_W2 | v_W3) over the workgroups, then the small vector
// over the wave slots. 32 elements per workgroup; each element's list is cut into kDfParts consecutive runs, one thread adds a
// run in order, then thread 0 of the element adds the runs in order (all in double).
__global__ void __launch_bounds__(32 * kDfParts) deform_finish_kernel(const float *part_big, int blocks, const float *part_small,
                                                                      float *v_big, float *v_small)
{
    __shared__ double s_run[kDfParts][32];
    const int e = (int)blockIdx.x * 32 + ((int)threadIdx.x & 31), p = (int)threadIdx.x >> 5;
    const bool big = e < kDfBig;
    const int k = big ? e : e - kDfBig;
    const bool live = big || k < kDfSmall;
    const float *src = big ? part_big : part_small;
    const int64_t stride = big ? kDfBig : kDfSmall;
    const int count = big ? blocks : blocks * kApWaves, run = (count + kDfParts - 1) / kDfParts;
    double t = 0.0;
    if (live) {
        const int end = min(count, (p + 1) * run);
        for (int b = p * run; b < end; ++b) t += (double)src[(int64_t)b * stride + k];
    }
    s_run[p][threadIdx.x & 31] = t;
    __syncthreads();
    if (p == 0 && live) {
        double s = s_run[0][threadIdx.x];
#pragma unroll
        for (int q = 1; q < kDfParts; ++q) s += s_run[q][threadIdx.x];
        (big ? v_big : v_small)[k] = (float)s;
    }
}

} // namespace gsx

using namespace gsx;

static int deform_args(const char *who, DfArgs &a, const float *plane_features, const float *W1, const float *b1, const float *W2,
                       const float *b2, const float *W3, const float *b3, const float *W_head, const float *b_head, int64_t N)
{
    GSX_REQUIRE(plane_features && W1 && b1 && W2 && b2 && W3 && b3 && W_head && b_head, "%s: null argument", who);
    GSX_REQUIRE(N > 0 && N < (int64_t)1 << 31, "%s: N %lld out of range", who, (long long)N);
    GSX_REQUIRE(((uintptr_t)plane_features & 15) == 0, "%s: plane_features not 16-byte aligned", who);
    a.x = plane_features; a.W1 = W1; a.b1 = b1; a.W2 = W2; a.b2 = b2; a.W3 = W3; a.b3 = b3; a.Wh = W_head; a.bh = b_head;
    a.N = N; a.ntiles = ceil_div(N, kApTile);
    return GSX_OK;
}

extern "C" int64_t gsx_deform_blocks(int64_t N)
{
    const int64_t blocks = ceil_div(ceil_div(N, kApTile), kApWaves);
    return blocks < 1 ? 1 : (blocks > kDfMaxBlocks ? kDfMaxBlocks : blocks);
}

extern "C" int64_t gsx_deform_bwd_workspace_floats(int64_t N)
{
    return gsx_deform_blocks(N) * (kDfBig + (int64_t)kApWaves * kDfSmall);
}

extern "C" int gsx_deform_fwd(const float *means, const float *quats, const float *opacities, const float *plane_features,
                              const float *W1, const float *b1, const float *W2, const float *b2, const float *W3, const float *b3,
                              const float *W_head, const float *b_head, int64_t N, float *means_out, float *quats_out,
                              float *opacities_out, void *stream)
{
    if (N == 0) return GSX_OK;
    DfArgs a{};
    if (int rc = deform_args("gsx_deform_fwd", a, plane_features, W1, b1, W2, b2, W3, b3, W_head, b_head, N)) return rc;
    GSX_REQUIRE(means && quats && opacities && means_out && quats_out && opacities_out, "gsx_deform_fwd: null argument");
    a.means = means; a.quats = quats; a.opac = opacities;
    a.means_out = means_out; a.quats_out = quats_out; a.opac_out = opacities_out;
    int64_t blocks = ceil_div(a.ntiles, kApWaves); // by its registers and LDS a CU holds three of these workgroups
    if (blocks > 3 * kDfMaxBlocks) blocks = 3 * kDfMaxBlocks;
    deform_fwd_kernel<<<dim3((unsigned)blocks), kApThreads, 0, (hipStream_t)stream>>>(a);
    return check_launch("deform_fwd");
}

extern "C" int gsx_deform_bwd(const float *plane_features, const float *W1, const float *b1, const float *W2, const float *b2,
                              const float *W3, const float *b3, const float *W_head, const float *b_head, int64_t N,
                              const float *v_means_out, const float *v_quats_out, const float *v_opacities_out, float *workspace,
                              float *v_plane_features, float *v_W, float *v_small, void *stream)
{
    if (N == 0) return GSX_OK;
    DfArgs a{};
    if (int rc = deform_args("gsx_deform_bwd", a, plane_features, W1, b1, W2, b2, W3, b3, W_head, b_head, N)) return rc;
    GSX_REQUIRE(workspace && v_W && v_small, "gsx_deform_bwd: null argument");
    GSX_REQUIRE(((uintptr_t)v_plane_features & 15) == 0, "gsx_deform_bwd: v_plane_features not 16-byte aligned");
    const int blocks = (int)gsx_deform_blocks(N);
    a.v_means = v_means_out; a.v_quats = v_quats_out; a.v_opac = v_opacities_out; a.v_x = v_plane_features;
    a.part_big = workspace; a.part_small = workspace + (int64_t)blocks * kDfBig;
    const size_t lds = (size_t)(kDfWeights + kApWaves * kApStage) * sizeof(float);
    // the dynamic-LDS limit is per device; a device counts as done only once both calls have succeeded (a racing thread sets
    // the same values again)
    static bool raised[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !raised[dev]) {
        if (hipFuncSetAttribute((const void *)deform_bwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess
            || hipFuncSetAttribute((const void *)deform_bwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            set_last_error("gsx_deform_bwd: cannot raise the dynamic LDS limit to %zu bytes", lds);
            return GSX_ERR_ARG;
        }
        if (dev >= 0 && dev < 64) raised[dev] = true;
    }
    if (v_plane_features) deform_bwd_kernel<true><<<dim3((unsigned)blocks), kApThreads, lds, (hipStream_t)stream>>>(a);
    else deform_bwd_kernel<false><<<dim3((unsigned)blocks), kApThreads, lds, (hipStream_t)stream>>>(a);
    if (int rc = check_launch("deform_bwd")) return rc;
    const int n_out = kDfBig + kDfSmall;
    deform_finish_kernel<<<dim3((unsigned)ceil_div(n_out, 32)), 32 * kDfParts, 0, (hipStream_t)stream>>>(
        a.part_big, blocks, a.part_small, v_W, v_small);
    return check_launch("deform_finish");
}
