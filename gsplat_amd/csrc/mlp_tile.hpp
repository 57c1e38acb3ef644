// Device helpers shared by the fused narrow MLPs over the Gaussians (appearance.hip, deformation.hip): 64 hidden units, products
// on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: a chain of fmaf, exact fp32), a wave owning a tile of 32 Gaussians.
//
// Everything is kept TRANSPOSED: the Gaussian is the column of every accumulator tile (the lane, l & 31) and the unit is its row
// (register r of lane half h = l >> 5 holds row (r & 3) + 8 (r >> 2) + 4 h), so that Z^T = W X^T and dX^T = W^T dZ^T sum over the
// ROW index of the previous result: register r of an accumulator tile is the B operand of one k step (lane half h supplies
// k = row(r, h)), and the matching A operand is the weight column of that k, read from LDS. A [64][64] weight matrix lives in LDS
// as [64][65]: with the odd stride the 32 lanes of a wave half hit 32 different banks in the row-wise and in the column-wise
// operand reads alike. Weight gradients sum over the Gaussians, the lane index, and take their operands through a wave-private
// LDS transposition ([unit][Gaussian], stride 33).
#pragma once
#include "common.hpp"

namespace gsx {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kApThreads = 256, kApWaves = 4;
constexpr int kApTile = 32;       // Gaussians per wave tile
constexpr int kApLd = 65;         // LDS row stride of the [64][64] weight matrices
constexpr int kApSt = 33;         // LDS row stride of a staged [64 units][32 Gaussians] tile
constexpr int kApStage = 2 * 64 * kApSt; // floats of one wave's two staged tiles (>= 64 * 64 for the final reduction)

#define AP_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

// row of register r in lane half h of a 32 x 32 accumulator tile
__device__ __forceinline__ constexpr int ap_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ v16f ap_zero()
{
    v16f v;
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = 0.0f;
    return v;
}

// lo in the lower half of the wave, hi in the upper one. Bit arithmetic, not `h ? hi : lo`: on two elements of a local array
// the compiler turns the conditional into one load at a lane-dependent index, which moves the whole array to scratch.
__device__ __forceinline__ float ap_pick(int h, float lo, float hi)
{
    const uint32_t m = 0u - (uint32_t)h;
    return __uint_as_float((__float_as_uint(lo) & ~m) | (__float_as_uint(hi) & m));
}

// d[i][g] += sum_k M(i, k) X[k][g] for X [64][32] held as two accumulator tiles (x0: rows 0-31, x1: rows 32-63) and
// M(i, k) = s_M[i * SI + k * SK]; `i` is this lane's row of the A operand (l & 31).
template <int SI, int SK>
__device__ __forceinline__ void ap_mm_acc(const float *s_M, int i, int h, const v16f &x0, const v16f &x1, v16f &d)
{
    const float *m = s_M + i * SI + 4 * h * SK;
#pragma unroll
    for (int r = 0; r < 16; ++r) d = AP_MFMA(m[ap_row(r, 0) * SK], x0[r], d);
#pragma unroll
    for (int r = 0; r < 16; ++r) d = AP_MFMA(m[(32 + ap_row(r, 0)) * SK], x1[r], d);
}

__device__ __forceinline__ void ap_relu(v16f &v)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = fmaxf(v[r], 0.0f);
}

// stage X [64 units][32 Gaussians] held as accumulator tiles into s[unit * 33 + Gaussian]
__device__ __forceinline__ void ap_stage(float *s, const v16f &x0, const v16f &x1, int g, int h)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        s[(ap_row(r, 0) + 4 * h) * kApSt + g] = x0[r];
        s[(32 + ap_row(r, 0) + 4 * h) * kApSt + g] = x1[r];
    }
}

// acc[2 tj + tk][j][k] += sum_g P[32 tj + j][g] Q[32 tk + k][g] for staged P, Q
__device__ __forceinline__ void ap_outer(const float *sP, const float *sQ, int i, int h, v16f (&acc)[4])
{
    const float *p0 = sP + i * kApSt + h, *p1 = p0 + 32 * kApSt, *q0 = sQ + i * kApSt + h, *q1 = q0 + 32 * kApSt;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const float a0 = p0[2 * s], a1 = p1[2 * s], b0 = q0[2 * s], b1 = q1[2 * s];
        acc[0] = AP_MFMA(a0, b0, acc[0]);
        acc[1] = AP_MFMA(a0, b1, acc[1]);
        acc[2] = AP_MFMA(a1, b0, acc[2]);
        acc[3] = AP_MFMA(a1, b1, acc[3]);
    }
}

// the four waves' 64 x 64 sums -> one partial of the workgroup (fixed order)
__device__ __forceinline__ void ap_reduce_big(float *s_stage, const v16f (&acc)[4], int wave, int g, int h, float *out)
{
    __syncthreads();
    float *mine = s_stage + wave * kApStage;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) mine[(32 * (t >> 1) + ap_row(r, 0) + 4 * h) * 64 + 32 * (t & 1) + g] = acc[t][r];
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 64; e += kApThreads)
        out[e] = ((s_stage[e] + s_stage[kApStage + e]) + s_stage[2 * kApStage + e]) + s_stage[3 * kApStage + e];
}

} // namespace gsx
