// Per-Gaussian appearance MLP of the training step (examples/simple_trainer.py:477, 547-566, 673-681 with app_opt=True;
// semantics restated from examples/utils.py:66-129). C-ABI: gsx_appearance_fwd / gsx_appearance_bwd.
//
// One row is one (camera c, Gaussian n) pair: x = [embed[c] (E) | features[n] (32) | SH bases of normalize(dirs[c, n]) (16)],
// colors = W3 relu(W2 relu(W1 x + b1) + b2) + b3 with 64 hidden units. The fused configuration only: float32, width 64, depth 2,
// 32 features, module degree 3 (16 bases, those beyond the degree in use are zero), E in {0, 16}.
//
// The embedding part of layer 1 is the same for every row of a camera, so the caller folds it into a per-camera bias
// bias1[c] = b1 + W1[:, :E] embed[c] ([C, 64]) and layer 1 is a K = 48 product over [features | SH].
//
// Products run on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: a chain of fmaf, exact fp32). A wave owns a tile of 32
// Gaussians and loops over the cameras. Everything is kept TRANSPOSED: the Gaussian is the column of every accumulator tile (the
// lane, l & 31) and the unit is its row (register r of lane half h = l >> 5 holds row (r & 3) + 8 (r >> 2) + 4 h), so that
// Z1^T = W1 X^T, Z2^T = W2 H1^T, dH1^T = W2^T dZ2^T and dX^T = W1^T dZ1^T all sum over the ROW index of the previous result:
// register r of an accumulator tile is the B operand of one k step (lane half h supplies k = row(r, h)), and the matching A
// operand is the weight column of that k, read from LDS. No hidden activation crosses lanes, LDS or memory for these.
// The three weight matrices live in LDS as [64][65] (W1 with its columns reordered to [features | SH | embedding]): with the odd
// stride the 32 lanes of a wave half hit 32 different banks in the row-wise and in the column-wise operand reads alike; the two
// halves read addresses 4 rows or columns apart and can still meet in a bank (no bank-conflict counter was read).
// Layer 3 (3 outputs) and its transpose are VALU work on the accumulator layout, halves joined by one cross-lane add.
//
// Backward (recomputes the forward; nothing of size [C, N, 64] is written to memory): the weight gradients v_W2 = dZ2^T H1 and
// v_W1 = dZ1^T X sum over the Gaussians, the lane index, so these two products take their operands through a wave-private LDS
// transposition ([unit][Gaussian], stride 33) and accumulate in 2 x 2 tiles of 32 x 32 per wave for the whole kernel. X is staged
// with the camera's embedding in columns 48-63, so the embedding columns of v_W1 come out of the same product. v_features
// accumulates over the cameras in one accumulator tile and is stored once. v_b2, v_W3, v_b3 and the per-camera column sums of dZ1
// (v_b1's and v_embed's source) are row sums of the staged tiles: lane l adds the 32 Gaussians of unit l, in order.
// No float atomics: a persistent grid; each wave writes its small sums to a slot of its own, each workgroup adds its four waves'
// weight-gradient tiles in LDS in a fixed order and writes one partial; appearance_finish_kernel adds the partials in order
// (in double). Waves without rows write zeros. Two runs give the same bits.
// The tile helpers (accumulator row map, the [64][64] product, staging, the weight-gradient product and its workgroup sum) are
// mlp_tile.hpp's, shared with deformation.hip.
#include "common.hpp"
#include "mlp_tile.hpp"
#include "sh_math.hpp"

namespace gsx {

constexpr int kApSmall = 260;    // floats of a wave's slot before the per-camera sums: v_b2 [64] | v_W3 [3][64] | v_b3 [3] | pad
constexpr int kApMaxBlocks = 256; // persistent backward grid: one workgroup per CU
constexpr int kApWeights = 2 * 64 * kApLd + 3 * 64 + 64; // W1, W2, W3, b2

struct ApArgs {
    const float *features; // [N, 32] contiguous
    const float *dirs;     // [C, N, 3] through sd
    int64_t sd[3];
    const float *emb;      // bwd: [C, 16] contiguous or null (no embedding / zero embedding)
    const float *bias1;    // [C, 64]: b1 + W1[:, :E] emb[c]
    const float *W1;       // [64, E + 48]
    const float *W2, *b2, *W3, *b3;
    int32_t E, C, degree;
    int64_t N, ntiles;
    float *colors;         // fwd: [C, N, 3]
    const float *v_colors; // bwd: [C, N, 3] contiguous
    float *v_features;     // bwd: [N, 32]
    float *v_dirs;         // bwd: [C, N, 3] or null
    float *part_big;       // bwd: [blocks][2][64 * 64]: v_W2, v_W1 (columns [features | SH | embedding])
    float *part_small;     // bwd: [blocks * 4][kApSmall + C * 64]
};

__device__ __forceinline__ void ap_load_weights(const ApArgs &a, float *s_W1, float *s_W2, float *s_W3, float *s_b2)
{
    const int in = a.E + 48;
    for (int e = threadIdx.x; e < 64 * 64; e += kApThreads) {
        const int j = e >> 6, k = e & 63;
        float w = 0.0f;
        if (k < 48) w = a.W1[j * in + a.E + k];
        else if (a.E) w = a.W1[j * in + (k - 48)];
        s_W1[j * kApLd + k] = w;
        s_W2[j * kApLd + k] = a.W2[e];
    }
    for (int e = threadIdx.x; e < 3 * 64; e += kApThreads) s_W3[e] = a.W3[e];
    for (int e = threadIdx.x; e < 64; e += kApThreads) s_b2[e] = a.b2[e];
    __syncthreads();
}

struct ApDir {
    float x, y, z, nrm, den, ux, uy, uz;
};

// F.normalize(dirs, dim=-1): d / max(|d|, 1e-12)
__device__ __forceinline__ ApDir ap_dir(const ApArgs &a, int c, int64_t n, bool valid)
{
    ApDir d;
    d.x = d.y = d.z = 0.0f;
    if (valid) {
        const float *p = a.dirs + c * a.sd[0] + n * a.sd[1];
        d.x = p[0]; d.y = p[a.sd[2]]; d.z = p[2 * a.sd[2]];
    }
    d.nrm = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
    d.den = fmaxf(d.nrm, 1e-12f);
    d.ux = d.x / d.den; d.uy = d.y / d.den; d.uz = d.z / d.den;
    return d;
}

// H1^T = relu(W1 X^T + bias1[c]) and H2^T = relu(W2 H1^T + b2) of this wave's 32 Gaussians, as accumulator tiles.
// f: features[n][16 h + s]; Y: the 16 SH bases of the row (both halves hold all of them).
__device__ __forceinline__ void ap_hidden(const float *s_W1, const float *s_W2, const float *s_b2, const float *bias1c,
                                          const float (&f)[16], const float (&Y)[16], int g, int h, v16f &h10, v16f &h11,
                                          v16f &h20, v16f &h21)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const v4f b0 = *reinterpret_cast<const v4f *>(bias1c + 8 * q + 4 * h);
        const v4f b1 = *reinterpret_cast<const v4f *>(bias1c + 32 + 8 * q + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) { h10[4 * q + j] = b0[j]; h11[4 * q + j] = b1[j]; }
    }
    // k step s of the features: lane half h supplies k = s + 16 h; of the bases: k = 32 + s + 8 h
    const float *w0 = s_W1 + g * kApLd + 16 * h, *w1 = w0 + 32 * kApLd;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        h10 = AP_MFMA(w0[s], f[s], h10);
        h11 = AP_MFMA(w1[s], f[s], h11);
    }
    const float *u0 = s_W1 + g * kApLd + 32 + 8 * h, *u1 = u0 + 32 * kApLd;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const float y = ap_pick(h, Y[s], Y[s + 8]);
        h10 = AP_MFMA(u0[s], y, h10);
        h11 = AP_MFMA(u1[s], y, h11);
    }
    ap_relu(h10);
    ap_relu(h11);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        h20[r] = s_b2[ap_row(r, 0) + 4 * h];
        h21[r] = s_b2[32 + ap_row(r, 0) + 4 * h];
    }
    ap_mm_acc<kApLd, 1>(s_W2, g, h, h10, h11, h20);
    ap_mm_acc<kApLd, 1>(s_W2 + 32 * kApLd, g, h, h10, h11, h21);
    ap_relu(h20);
    ap_relu(h21);
}

__device__ __forceinline__ void ap_load_features(const ApArgs &a, int64_t n, bool valid, int h, float (&f)[16])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v4f v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid) v = *reinterpret_cast<const v4f *>(a.features + n * 32 + 16 * h + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) f[4 * q + j] = v[j];
    }
}

__global__ void __launch_bounds__(kApThreads) appearance_fwd_kernel(const ApArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_w[kApWeights];
    float *s_W1 = s_w, *s_W2 = s_W1 + 64 * kApLd, *s_W3 = s_W2 + 64 * kApLd, *s_b2 = s_W3 + 3 * 64;
    ap_load_weights(a, s_W1, s_W2, s_W3, s_b2);
    const int lane = lane_id(), wave = (int)threadIdx.x >> 6, g = lane & 31, h = lane >> 5;
    const float b30 = a.b3[0], b31 = a.b3[1], b32 = a.b3[2];
    for (int64_t tile = (int64_t)blockIdx.x * kApWaves + wave; tile < a.ntiles; tile += (int64_t)gridDim.x * kApWaves) {
        const int64_t n = tile * kApTile + g;
        const bool valid = n < a.N;
        float f[16];
        ap_load_features(a, n, valid, h, f);
        for (int c = 0; c < a.C; ++c) {
            const ApDir d = ap_dir(a, c, n, valid);
            float Y[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) Y[k] = 0.0f;
            sh_bases<false>(a.degree, d.ux, d.uy, d.uz, Y, nullptr, nullptr, nullptr);
            v16f h10, h11, h20, h21;
            ap_hidden(s_W1, s_W2, s_b2, a.bias1 + c * 64, f, Y, g, h, h10, h11, h20, h21);
            float o[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j0 = ap_row(r, 0) + 4 * h;
#pragma unroll
                for (int k = 0; k < 3; ++k) o[k] += s_W3[k * 64 + j0] * h20[r] + s_W3[k * 64 + 32 + j0] * h21[r];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) o[k] += __shfl_xor(o[k], 32);
            if (valid && h == 0) {
                float *out = a.colors + ((int64_t)c * a.N + n) * 3;
                out[0] = o[0] + b30; out[1] = o[1] + b31; out[2] = o[2] + b32;
            }
        }
    }
}

template <bool WANT_DIRS>
__global__ void __launch_bounds__(kApThreads) appearance_bwd_kernel(const ApArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_ap[];
    float *s_W1 = s_ap, *s_W2 = s_W1 + 64 * kApLd, *s_W3 = s_W2 + 64 * kApLd, *s_b2 = s_W3 + 3 * 64;
    float *s_stage = s_ap + kApWeights;
    ap_load_weights(a, s_W1, s_W2, s_W3, s_b2);
    const int lane = lane_id(), wave = (int)threadIdx.x >> 6, g = lane & 31, h = lane >> 5;
    float *sP = s_stage + wave * kApStage, *sQ = sP + 64 * kApSt;
    // lane l owns unit l of the sums over a tile's Gaussians, which it takes row-wise from the staged [unit][Gaussian] tiles
    const int small_len = kApSmall + a.C * 64;
    float *slot = a.part_small + ((int64_t)blockIdx.x * kApWaves + wave) * small_len;
    for (int c = 0; c < a.C; ++c) slot[kApSmall + c * 64 + lane] = 0.0f;
    v16f accW2[4], accW1[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { accW2[t] = ap_zero(); accW1[t] = ap_zero(); }
    float vb2 = 0.0f, vW3[3] = {0.0f, 0.0f, 0.0f}, vb3[3] = {0.0f, 0.0f, 0.0f};

    for (int64_t tile = (int64_t)blockIdx.x * kApWaves + wave; tile < a.ntiles; tile += (int64_t)gridDim.x * kApWaves) {
        const int64_t n = tile * kApTile + g;
        const bool valid = n < a.N;
        float f[16];
        ap_load_features(a, n, valid, h, f);
        v16f vf = ap_zero();
        for (int c = 0; c < a.C; ++c) {
            const ApDir d = ap_dir(a, c, n, valid);
            float Y[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) Y[k] = 0.0f;
            sh_bases<false>(a.degree, d.ux, d.uy, d.uz, Y, nullptr, nullptr, nullptr);
            v16f h10, h11, h20, h21;
            ap_hidden(s_W1, s_W2, s_b2, a.bias1 + c * 64, f, Y, g, h, h10, h11, h20, h21);
            float vo[3] = {0.0f, 0.0f, 0.0f}; // a row past N contributes nothing to any sum
            if (valid) {
                const float *p = a.v_colors + ((int64_t)c * a.N + n) * 3;
                vo[0] = p[0]; vo[1] = p[1]; vo[2] = p[2];
            }
            // layer 3 backwards. v_W3[k][j] = sum_g v_colors[g][k] H2[g][j] and v_b3: from H2 and v_colors staged
            ap_stage(sP, h20, h21, g, h);
            if (h == 0) { sQ[g] = vo[0]; sQ[kApSt + g] = vo[1]; sQ[2 * kApSt + g] = vo[2]; }
            wave_lds_sync();
            {
                const float *row = sP + lane * kApSt;
                float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
#pragma unroll 4
                for (int k = 0; k < kApTile; ++k) {
                    const float hv = row[k], v0 = sQ[k], v1 = sQ[kApSt + k], v2 = sQ[2 * kApSt + k];
                    w0 += v0 * hv; w1 += v1 * hv; w2 += v2 * hv;
                    c0 += v0; c1 += v1; c2 += v2;
                }
                vW3[0] += w0; vW3[1] += w1; vW3[2] += w2;
                vb3[0] += c0; vb3[1] += c1; vb3[2] += c2;
            }
            // dZ2 (into h20 / h21)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = ap_row(r, 0) + 4 * h;
                const float dh0 = s_W3[j] * vo[0] + s_W3[64 + j] * vo[1] + s_W3[128 + j] * vo[2];
                const float dh1 = s_W3[32 + j] * vo[0] + s_W3[96 + j] * vo[1] + s_W3[160 + j] * vo[2];
                h20[r] = h20[r] > 0.0f ? dh0 : 0.0f;
                h21[r] = h21[r] > 0.0f ? dh1 : 0.0f;
            }
            wave_lds_sync(); // the row sums above are done
            // v_W2 += dZ2^T H1, v_b2 += the row sums of dZ2^T
            ap_stage(sP, h20, h21, g, h);
            ap_stage(sQ, h10, h11, g, h);
            wave_lds_sync();
            {
                const float *row = sP + lane * kApSt;
                float t = 0.0f;
#pragma unroll 4
                for (int k = 0; k < kApTile; ++k) t += row[k];
                vb2 += t;
            }
            ap_outer(sP, sQ, g, h, accW2);
            // dZ1^T = (W2^T dZ2^T) where H1 > 0
            v16f d10 = ap_zero(), d11 = ap_zero();
            ap_mm_acc<1, kApLd>(s_W2, g, h, h20, h21, d10);
            ap_mm_acc<1, kApLd>(s_W2 + 32, g, h, h20, h21, d11);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                d10[r] = h10[r] > 0.0f ? d10[r] : 0.0f;
                d11[r] = h11[r] > 0.0f ? d11[r] : 0.0f;
            }
            // v_W1 += dZ1^T X, X = [features | SH | embedding]
            wave_lds_sync(); // the reads of the v_W2 product are done
            ap_stage(sP, d10, d11, g, h);
#pragma unroll
            for (int s = 0; s < 16; ++s) sQ[(s + 16 * h) * kApSt + g] = f[s];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                sQ[(32 + s + 8 * h) * kApSt + g] = ap_pick(h, Y[s], Y[s + 8]);
                sQ[(48 + s + 8 * h) * kApSt + g] = a.emb ? a.emb[c * 16 + s + 8 * h] : 0.0f;
            }
            wave_lds_sync();
            {   // this camera's column sums of dZ1: v_b1's and v_embed's source
                const float *row = sP + lane * kApSt;
                float t = 0.0f;
#pragma unroll 4
                for (int k = 0; k < kApTile; ++k) t += row[k];
                slot[kApSmall + c * 64 + lane] += t;
            }
            ap_outer(sP, sQ, g, h, accW1);
            // dX^T = W1^T dZ1^T: the features' rows accumulate over the cameras, the bases' rows give v_dirs
            ap_mm_acc<1, kApLd>(s_W1, g, h, d10, d11, vf);
            if constexpr (WANT_DIRS) {
                v16f dsh = ap_zero(); // rows 0-15: the bases (16-31: the embedding's columns, unused)
                ap_mm_acc<1, kApLd>(s_W1 + 32, g, h, d10, d11, dsh);
                float Yb[16], Yx[16], Yy[16], Yz[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) Yb[k] = Yx[k] = Yy[k] = Yz[k] = 0.0f;
                sh_bases<true>(a.degree, d.ux, d.uy, d.uz, Yb, Yx, Yy, Yz);
                float vx = 0.0f, vy = 0.0f, vz = 0.0f;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int k = ap_row(r, 0); // + 4 h
                    vx += dsh[r] * ap_pick(h, Yx[k], Yx[k + 4]);
                    vy += dsh[r] * ap_pick(h, Yy[k], Yy[k + 4]);
                    vz += dsh[r] * ap_pick(h, Yz[k], Yz[k + 4]);
                }
                vx += __shfl_xor(vx, 32); vy += __shfl_xor(vy, 32); vz += __shfl_xor(vz, 32);
                if (d.nrm >= 1e-12f) { // not clamped: through the norm as well
                    const float dot = d.ux * vx + d.uy * vy + d.uz * vz;
                    vx -= d.ux * dot; vy -= d.uy * dot; vz -= d.uz * dot;
                }
                if (valid && h == 0) {
                    float *out = a.v_dirs + ((int64_t)c * a.N + n) * 3;
                    out[0] = vx / d.den; out[1] = vy / d.den; out[2] = vz / d.den;
                }
            }
            wave_lds_sync(); // the reads of the v_W1 product are done before the next camera stages
        }
        if (valid) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4f v = {vf[4 * q], vf[4 * q + 1], vf[4 * q + 2], vf[4 * q + 3]};
                *reinterpret_cast<v4f *>(a.v_features + n * 32 + 8 * q + 4 * h) = v;
            }
        }
    }
    slot[lane] = vb2;
#pragma unroll
    for (int k = 0; k < 3; ++k) slot[64 + k * 64 + lane] = vW3[k];
    if (lane == 0) { slot[256] = vb3[0]; slot[257] = vb3[1]; slot[258] = vb3[2]; slot[259] = 0.0f; }
    float *big = a.part_big + (int64_t)blockIdx.x * 2 * 64 * 64;
    ap_reduce_big(s_stage, accW2, wave, g, h, big);
    ap_reduce_big(s_stage, accW1, wave, g, h, big + 64 * 64);
}

// sums of the partials in a fixed order: element e < 8192 of (v_W2 | v_W1) over the workgroups, then the small vector over
// the wave slots
__global__ void __launch_bounds__(256) appearance_finish_kernel(const float *part_big, int blocks, const float *part_small,
                                                                int small_len, float *v_W2, float *v_W1x, float *v_small)
{
    const int e = (int)(blockIdx.x * 256 + threadIdx.x);
    if (e < 2 * 64 * 64) {
        double t = 0.0;
        for (int b = 0; b < blocks; ++b) t += (double)part_big[(int64_t)b * 2 * 64 * 64 + e];
        if (e < 64 * 64) v_W2[e] = (float)t;
        else v_W1x[e - 64 * 64] = (float)t;
    } else if (e - 2 * 64 * 64 < small_len) {
        const int k = e - 2 * 64 * 64;
        double t = 0.0;
        for (int b = 0; b < blocks * kApWaves; ++b) t += (double)part_small[(int64_t)b * small_len + k];
        v_small[k] = (float)t;
    }
}

} // namespace gsx

using namespace gsx;

static int appearance_args(const char *who, ApArgs &a, const float *features, const float *dirs, const int64_t *strides_dirs,
                           const float *bias1, const float *W1, uint32_t embed_dim, const float *W2, const float *b2,
                           const float *W3, const float *b3, int64_t N, uint32_t C, uint32_t sh_degree)
{
    GSX_REQUIRE(features && dirs && strides_dirs && bias1 && W1 && W2 && b2 && W3 && b3, "%s: null argument", who);
    GSX_REQUIRE(embed_dim == 0 || embed_dim == 16, "%s: embed_dim %u (the kernel covers 0 and 16)", who, embed_dim);
    GSX_REQUIRE(sh_degree <= 3, "%s: sh_degree %u beyond the module's 3", who, sh_degree);
    GSX_REQUIRE(N > 0 && N < (int64_t)1 << 31 && C > 0 && C < 1u << 16, "%s: N %lld, C %u out of range", who, (long long)N, C);
    GSX_REQUIRE(((uintptr_t)features & 15) == 0 && ((uintptr_t)bias1 & 15) == 0, "%s: features / bias1 not 16-byte aligned", who);
    a.features = features; a.dirs = dirs; a.bias1 = bias1; a.W1 = W1; a.W2 = W2; a.b2 = b2; a.W3 = W3; a.b3 = b3;
    for (int k = 0; k < 3; ++k) a.sd[k] = strides_dirs[k];
    a.E = (int32_t)embed_dim; a.C = (int32_t)C; a.degree = (int32_t)sh_degree; a.N = N; a.ntiles = ceil_div(N, kApTile);
    return GSX_OK;
}

extern "C" int gsx_appearance_fwd(const float *features, const float *dirs, const int64_t *strides_dirs, const float *bias1,
                                  const float *W1, uint32_t embed_dim, const float *W2, const float *b2, const float *W3,
                                  const float *b3, int64_t N, uint32_t C, uint32_t sh_degree, float *colors, void *stream)
{
    if (N == 0 || C == 0) return GSX_OK;
    ApArgs a{};
    if (int rc = appearance_args("gsx_appearance_fwd", a, features, dirs, strides_dirs, bias1, W1, embed_dim, W2, b2, W3, b3, N, C,
                                 sh_degree))
        return rc;
    GSX_REQUIRE(colors, "gsx_appearance_fwd: null argument");
    a.colors = colors;
    int64_t blocks = ceil_div(a.ntiles, kApWaves);
    if (blocks > 4 * kApMaxBlocks) blocks = 4 * kApMaxBlocks;
    appearance_fwd_kernel<<<dim3((unsigned)blocks), kApThreads, 0, (hipStream_t)stream>>>(a);
    return check_launch("appearance_fwd");
}

extern "C" int64_t gsx_appearance_bwd_blocks(int64_t N)
{
    const int64_t blocks = ceil_div(ceil_div(N, kApTile), kApWaves);
    return blocks < 1 ? 1 : (blocks > kApMaxBlocks ? kApMaxBlocks : blocks);
}

extern "C" int64_t gsx_appearance_bwd_workspace_floats(int64_t N, uint32_t C)
{
    return gsx_appearance_bwd_blocks(N) * (2 * 64 * 64 + (int64_t)kApWaves * (kApSmall + (int64_t)C * 64));
}

extern "C" int gsx_appearance_bwd(const float *features, const float *dirs, const int64_t *strides_dirs, const float *embeds,
                                  const float *bias1, const float *W1, uint32_t embed_dim, const float *W2, const float *b2,
                                  const float *W3, const float *b3, int64_t N, uint32_t C, uint32_t sh_degree,
                                  const float *v_colors, float *workspace, float *v_features, float *v_dirs, float *v_W1x,
                                  float *v_W2, float *v_small, void *stream)
{
    if (N == 0 || C == 0) return GSX_OK;
    ApArgs a{};
    if (int rc = appearance_args("gsx_appearance_bwd", a, features, dirs, strides_dirs, bias1, W1, embed_dim, W2, b2, W3, b3, N, C,
                                 sh_degree))
        return rc;
    GSX_REQUIRE(v_colors && workspace && v_features && v_W1x && v_W2 && v_small, "gsx_appearance_bwd: null argument");
    GSX_REQUIRE(((uintptr_t)v_features & 15) == 0, "gsx_appearance_bwd: v_features not 16-byte aligned");
    GSX_REQUIRE(!embeds || embed_dim == 16, "gsx_appearance_bwd: embeddings without embed_dim 16");
    const int blocks = (int)gsx_appearance_bwd_blocks(N);
    const int small_len = kApSmall + (int)C * 64;
    a.emb = embeds; a.v_colors = v_colors; a.v_features = v_features; a.v_dirs = v_dirs;
    a.part_big = workspace; a.part_small = workspace + (int64_t)blocks * 2 * 64 * 64;
    const size_t lds = (size_t)(kApWeights + kApWaves * kApStage) * sizeof(float);
    // the dynamic-LDS limit is per device; a device counts as done only once both calls have succeeded (a racing thread sets
    // the same values again)
    static bool raised[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !raised[dev]) {
        if (hipFuncSetAttribute((const void *)appearance_bwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess
            || hipFuncSetAttribute((const void *)appearance_bwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
            set_last_error("gsx_appearance_bwd: cannot raise the dynamic LDS limit to %zu bytes", lds);
            return GSX_ERR_ARG;
        }
        if (dev >= 0 && dev < 64) raised[dev] = true;
    }
    if (v_dirs) appearance_bwd_kernel<true><<<dim3((unsigned)blocks), kApThreads, lds, (hipStream_t)stream>>>(a);
    else appearance_bwd_kernel<false><<<dim3((unsigned)blocks), kApThreads, lds, (hipStream_t)stream>>>(a);
    if (int rc = check_launch("appearance_bwd")) return rc;
    const int n_out = 2 * 64 * 64 + small_len;
    appearance_finish_kernel<<<dim3((unsigned)ceil_div(n_out, 256)), 256, 0, (hipStream_t)stream>>>(
        a.part_big, blocks, a.part_small, small_len, v_W2, v_W1x, v_small);
    return check_launch("appearance_finish");
}
