// gsplat_amd — colour correction of a render against its ground truth before it is scored (gfx950, MI355X, CDNA4).
// C-ABI: gsx_cc_blocks / gsx_cc_quadratic / gsx_cc_affine.
//
// What they replace (values: gsplat/color_correct.py; the trainer's use_color_correction_metric block):
//   quadratic   num_iters times: per channel c the least-squares fit of ref_c by the ten features (rr, rg, rb, gg, gb, bb, r, g,
//               b, 1) of the current image over the rows where the original img_c, the current img_c and ref_c all lie in
//               [eps, 1 - eps]; then img = clip(features @ W, 0, 1). The reference builds the [pixels, 10] matrix and calls
//               lstsq on a masked copy per channel and iteration, each followed by a host read.
//   affine      per channel the fit a ref + b = img over all pixels, then clip((img - b) / a, 0, 1).
//
// Quadratic, the Gram-solve formulation: iteration k is one pass that reads img and ref only, re-applies W_0 .. W_{k-1} in
// registers (no intermediate image is stored; the mask of the original image comes from img itself), and sums per channel the
// upper triangle of A^T M A (55 sums) and A^T M ref_c (10 sums) in double, the products formed in double. One workgroup then adds
// the workgroups' sums in a fixed order, scales each channel's 10 x 10 Gram matrix to unit diagonal, solves by Cholesky in double
// and writes W_k[:, c]. A scaled pivot <= 1e-10 or a zero diagonal entry sets bit c of a device status word and leaves W_k[:, c]
// zero: beyond a condition number of 1e10 a double solve no longer carries float32 accuracy, and an exactly rank-deficient
// system (a grey image, a channel without usable rows, fewer than ten distinct pixels) shows pivots near 1e-16. A last pass
// applies all warps and writes the output: 2 num_iters + 1 launches. Each warp is evaluated in double, clipped to [0, 1] and
// rounded to float32 once, as the reference's float32 img_mat is.
//
// Affine: one pass leaves per workgroup and channel the centred moments of (ref, img) (moments.hpp), one workgroup merges them
// and applies the reference's two clamps in double (var_ref >= 1e-8; a = 1 where |a| < 1e-8), a second pass writes the output.
//
// Reductions follow depth_loss.hip: per-workgroup results in a scratch buffer in double, combined by ONE workgroup in a fixed
// order; no float atomics, so an output repeats bit for bit.
#include "moments.hpp"

#include <math.h>

namespace gsx {

constexpr int kCcThreads = 256, kCcPerThread = 4, kCcMaxBlocks = 512;
constexpr int kCcFeatures = 10, kCcTriangle = 55, kCcSums = kCcTriangle + kCcFeatures; // per channel
constexpr int kCcFinishThreads = 1024, kCcFinishGroups = kCcFinishThreads / 256;
constexpr double kCcMinPivot = 1e-10;
static_assert(GSX_CC_PARTIALS == 3 * kCcSums, "the Gram pass leaves 65 sums per channel and workgroup");
static_assert(GSX_CC_PARTIALS >= 3 * kMomentQuantities && GSX_CC_PARTIALS <= 256, "one scratch size serves both methods");

struct CcPixel { float v[3]; };

__device__ __forceinline__ CcPixel cc_load(const float *img, uint64_t p)
{
    return {{img[3 * p], img[3 * p + 1], img[3 * p + 2]}};
}

// torch.clip: a NaN stays a NaN
__device__ __forceinline__ double cc_clip01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

__device__ __forceinline__ void cc_features(const CcPixel &x, double (&f)[kCcFeatures])
{
    const double r = (double)x.v[0], g = (double)x.v[1], b = (double)x.v[2];
    f[0] = r * r; f[1] = r * g; f[2] = r * b; f[3] = g * g; f[4] = g * b; f[5] = b * b; f[6] = r; f[7] = g; f[8] = b; f[9] = 1.0;
}

// x <- float32(clip(features(x) @ W, 0, 1)), W [10, 3] doubles
__device__ __forceinline__ CcPixel cc_warp(const CcPixel &x, const double *__restrict__ W)
{
    double f[kCcFeatures];
    cc_features(x, f);
    CcPixel y;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < kCcFeatures; ++i) s += f[i] * W[3 * i + c];
        y.v[c] = (float)cc_clip01(s);
    }
    return y;
}

__device__ __forceinline__ bool cc_unclipped(float z, float lo, float hi) { return z >= lo && z <= hi; }

__device__ __forceinline__ double cc_wave_sum_f64(double x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// Iteration n_warps of the quadratic fit, channel blockIdx.y: partial[(blockIdx.x * 3 + c) * 65 + k] = this workgroup's sums.
__global__ void __launch_bounds__(kCcThreads) cc_gram_kernel(const float *__restrict__ img, const float *__restrict__ ref,
                                                              uint32_t n, const double *__restrict__ warps, int n_warps, float lo,
                                                              float hi, double *__restrict__ partial)
{
    __shared__ double s_red[kCcThreads / kWave][kCcSums];
    const int c = (int)blockIdx.y;
    double acc[kCcSums] = {};
    for (uint64_t p = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; p < n; p += (uint64_t)gridDim.x * kCcThreads) {
        CcPixel x    = cc_load(img, p);
        const float b = ref[3 * p + c];
        bool use      = cc_unclipped(x.v[c], lo, hi) && cc_unclipped(b, lo, hi);
        for (int k = 0; k < n_warps; ++k) x = cc_warp(x, warps + k * 3 * kCcFeatures);
        use = use && cc_unclipped(x.v[c], lo, hi);
        if (!use) continue;
        double f[kCcFeatures];
        cc_features(x, f);
        int t = 0;
#pragma unroll
        for (int i = 0; i < kCcFeatures; ++i)
#pragma unroll
            for (int j = i; j < kCcFeatures; ++j) acc[t++] += f[i] * f[j];
#pragma unroll
        for (int i = 0; i < kCcFeatures; ++i) acc[kCcTriangle + i] += f[i] * (double)b;
    }
#pragma unroll
    for (int k = 0; k < kCcSums; ++k) {
        const double t = cc_wave_sum_f64(acc[k]);
        if (lane_id() == 0) s_red[threadIdx.x / kWave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < kCcSums) {
        double t = 0.0;
        for (int w = 0; w < kCcThreads / kWave; ++w) t += s_red[w][threadIdx.x];
        partial[((int64_t)blockIdx.x * 3 + c) * kCcSums + threadIdx.x] = t;
    }
}

// index of (i, j), i <= j, in the row-major upper triangle
__device__ __forceinline__ int cc_tri(int i, int j) { return i * kCcFeatures - i * (i - 1) / 2 + (j - i); }

// One workgroup: the workgroups' sums in a fixed order, then thread c solves channel c and writes W[:, c] (W [10, 3]).
__global__ void __launch_bounds__(kCcFinishThreads) cc_solve_kernel(const double *__restrict__ partial, int n_blocks,
                                                                     double *__restrict__ W, uint32_t *status)
{
    __shared__ double s_part[kCcFinishGroups][GSX_CC_PARTIALS];
    __shared__ double s_sum[GSX_CC_PARTIALS];
    __shared__ double s_L[3][kCcFeatures][kCcFeatures];
    const int q = (int)threadIdx.x & 255, g = (int)threadIdx.x >> 8;
    if (q < GSX_CC_PARTIALS) {
        double acc = 0.0;
        for (int b = g; b < n_blocks; b += kCcFinishGroups) acc += partial[(int64_t)b * GSX_CC_PARTIALS + q];
        s_part[g][q] = acc;
    }
    __syncthreads();
    if (threadIdx.x < GSX_CC_PARTIALS) {
        double t = 0.0;
        for (int k = 0; k < kCcFinishGroups; ++k) t += s_part[k][threadIdx.x];
        s_sum[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x >= 3) return;
    const int c         = (int)threadIdx.x;
    const double *gram  = s_sum + c * kCcSums, *rhs = gram + kCcTriangle;
    double (*L)[kCcFeatures] = s_L[c];
    double scale[kCcFeatures], y[kCcFeatures];
    bool bad = false;
    for (int i = 0; i < kCcFeatures; ++i) {
        const double d = gram[cc_tri(i, i)];
        bad            = bad || !(d > 0.0) || !(d < INFINITY);
        scale[i]       = bad ? 1.0 : 1.0 / sqrt(d);
    }
    // Cholesky of S = D^-1/2 G D^-1/2 (unit diagonal), column by column
    for (int j = 0; j < kCcFeatures && !bad; ++j) {
        double d = 1.0;
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > kCcMinPivot)) { bad = true; break; }
        const double l = sqrt(d);
        L[j][j]        = l;
        for (int i = j + 1; i < kCcFeatures; ++i) {
            double s = gram[cc_tri(j, i)] * scale[i] * scale[j];
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            L[i][j] = s / l;
        }
    }
    if (!bad) {
        for (int i = 0; i < kCcFeatures; ++i) { // L y = D^-1/2 rhs
            double s = rhs[i] * scale[i];
            for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
            y[i] = s / L[i][i];
        }
        for (int i = kCcFeatures - 1; i >= 0; --i) { // L^T x = y
            double s = y[i];
            for (int k = i + 1; k < kCcFeatures; ++k) s -= L[k][i] * y[k];
            y[i] = s / L[i][i];
        }
    }
    for (int i = 0; i < kCcFeatures; ++i) W[3 * i + c] = bad ? 0.0 : y[i] * scale[i];
    if (bad) atomicOr(status, 1u << c);
}

__global__ void __launch_bounds__(kCcThreads) cc_apply_kernel(const float *__restrict__ img, uint32_t n,
                                                               const double *__restrict__ warps, int n_warps,
                                                               float *__restrict__ out)
{
    for (uint64_t p = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; p < n; p += (uint64_t)gridDim.x * kCcThreads) {
        CcPixel x = cc_load(img, p);
        for (int k = 0; k < n_warps; ++k) x = cc_warp(x, warps + k * 3 * kCcFeatures);
        out[3 * p] = x.v[0]; out[3 * p + 1] = x.v[1]; out[3 * p + 2] = x.v[2];
    }
}

// ---- affine -------------------------------------------------------------------------------------------------------------------
// partial[(c * 6 + quantity) * gridDim.x + blockIdx.x]: the moments of (ref_c, img_c) over this workgroup's pixels
__global__ void __launch_bounds__(kCcThreads) cc_affine_moments_kernel(const float *__restrict__ img, const float *__restrict__ ref,
                                                                        uint32_t n, double *__restrict__ partial)
{
    __shared__ double s_red[kMomentQuantities * kCcThreads / kWave];
    MomentSums sums[3];
    for (uint64_t p = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; p < n; p += (uint64_t)gridDim.x * kCcThreads) {
        const CcPixel x = cc_load(img, p), r = cc_load(ref, p);
#pragma unroll
        for (int c = 0; c < 3; ++c) sums[c].add((double)r.v[c], (double)x.v[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c) __syncthreads(); // s_red is rewritten
        const Moments m = mom_block<kCcThreads>(sums[c].moments(), s_red);
        if (threadIdx.x == 0) mom_store(partial + (int64_t)c * kMomentQuantities * gridDim.x + blockIdx.x, gridDim.x, m);
    }
}

// One workgroup: coef[2 c] = a, coef[2 c + 1] = b of channel c
__global__ void __launch_bounds__(kCcThreads) cc_affine_finish_kernel(const double *__restrict__ partial, int n_blocks,
                                                                       double *__restrict__ coef)
{
    __shared__ double s_red[kMomentQuantities * kCcThreads / kWave];
    for (int c = 0; c < 3; ++c) {
        if (c) __syncthreads(); // s_red is rewritten
        const double *src = partial + (int64_t)c * kMomentQuantities * n_blocks;
        Moments m{};
        for (int i = threadIdx.x; i < n_blocks; i += kCcThreads) m = mom_merge(m, mom_load(src + i, n_blocks));
        m = mom_block<kCcThreads>(m, s_red);
        if (threadIdx.x != 0) continue;
        // p = ref, g = img: a = Cov(ref, img) / max(Var(ref), 1e-8), b = mean(img) - a mean(ref)
        const double var_ref = fmax(m.spp / m.n, 1e-8);
        double a             = (m.spg / m.n) / var_ref;
        const double b       = m.mg - a * m.mp;
        if (fabs(a) < 1e-8) a = 1.0;
        coef[2 * c] = a; coef[2 * c + 1] = b;
    }
}

__global__ void __launch_bounds__(kCcThreads) cc_affine_apply_kernel(const float *__restrict__ img, uint32_t n,
                                                                      const double *__restrict__ coef, float *__restrict__ out)
{
    for (uint64_t p = (uint64_t)blockIdx.x * kCcThreads + threadIdx.x; p < n; p += (uint64_t)gridDim.x * kCcThreads) {
        const CcPixel x = cc_load(img, p);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * p + c] = (float)cc_clip01(((double)x.v[c] - coef[2 * c + 1]) / coef[2 * c]);
    }
}

} // namespace gsx

using namespace gsx;

extern "C" int64_t gsx_cc_blocks(int64_t n)
{
    const int64_t blocks = n <= 0 ? 1 : ceil_div(n, (int64_t)kCcThreads * kCcPerThread);
    return blocks < 1 ? 1 : (blocks > kCcMaxBlocks ? kCcMaxBlocks : blocks);
}

static int cc_args(const char *who, const float *img, const float *ref, int64_t n, const double *partial_sums, const float *out)
{
    GSX_REQUIRE(img && ref && partial_sums && out, "%s: null argument", who);
    GSX_REQUIRE(n > 0, "%s: empty input (%lld pixels)", who, (long long)n);
    GSX_REQUIRE(3 * (double)n < 2147483648.0, "%s: 2^31 elements or more (%lld pixels)", who, (long long)n);
    return GSX_OK;
}

extern "C" int gsx_cc_quadratic(const float *img, const float *ref, int64_t n, int num_iters, double eps, double *partial_sums,
                                double *warps, uint32_t *status, float *out, void *stream)
{
    if (int rc = cc_args("gsx_cc_quadratic", img, ref, n, partial_sums, out)) return rc;
    GSX_REQUIRE(warps && status, "gsx_cc_quadratic: null argument");
    GSX_REQUIRE(num_iters >= 1 && num_iters <= GSX_CC_MAX_ITERS, "gsx_cc_quadratic: num_iters %d outside [1, %d]", num_iters,
                GSX_CC_MAX_ITERS);
    GSX_REQUIRE(eps == eps, "gsx_cc_quadratic: eps is NaN");
    const float lo = (float)eps, hi = (float)(1.0 - eps); // a float32 tensor compared with a Python scalar: the scalar is rounded
    hipStream_t s  = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(uint32_t), s) != hipSuccess) {
        set_last_error("gsx_cc_quadratic: clearing the status word failed");
        return GSX_ERR_LAUNCH;
    }
    const int blocks = (int)gsx_cc_blocks(n);
    for (int k = 0; k < num_iters; ++k) {
        cc_gram_kernel<<<dim3(blocks, 3), kCcThreads, 0, s>>>(img, ref, (uint32_t)n, warps, k, lo, hi, partial_sums);
        if (int rc = check_launch("cc_gram")) return rc;
        cc_solve_kernel<<<1, kCcFinishThreads, 0, s>>>(partial_sums, blocks, warps + (int64_t)k * 3 * kCcFeatures, status);
        if (int rc = check_launch("cc_solve")) return rc;
    }
    cc_apply_kernel<<<blocks, kCcThreads, 0, s>>>(img, (uint32_t)n, warps, num_iters, out);
    return check_launch("cc_apply");
}

extern "C" int gsx_cc_affine(const float *img, const float *ref, int64_t n, double *partial_sums, double *coef, float *out,
                             void *stream)
{
    if (int rc = cc_args("gsx_cc_affine", img, ref, n, partial_sums, out)) return rc;
    GSX_REQUIRE(coef, "gsx_cc_affine: null argument");
    hipStream_t s    = (hipStream_t)stream;
    const int blocks = (int)gsx_cc_blocks(n);
    cc_affine_moments_kernel<<<blocks, kCcThreads, 0, s>>>(img, ref, (uint32_t)n, partial_sums);
    if (int rc = check_launch("cc_affine_moments")) return rc;
    cc_affine_finish_kernel<<<1, kCcThreads, 0, s>>>(partial_sums, blocks, coef);
    if (int rc = check_launch("cc_affine_finish")) return rc;
    cc_affine_apply_kernel<<<blocks, kCcThreads, 0, s>>>(img, (uint32_t)n, coef, out);
    return check_launch("cc_affine_apply");
}
