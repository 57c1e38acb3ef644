// gsplat_amd — depth-supervision losses of the training step for gfx950 (MI355X, CDNA4).
// C-ABI: gsx_depth_blocks / gsx_depth_pearson_fwd / _bwd / gsx_depth_disparity_fwd / _bwd / gsx_depth_sampled_fwd / _bwd.
//
// What they replace (values: gsplat/losses.py:209-320; the sampled form: examples/simple_trainer.py:962-980):
//   depth_l1_loss            scale * mean |disp(p) - disp(g)|, disp(x) = x > 0 ? 1 / x : 0, over all elements
//   binocular_disparity_l1   mean |1 / p - 1 / g| over the pairs with |p| > eps, |g| > eps and mask != 0 (0 when none)
//   pearson_depth_loss       1 - Spg / sqrt(max(Spp Sgg, 1e-12)) over the elements with mask != 0 (0 when fewer than two)
//   sampled                  depth_l1_loss of a bilinear sample (align_corners=True, zeros outside) of a depth map at M points
// each a dozen torch launches and, with a mask, a device-to-host read of the selected count. Here every loss is one pass over its
// inputs per direction plus a one-workgroup finish; what the host would have decided (fewer than two samples, nothing selected,
// the clamp of the Pearson denominator) is decided by the finish kernel and left in a small device record for the backward.
//
// Reduction (the shape of gsx_tv_fwd): the pass leaves per-workgroup results in a scratch buffer, GSX_DEPTH_PARTIALS doubles per
// workgroup, quantity-major (sums for the disparity modes, centred moments for Pearson); ONE workgroup combines them in a fixed
// order. Threads, waves and workgroups are all combined in a fixed order and no float atomic takes part, so a loss and every
// dense gradient repeat bit for bit.
//
// Arithmetic. The sums are taken in double, and so is each element's term: a float32 evaluation of the Pearson raw moments is
// off by 1e-4 .. 3e-4 at depths of 20 +- 0.5, and the launch-bound passes have the time. The Pearson moments are kept centred:
// a thread sums about its own first selected pair (p - pivot is exact in double for float32 depths), turns its sums into
// (n, mean_p, mean_g, Spp, Sgg, Spg), and lanes, waves and workgroups are merged pairwise (n = na + nb, d = mb - ma,
// mean = ma + d nb / n, S = Sa + Sb + d d' na nb / n) in a fixed order. Nothing is read where the mask is 0, an outlier there
// cannot cost precision, and a constant pred gives Spp = Spg = 0 exactly, so the clamp decides as in the centred float64
// evaluation.
//
// The one departure from the reference: where a (sampled) predicted depth is <= 0 its gradient is 0. torch.where(d > 0, 1 / d, 0)
// back-propagates inf * 0 = NaN there, and an expected-depth render is 0 at every uncovered pixel. Loss values are unchanged.
//
// Atomics: only gsx_depth_sampled_bwd uses them. It zero-fills the dense [C, H, W] gradient and adds each point's four weighted
// taps with hardware float atomics (two SfM points may share a pixel), so that gradient is a float atomic sum: bit-equal between
// runs when no two points share a tap, equal to a few ulp otherwise.
#include "moments.hpp"

#include <math.h>

namespace gsx {

constexpr int kDpThreads = 256, kDpPerThread = 4, kDpMaxBlocks = 1024;
constexpr int kDpRecord = GSX_DEPTH_RECORD;
static_assert(GSX_DEPTH_PARTIALS == kMomentQuantities, "the Pearson pass leaves six sums per workgroup");
constexpr int kDpPearson = -1; // the backward kernel's third mode, next to GSX_DEPTH_L1 / GSX_DEPTH_BINOCULAR

struct DpArgs {
    const float *pred, *gt;
    const void *mask; // NULL: every element selected
    int32_t mask_u8;
    int64_t sp[4], sg[4], sm[4]; // element strides of pred, gt and mask (0 along a broadcast dimension)
    uint32_t d1, d2, d3, n;      // n = d0 d1 d2 d3 < 2^31
    float eps; // GSX_DEPTH_BINOCULAR: a depth counts where |depth| > eps
};

struct DpOffsets { int64_t p, g, m; };

template <bool LINEAR>
__device__ __forceinline__ DpOffsets dp_offsets(const DpArgs &a, uint32_t e)
{
    if (LINEAR) return {(int64_t)e, (int64_t)e, (int64_t)e};
    const uint32_t i3 = e % a.d3, t3 = e / a.d3, i2 = t3 % a.d2, t2 = t3 / a.d2, i1 = t2 % a.d1, i0 = t2 / a.d1;
    return {i0 * a.sp[0] + i1 * a.sp[1] + i2 * a.sp[2] + i3 * a.sp[3], i0 * a.sg[0] + i1 * a.sg[1] + i2 * a.sg[2] + i3 * a.sg[3],
            i0 * a.sm[0] + i1 * a.sm[1] + i2 * a.sm[2] + i3 * a.sm[3]};
}

__device__ __forceinline__ bool dp_selected(const DpArgs &a, int64_t off)
{
    if (!a.mask) return true;
    return a.mask_u8 ? static_cast<const uint8_t *>(a.mask)[off] != 0 : static_cast<const float *>(a.mask)[off] != 0.0f;
}

__device__ __forceinline__ double dp_sign(double d) { return d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0); }

// disparity of one pair: the difference, and whether the pair counts / whether pred passes a gradient
template <int MODE>
__device__ __forceinline__ bool dp_disparity(const DpArgs &a, float p, float g, double &d, double &inv_p)
{
    if (MODE == GSX_DEPTH_L1) {
        inv_p          = p > 0.0f ? 1.0 / (double)p : 0.0;
        const double q = g > 0.0f ? 1.0 / (double)g : 0.0;
        d              = inv_p - q;
        return p > 0.0f;
    }
    const bool ok = fabsf(p) > a.eps && fabsf(g) > a.eps;
    inv_p         = ok ? 1.0 / (double)p : 0.0;
    d             = ok ? inv_p - 1.0 / (double)g : 0.0;
    return ok;
}

__device__ __forceinline__ double wave_sum_f64(double x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// acc[NACC] of every thread -> partial[k * gridDim.x + blockIdx.x], lanes, then waves, in a fixed order
template <int NACC>
__device__ __forceinline__ void dp_block_sums(double (&acc)[NACC], double *partial)
{
    __shared__ double s_red[kDpThreads / kWave][NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const double t = wave_sum_f64(acc[k]);
        if (lane_id() == 0) s_red[threadIdx.x / kWave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        double t = 0.0;
        for (int w = 0; w < kDpThreads / kWave; ++w) t += s_red[w][threadIdx.x];
        partial[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

template <int MODE, bool LINEAR>
__global__ void __launch_bounds__(kDpThreads) depth_partial_kernel(const DpArgs a, double *partial)
{
    double acc[2] = {};
    for (uint64_t e = (uint64_t)blockIdx.x * kDpThreads + threadIdx.x; e < a.n; e += (uint64_t)gridDim.x * kDpThreads) {
        const DpOffsets o = dp_offsets<LINEAR>(a, (uint32_t)e);
        if (!dp_selected(a, o.m)) continue; // an element the mask drops is not read
        double d, inv_p;
        const bool ok = dp_disparity<MODE>(a, a.pred[o.p], a.gt[o.g], d, inv_p);
        if (MODE == GSX_DEPTH_L1 || ok) { acc[0] += 1.0; acc[1] += fabs(d); }
    }
    dp_block_sums<2>(acc, partial);
}

template <bool LINEAR>
__global__ void __launch_bounds__(kDpThreads) depth_pearson_partial_kernel(const DpArgs a, double *partial)
{
    __shared__ double s_red[GSX_DEPTH_PARTIALS * kDpThreads / kWave];
    MomentSums sums; // about the thread's pivot: its first selected pair
    for (uint64_t e = (uint64_t)blockIdx.x * kDpThreads + threadIdx.x; e < a.n; e += (uint64_t)gridDim.x * kDpThreads) {
        const DpOffsets o = dp_offsets<LINEAR>(a, (uint32_t)e);
        if (!dp_selected(a, o.m)) continue; // an element the mask drops is not read
        sums.add((double)a.pred[o.p], (double)a.gt[o.g]);
    }
    Moments m = sums.moments();
    m = mom_block<kDpThreads>(m, s_red);
    if (threadIdx.x == 0) mom_store(partial + blockIdx.x, gridDim.x, m);
}

// One workgroup: the workgroups' moments merged in a fixed order, then the loss and
// record = (loss, n, mean_p, mean_g, Spp, Sgg, Spg, denom), all zero but n when n < 2.
__global__ void __launch_bounds__(kDpThreads) depth_pearson_finish_kernel(const double *partial, int n_blocks, float *loss,
                                                                          double *record)
{
    __shared__ double s_red[GSX_DEPTH_PARTIALS * kDpThreads / kWave];
    Moments m{};
    for (int i = threadIdx.x; i < n_blocks; i += kDpThreads) m = mom_merge(m, mom_load(partial + i, n_blocks));
    m = mom_block<kDpThreads>(m, s_red);
    if (threadIdx.x != 0) return;
    double r[kDpRecord] = {};
    r[1] = m.n;
    if (m.n >= 2.0) {
        const double spp = fmax(m.spp, 0.0), sgg = fmax(m.sgg, 0.0), denom = sqrt(fmax(spp * sgg, 1e-12));
        r[0] = 1.0 - m.spg / denom;
        r[2] = m.mp; r[3] = m.mg; r[4] = spp; r[5] = sgg; r[6] = m.spg; r[7] = denom;
    }
    for (int k = 0; k < kDpRecord; ++k) record[k] = r[k];
    loss[0] = (float)r[0];
}

// One workgroup: the per-workgroup (count, sum |d|) in a fixed order, then the loss and
// record = (loss, count, sum |d|, gradient scale = scale / count, 0 when nothing counts).
__global__ void __launch_bounds__(kDpThreads) depth_finish_kernel(const double *partial, int n_blocks, double scale, float *loss,
                                                                  double *record)
{
    __shared__ double s[kDpThreads];
    __shared__ double s_tot[2];
    for (int k = 0; k < 2; ++k) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < n_blocks; i += kDpThreads) acc += partial[(int64_t)k * n_blocks + i];
        s[threadIdx.x] = acc;
        __syncthreads();
        for (int o = kDpThreads / 2; o >= 1; o >>= 1) {
            if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) s_tot[k] = s[0];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double r[kDpRecord] = {};
    const double cnt = s_tot[0], sum = s_tot[1];
    r[1] = cnt; r[2] = sum;
    r[3] = cnt > 0.0 ? scale / cnt : 0.0;
    r[0] = sum * r[3];
    for (int k = 0; k < kDpRecord; ++k) record[k] = r[k];
    loss[0] = (float)r[0];
}

template <int MODE, bool LINEAR>
__global__ void __launch_bounds__(kDpThreads) depth_bwd_kernel(const DpArgs a, const double *record, const float *grad,
                                                               float *v_pred)
{
    const uint64_t e = (uint64_t)blockIdx.x * kDpThreads + threadIdx.x;
    if (e >= a.n) return;
    const DpOffsets o = dp_offsets<LINEAR>(a, (uint32_t)e);
    float v           = 0.0f;
    if (dp_selected(a, o.m)) {
        const float p = a.pred[o.p], g = a.gt[o.g];
        const double vl = (double)grad[0];
        if (MODE == kDpPearson) {
            if (record[1] >= 2.0) {
                const double pc = (double)p - record[2], gc = (double)g - record[3];
                const double spp = record[4], sgg = record[5], num = record[6], denom = record[7];
                const bool clamped = !(spp * sgg >= 1e-12); // torch's clamp passes its gradient where the input is >= min
                v = (float)(-vl * (clamped ? gc : gc - num * pc / spp) / denom);
            }
        } else {
            double d, inv_p;
            if (dp_disparity<MODE>(a, p, g, d, inv_p)) v = (float)(dp_sign(d) * -(inv_p * inv_p) * record[3] * vl);
        }
    }
    v_pred[e] = v;
}

// ---- the trainer's sampled form: depth_map [C, H, W] through strides, points [C, M, 2] = (x, y) in pixels, depths_gt [C, M] ----
struct SmArgs {
    const float *map, *pts, *gt;
    int64_t s[3];           // element strides (c, h, w) of the map
    int32_t C, H, W, M;
    uint32_t n;             // C M < 2^31
};

struct SmTaps {
    int32_t x[2], y[2];
    double wx[2], wy[2];
    bool any; // the point lies within one pixel of the image: some tap may be inside
};

__device__ __forceinline__ SmTaps sm_taps(const SmArgs &a, uint32_t i)
{
    SmTaps t{};
    const float x = a.pts[2 * (int64_t)i], y = a.pts[2 * (int64_t)i + 1];
    t.any = x > -1.0f && x < (float)a.W && y > -1.0f && y < (float)a.H; // false for NaN: no index is formed from it
    if (!t.any) return t;
    const float x0 = floorf(x), y0 = floorf(y);
    t.x[0] = (int32_t)x0; t.x[1] = t.x[0] + 1; t.y[0] = (int32_t)y0; t.y[1] = t.y[0] + 1;
    t.wx[1] = (double)x - (double)x0; t.wx[0] = 1.0 - t.wx[1];
    t.wy[1] = (double)y - (double)y0; t.wy[0] = 1.0 - t.wy[1];
    return t;
}

__device__ __forceinline__ bool sm_inside(const SmArgs &a, int32_t x, int32_t y) { return x >= 0 && x < a.W && y >= 0 && y < a.H; }

__device__ __forceinline__ double sm_sample(const SmArgs &a, const SmTaps &t, int32_t c)
{
    double s = 0.0;
    if (!t.any) return s;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (sm_inside(a, t.x[k], t.y[j])) s += t.wy[j] * t.wx[k] * (double)a.map[c * a.s[0] + t.y[j] * a.s[1] + t.x[k] * a.s[2]];
    return s;
}

__global__ void __launch_bounds__(kDpThreads) depth_sampled_partial_kernel(const SmArgs a, double *partial)
{
    double acc[2] = {};
    for (uint64_t i = (uint64_t)blockIdx.x * kDpThreads + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * kDpThreads) {
        const SmTaps t = sm_taps(a, (uint32_t)i);
        const double s = sm_sample(a, t, (int32_t)(i / (uint32_t)a.M));
        const float g  = a.gt[i];
        acc[0] += 1.0;
        acc[1] += fabs((s > 0.0 ? 1.0 / s : 0.0) - (g > 0.0f ? 1.0 / (double)g : 0.0));
    }
    dp_block_sums<2>(acc, partial);
}

__global__ void __launch_bounds__(kDpThreads) depth_sampled_bwd_kernel(const SmArgs a, const double *record, const float *grad,
                                                                       float *v_map)
{
    const uint64_t i = (uint64_t)blockIdx.x * kDpThreads + threadIdx.x;
    if (i >= a.n) return;
    const SmTaps t = sm_taps(a, (uint32_t)i);
    if (!t.any) return;
    const int32_t c = (int32_t)(i / (uint32_t)a.M);
    const double s  = sm_sample(a, t, c);
    if (!(s > 0.0)) return; // the departure: no gradient through a sample that is not a depth
    const float g      = a.gt[i];
    const double inv_s = 1.0 / s, d = inv_s - (g > 0.0f ? 1.0 / (double)g : 0.0);
    const double coef  = dp_sign(d) * -(inv_s * inv_s) * record[3] * (double)grad[0];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float v = (float)(coef * t.wy[j] * t.wx[k]);
            if (v != 0.0f && sm_inside(a, t.x[k], t.y[j])) atomic_add_f32(v_map + ((int64_t)c * a.H + t.y[j]) * a.W + t.x[k], v);
        }
}

} // namespace gsx

using namespace gsx;

// the element strides of a contiguous [d0, d1, d2, d3] tensor, dimensions of size 1 aside
static bool dp_linear(const int64_t *s, const uint32_t *d)
{
    int64_t expect = 1;
    for (int k = 3; k >= 0; --k) {
        if (d[k] != 1 && s[k] != expect) return false;
        expect *= d[k];
    }
    return true;
}

static int dp_args(const char *who, DpArgs &a, bool &linear, const float *pred, const int64_t *strides_pred, const float *gt,
                   const int64_t *strides_gt, const void *mask, const int64_t *strides_mask, int mask_dtype, uint32_t d0,
                   uint32_t d1, uint32_t d2, uint32_t d3)
{
    GSX_REQUIRE(pred && strides_pred && gt && strides_gt, "%s: null argument", who);
    GSX_REQUIRE(!mask || strides_mask, "%s: a mask needs its strides", who);
    GSX_REQUIRE(mask_dtype == GSX_MASK_F32 || mask_dtype == GSX_MASK_U8, "%s: unknown mask dtype tag %d", who, mask_dtype);
    GSX_REQUIRE(d0 > 0 && d1 > 0 && d2 > 0 && d3 > 0, "%s: empty input [%u, %u, %u, %u]", who, d0, d1, d2, d3);
    GSX_REQUIRE((double)d0 * d1 * d2 * d3 < 2147483648.0, "%s: 2^31 elements or more", who);
    const int64_t n = (int64_t)d0 * d1 * d2 * d3;
    a.pred = pred; a.gt = gt; a.mask = mask; a.mask_u8 = mask_dtype == GSX_MASK_U8;
    a.d1 = d1; a.d2 = d2; a.d3 = d3; a.n = (uint32_t)n;
    const uint32_t d[4] = {d0, d1, d2, d3};
    for (int k = 0; k < 4; ++k) { a.sp[k] = strides_pred[k]; a.sg[k] = strides_gt[k]; a.sm[k] = mask ? strides_mask[k] : 0; }
    linear = dp_linear(a.sp, d) && dp_linear(a.sg, d) && (!mask || dp_linear(a.sm, d));
    return GSX_OK;
}

template <int MODE>
static int dp_forward(const char *who, const DpArgs &a, bool linear, double scale, double *partial, float *loss, double *record,
                      void *stream)
{
    const int blocks = (int)gsx_depth_blocks(a.n);
    if (linear) depth_partial_kernel<MODE, true><<<blocks, kDpThreads, 0, (hipStream_t)stream>>>(a, partial);
    else depth_partial_kernel<MODE, false><<<blocks, kDpThreads, 0, (hipStream_t)stream>>>(a, partial);
    if (int rc = check_launch(who)) return rc;
    depth_finish_kernel<<<1, kDpThreads, 0, (hipStream_t)stream>>>(partial, blocks, scale, loss, record);
    return check_launch("depth_finish");
}

static int dp_pearson_forward(const DpArgs &a, bool linear, double *partial, float *loss, double *record, void *stream)
{
    const int blocks = (int)gsx_depth_blocks(a.n);
    if (linear) depth_pearson_partial_kernel<true><<<blocks, kDpThreads, 0, (hipStream_t)stream>>>(a, partial);
    else depth_pearson_partial_kernel<false><<<blocks, kDpThreads, 0, (hipStream_t)stream>>>(a, partial);
    if (int rc = check_launch("depth_pearson_fwd")) return rc;
    depth_pearson_finish_kernel<<<1, kDpThreads, 0, (hipStream_t)stream>>>(partial, blocks, loss, record);
    return check_launch("depth_pearson_finish");
}

template <int MODE>
static int dp_backward(const char *who, const DpArgs &a, bool linear, const double *record, const float *grad, float *v_pred,
                       void *stream)
{
    const dim3 grid((unsigned)ceil_div(a.n, kDpThreads));
    if (linear) depth_bwd_kernel<MODE, true><<<grid, kDpThreads, 0, (hipStream_t)stream>>>(a, record, grad, v_pred);
    else depth_bwd_kernel<MODE, false><<<grid, kDpThreads, 0, (hipStream_t)stream>>>(a, record, grad, v_pred);
    return check_launch(who);
}

extern "C" int64_t gsx_depth_blocks(int64_t n)
{
    const int64_t blocks = n <= 0 ? 1 : ceil_div(n, (int64_t)kDpThreads * kDpPerThread);
    return blocks < 1 ? 1 : (blocks > kDpMaxBlocks ? kDpMaxBlocks : blocks);
}

extern "C" int gsx_depth_pearson_fwd(const float *pred, const int64_t *strides_pred, const float *gt, const int64_t *strides_gt,
                                     const void *mask, const int64_t *strides_mask, int mask_dtype, uint32_t d0, uint32_t d1,
                                     uint32_t d2, uint32_t d3, double *partial_sums, float *loss, double *record, void *stream)
{
    DpArgs a{};
    bool linear = false;
    if (int rc = dp_args("gsx_depth_pearson_fwd", a, linear, pred, strides_pred, gt, strides_gt, mask, strides_mask, mask_dtype, d0,
                         d1, d2, d3))
        return rc;
    GSX_REQUIRE(partial_sums && loss && record, "gsx_depth_pearson_fwd: null argument");
    return dp_pearson_forward(a, linear, partial_sums, loss, record, stream);
}

extern "C" int gsx_depth_pearson_bwd(const float *pred, const int64_t *strides_pred, const float *gt, const int64_t *strides_gt,
                                     const void *mask, const int64_t *strides_mask, int mask_dtype, uint32_t d0, uint32_t d1,
                                     uint32_t d2, uint32_t d3, const double *record, const float *grad_device, float *v_pred,
                                     void *stream)
{
    DpArgs a{};
    bool linear = false;
    if (int rc = dp_args("gsx_depth_pearson_bwd", a, linear, pred, strides_pred, gt, strides_gt, mask, strides_mask, mask_dtype, d0,
                         d1, d2, d3))
        return rc;
    GSX_REQUIRE(record && grad_device && v_pred, "gsx_depth_pearson_bwd: null argument");
    return dp_backward<kDpPearson>("depth_pearson_bwd", a, linear, record, grad_device, v_pred, stream);
}

static int dp_disparity_args(const char *who, DpArgs &a, int mode, float scale, float eps)
{
    GSX_REQUIRE(mode == GSX_DEPTH_L1 || mode == GSX_DEPTH_BINOCULAR, "%s: unknown mode %d", who, mode);
    GSX_REQUIRE(mode == GSX_DEPTH_BINOCULAR || !a.mask, "%s: depth_l1_loss takes no mask", who);
    GSX_REQUIRE(isfinite(scale) && eps >= 0.0f, "%s: scale %g must be finite and eps %g >= 0", who, (double)scale, (double)eps);
    a.eps = eps;
    return GSX_OK;
}

extern "C" int gsx_depth_disparity_fwd(const float *pred, const int64_t *strides_pred, const float *gt, const int64_t *strides_gt,
                                       const void *mask, const int64_t *strides_mask, int mask_dtype, uint32_t d0, uint32_t d1,
                                       uint32_t d2, uint32_t d3, int mode, float scale, float eps, double *partial_sums,
                                       float *loss, double *record, void *stream)
{
    DpArgs a{};
    bool linear = false;
    if (int rc = dp_args("gsx_depth_disparity_fwd", a, linear, pred, strides_pred, gt, strides_gt, mask, strides_mask, mask_dtype,
                         d0, d1, d2, d3))
        return rc;
    if (int rc = dp_disparity_args("gsx_depth_disparity_fwd", a, mode, scale, eps)) return rc;
    GSX_REQUIRE(partial_sums && loss && record, "gsx_depth_disparity_fwd: null argument");
    if (mode == GSX_DEPTH_L1) return dp_forward<GSX_DEPTH_L1>("depth_l1_fwd", a, linear, scale, partial_sums, loss, record, stream);
    return dp_forward<GSX_DEPTH_BINOCULAR>("depth_binocular_fwd", a, linear, 1.0, partial_sums, loss, record, stream);
}

extern "C" int gsx_depth_disparity_bwd(const float *pred, const int64_t *strides_pred, const float *gt, const int64_t *strides_gt,
                                       const void *mask, const int64_t *strides_mask, int mask_dtype, uint32_t d0, uint32_t d1,
                                       uint32_t d2, uint32_t d3, int mode, float eps, const double *record,
                                       const float *grad_device, float *v_pred, void *stream)
{
    DpArgs a{};
    bool linear = false;
    if (int rc = dp_args("gsx_depth_disparity_bwd", a, linear, pred, strides_pred, gt, strides_gt, mask, strides_mask, mask_dtype,
                         d0, d1, d2, d3))
        return rc;
    if (int rc = dp_disparity_args("gsx_depth_disparity_bwd", a, mode, 1.0f, eps)) return rc;
    GSX_REQUIRE(record && grad_device && v_pred, "gsx_depth_disparity_bwd: null argument");
    if (mode == GSX_DEPTH_L1) return dp_backward<GSX_DEPTH_L1>("depth_l1_bwd", a, linear, record, grad_device, v_pred, stream);
    return dp_backward<GSX_DEPTH_BINOCULAR>("depth_binocular_bwd", a, linear, record, grad_device, v_pred, stream);
}

static int sm_args(const char *who, SmArgs &a, const float *depth_map, const int64_t *strides_map, uint32_t C, uint32_t H,
                   uint32_t W, const float *points, const float *depths_gt, uint32_t M)
{
    GSX_REQUIRE(depth_map && strides_map && points && depths_gt, "%s: null argument", who);
    GSX_REQUIRE(C > 0 && H > 0 && W > 0 && M > 0, "%s: empty input (map [%u, %u, %u], %u points)", who, C, H, W, M);
    GSX_REQUIRE(H < 1u << 24 && W < 1u << 24, "%s: image side beyond 2^24 (%u x %u)", who, H, W); // pixel indices exact in float32
    GSX_REQUIRE((double)C * H * W < 2147483648.0, "%s: 2^31 map elements or more", who);
    GSX_REQUIRE((double)C * M < 2147483648.0, "%s: 2^31 points or more", who);
    a.map = depth_map; a.pts = points; a.gt = depths_gt;
    for (int k = 0; k < 3; ++k) a.s[k] = strides_map[k];
    a.C = (int32_t)C; a.H = (int32_t)H; a.W = (int32_t)W; a.M = (int32_t)M; a.n = C * M;
    return GSX_OK;
}

extern "C" int gsx_depth_sampled_fwd(const float *depth_map, const int64_t *strides_map, uint32_t C, uint32_t H, uint32_t W,
                                     const float *points, const float *depths_gt, uint32_t M, float scale, double *partial_sums,
                                     float *loss, double *record, void *stream)
{
    SmArgs a{};
    if (int rc = sm_args("gsx_depth_sampled_fwd", a, depth_map, strides_map, C, H, W, points, depths_gt, M)) return rc;
    GSX_REQUIRE(isfinite(scale), "gsx_depth_sampled_fwd: scale %g must be finite", (double)scale);
    GSX_REQUIRE(partial_sums && loss && record, "gsx_depth_sampled_fwd: null argument");
    const int blocks = (int)gsx_depth_blocks(a.n);
    depth_sampled_partial_kernel<<<blocks, kDpThreads, 0, (hipStream_t)stream>>>(a, partial_sums);
    if (int rc = check_launch("depth_sampled_fwd")) return rc;
    depth_finish_kernel<<<1, kDpThreads, 0, (hipStream_t)stream>>>(partial_sums, blocks, (double)scale, loss, record);
    return check_launch("depth_finish");
}

extern "C" int gsx_depth_sampled_bwd(const float *depth_map, const int64_t *strides_map, uint32_t C, uint32_t H, uint32_t W,
                                     const float *points, const float *depths_gt, uint32_t M, const double *record,
                                     const float *grad_device, float *v_map, void *stream)
{
    SmArgs a{};
    if (int rc = sm_args("gsx_depth_sampled_bwd", a, depth_map, strides_map, C, H, W, points, depths_gt, M)) return rc;
    GSX_REQUIRE(record && grad_device && v_map, "gsx_depth_sampled_bwd: null argument");
    if (hipMemsetAsync(v_map, 0, (size_t)C * H * W * sizeof(float), (hipStream_t)stream) != hipSuccess) {
        set_last_error("gsx_depth_sampled_bwd: zero-fill of the gradient failed");
        return GSX_ERR_LAUNCH;
    }
    depth_sampled_bwd_kernel<<<dim3((unsigned)ceil_div(a.n, kDpThreads)), kDpThreads, 0, (hipStream_t)stream>>>(a, record,
                                                                                                                grad_device, v_map);
    return check_launch("depth_sampled_bwd");
}
