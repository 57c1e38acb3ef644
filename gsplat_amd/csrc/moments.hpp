// gsplat_amd — centred second moments of a set of (p, g) pairs in double, merged pairwise in a fixed order (gfx950, wave64).
// Shared by the Pearson depth loss (depth_loss.hip) and the affine colour correction (color_correct.hip).
//
// A thread sums about its own first pair (p - pivot is exact in double for float32 values), turns its sums into
// (n, mean_p, mean_g, Spp, Sgg, Spg), and lanes, waves and workgroups are merged pairwise (n = na + nb, d = mb - ma,
// mean = ma + d nb / n, S = Sa + Sb + d d' na nb / n). Every caller merges in a fixed order, so a result repeats bit for bit.
#pragma once

#include "common.hpp"

namespace gsx {

constexpr int kMomentQuantities = 6;

struct Moments { double n, mp, mg, spp, sgg, spg; };

// a thread's running sums about its pivot (its first pair)
struct MomentSums {
    double n = 0.0, qp = 0.0, qg = 0.0, sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;

    __device__ __forceinline__ void add(double p, double g)
    {
        if (n == 0.0) { qp = p; qg = g; }
        const double x = p - qp, y = g - qg;
        n += 1.0; sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
    }

    __device__ __forceinline__ Moments moments() const
    {
        if (!(n > 0.0)) return Moments{};
        const double mx = sx / n, my = sy / n;
        return {n, qp + mx, qg + my, sxx - sx * mx, syy - sy * my, sxy - sx * my};
    }
};

// a and b merged, in this order (the rounding depends on it: every caller merges in a fixed order)
__device__ __forceinline__ Moments mom_merge(const Moments &a, const Moments &b)
{
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, dp = b.mp - a.mp, dg = b.mg - a.mg, w = a.n * b.n / n, f = b.n / n;
    return {n, a.mp + dp * f, a.mg + dg * f, a.spp + b.spp + dp * dp * w, a.sgg + b.sgg + dg * dg * w, a.spg + b.spg + dp * dg * w};
}

__device__ __forceinline__ Moments mom_shfl_down(const Moments &m, int o)
{
    return {__shfl_down(m.n, o), __shfl_down(m.mp, o), __shfl_down(m.mg, o), __shfl_down(m.spp, o), __shfl_down(m.sgg, o),
            __shfl_down(m.spg, o)};
}

__device__ __forceinline__ void mom_store(double *dst, int64_t stride, const Moments &m)
{
    dst[0] = m.n; dst[stride] = m.mp; dst[2 * stride] = m.mg; dst[3 * stride] = m.spp; dst[4 * stride] = m.sgg; dst[5 * stride] = m.spg;
}

__device__ __forceinline__ Moments mom_load(const double *src, int64_t stride)
{
    return {src[0], src[stride], src[2 * stride], src[3 * stride], src[4 * stride], src[5 * stride]};
}

// the moments of all THREADS threads of the workgroup, valid in thread 0: lanes by a shuffle tree, then the waves in order.
// s_red: kMomentQuantities * THREADS / kWave doubles of LDS; a second call on the same s_red needs a __syncthreads() first.
template <int THREADS>
__device__ __forceinline__ Moments mom_block(Moments m, double *s_red)
{
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) m = mom_merge(m, mom_shfl_down(m, o)); // lane 0: ((0, 1), (2, 3)), ...
    if (lane_id() == 0) mom_store(s_red + threadIdx.x / kWave, THREADS / kWave, m);
    __syncthreads();
    Moments t{};
    if (threadIdx.x == 0)
        for (int w = 0; w < THREADS / kWave; ++w) t = mom_merge(t, mom_load(s_red + w, THREADS / kWave));
    return t;
}

} // namespace gsx
