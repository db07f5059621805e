// What the two events-only training terms state once for every call that takes
// them alone or together (contrast.hip, avg_timestamp.hip; the joint calls of
// include/dvsof_event_terms_joint.h at the end of avg_timestamp.hip): the
// statistics of an image of warped events (iwe.hip, whose dvsof_iwe_stats the
// contrast term runs), the contrast record of an image, and the unit of the
// fixed-point gradient sums of a frame.  Everything here relies on
// -ffp-contract=off.
#pragma once
#include "event_images.h"

namespace {

constexpr int kUnitBits = 40;   // R = 1: |one event's addend| < 2^(kUnitBits + 1) units
constexpr int kSharedBits = 2;  // R > 1: up to three addends of a pixel's event share a sum

// 2^k: the flow gradient of a frame is summed in units of 1/unit; |G_m| <= gmax < 2^e for every image of the frame
__device__ __forceinline__ double unit_of(double gmax, int unit_bits)
{
    int e = 0;
    if (gmax > 0.0) (void)frexp(gmax, &e);
    return ldexp(1.0, unit_bits - e);
}

// ---------------------------------------------------------------------------
// Statistics of an image of warped events and its count image, by the
// fixed-order reduction of frame_common.h; the result row is the accumulator.
// ---------------------------------------------------------------------------
struct IweSum {
    using Row = dvsof_iwe_result_t;
    static __device__ __forceinline__ Row zero() { return Row{0.0, 0, 0, 0, 0, 0}; }
    static __device__ __forceinline__ Row add(const Row &a, const Row &b)
    {
        return Row{a.sum_sq + b.sum_sq, a.sum_q + b.sum_q, a.max_q > b.max_q ? a.max_q : b.max_q,
                   a.count_sum + b.count_sum, a.count_sq + b.count_sq,
                   a.count_max > b.count_max ? a.count_max : b.count_max};
    }
};

// what a pixel of Q units and c events adds to the row
__device__ __forceinline__ void iwe_stats_pixel(dvsof_iwe_result_t &a, int64_t Q, int64_t c)
{
    const double I = (double)Q * 0x1p-32;
    a.sum_sq += I * I;
    a.sum_q += Q;
    a.max_q = a.max_q > Q ? a.max_q : Q;
    a.count_sum += c;
    a.count_sq += c * c;
    a.count_max = a.count_max > c ? a.count_max : c;
}

// ---------------------------------------------------------------------------
// The contrast term's record of an image, in the workspace behind the sums.
// ---------------------------------------------------------------------------
struct ContrastRec {
    double mean;  // of I_m
    double coef;  // -2 / (N var(c_m)); 0 where var(c_m) is not positive
    double gmax;  // |coef (I_m - mean)| <= gmax on every pixel
    double term;  // 1 - var(I_m)/var(c_m); 0 where var(c_m) is not positive
};
static_assert(sizeof(ContrastRec) == 32, "the workspace holds 32 bytes per image");

// from the statistics row of an image of N pixels
__device__ __forceinline__ ContrastRec contrast_record_of(const dvsof_iwe_result_t &r, double N)
{
    const double mean = (double)r.sum_q * 0x1p-32 / N;
    const double var_i = r.sum_sq / N - mean * mean;
    const double cmean = (double)r.count_sum / N;
    const double var_c = (double)r.count_sq / N - cmean * cmean;
    ContrastRec o;
    o.mean = mean;
    o.coef = var_c > 0.0 ? -2.0 / (N * var_c) : 0.0;
    o.term = var_c > 0.0 ? 1.0 - var_i / var_c : 0.0;
    o.gmax = fabs(o.coef) * fmax((double)r.max_q * 0x1p-32 - mean, mean);
    return o;
}

}  // namespace
