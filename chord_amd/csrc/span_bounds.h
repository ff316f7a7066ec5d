// The span of one pixel row of a triangle, in steps k of the row loop: the ONE definition that scan_row,
// scan_span_i32 and masked_rows (kernels_raster.hip) bound their loops with.  Compiles for host and device: the device passes
// __builtin_amdgcn_rcpf as the reciprocal, a host program (tests/span_bounds_main.cpp) whatever it wants to try.
//
// A row loop walks k = 0 .. n (n = lx1 - lx0) with three exact incremental edge values E_i + k * st_i; the pixel at step k is
// covered iff all three are >= 0 (the top-left bias is folded into E_i).  Edge i alone allows
//     st_i > 0:  k >= q_i        st_i < 0:  k <= q_i        with  q_i = -E_i / st_i  (a real number),
// so the covered steps are  max(0, max ceil(q_i)) .. min(n, min floor(q_i)).  The loop does not need that interval exactly: it
// decides coverage by the exact integers (or exact doubles) itself and merges 0 for a pixel outside, so any interval that CONTAINS
// the covered steps gives the same image.  span_bounds() returns such an interval from fp32 estimates of the q_i, and as tight a
// one as the estimates' error allows:
//     k0 = max(0, max over st_i > 0 of ceil(q_i - delta)),      k1 = min(n, min over st_i < 0 of floor(q_i + delta)).
//
// The error that delta has to clear.  q = -(float)E * rcp((float)st):
//   (float)E       one rounding of an exact integer or double: relative error <= 2^-24
//   (float)st      exact for the int32 kind (|a| <= 2^14, st = 256 a), one rounding otherwise: <= 2^-24
//   rcp            v_rcp_f32 is accurate to 1 ulp: <= 2^-23
//   the product    one rounding: <= 2^-24
// together (1 + 2^-24)^3 (1 + 2^-23) - 1 < 2^-22 relative.  A crossing matters only where it can move a bound that the bbox has
// not already set, that is for q in [0, n] with n <= 63 (a row segment is at most 64 pixels); with the margin the code takes,
// q in [-4, 68], |q| * 2^-22 < 2^-15 pixels.  At the clamp value 4096 it is 2^-10.  SPAN_DELTA = 2^-6 clears both a
// hundredfold; q -+ delta is exact to half an ulp of q (<= 2^-18 below 68), which changes nothing in that.  Conservative means:
// the estimate q' of a true crossing q satisfies |q' - q| < delta, so ceil(q' - delta) <= ceil(q) and floor(q' + delta) >=
// floor(q): a covered step is never cut.  Tight means: ceil(q' - delta) >= ceil(q - 2 delta) >= ceil(q) - 1, and the same on the
// right: at most one pixel beyond the span on either side (and none unless the crossing lies within 2 delta = 1/32 px of
// a pixel centre), where the earlier floor(q) - 1 / floor(q) + 1 scanned one to two beyond on either side.
//
// The clamp of q to [-4, 4096] keeps the conversion to int32 defined and stays as it was.  It is safe because a true crossing
// beyond a clamp value lies on the same side of the whole row as the clamp value does: st > 0 and q > 4096 gives k0 = 4096 > n
// (nothing covered: right), q < -4 gives k0 = 0 (every step allowed: right); st < 0 and q > 4096 gives k1 = n, q < -4 gives
// k1 = -4 < 0 (nothing covered).  A zero step makes the edge constant along the row: outside (E < 0) empties the span (k1 = -1),
// otherwise the edge sets no bound; its q is -E * inf = -+inf, or NaN for E == 0 (0 * inf), which fmaxf turns into -4 -- either
// way a finite value that no branch reads.
//
// -DSPAN_SLACK_LEGACY=1 (a measurement variant, build switch only) returns the earlier bounds floor(q) - 1 / floor(q) + 1.
//
// The form of the code.  The three cases of an edge (st > 0, st < 0, st == 0 and outside) are an if / else-if ladder; the lanes
// of a wave hold different edges with different signs, so a wave runs every arm anyway and pays the exec-mask bookkeeping of three
// nested ladders on top.  -DSPAN_STRAIGHT=1 (a measurement variant) compiles the same values as selects:
//     klo = max(klo, st > 0 ? ceil(q - delta) : 0)                       0 is neutral: klo starts at 0 and only grows
//     khi = st == 0 && E < 0 ? -1 : min(khi, st < 0 ? floor(q + delta) : SPAN_NONE)     SPAN_NONE is above every khi
// (the constant-and-outside case ASSIGNS -1 as the ladder does; it does not take the minimum: an earlier edge may have left khi at
// -4, and k1 is the ladder's for every input; tests/span_bounds_equal_main.cpp holds a copy of the ladder and compares).  The tile
// kernel then issues 75 scalar instructions and 13 branches fewer (static), 14 vector ones and 10 registers more, and its frame
// is 0.4 % SLOWER on the flagship workload (profiles/r11_row_units.txt): the ladder is the product.
//
// Two entrances, one body.  span_bounds() computes the three reciprocals with the reciprocal it is given; span_bounds_rcp() takes
// them ready-made (they belong to the triangle, not to the row: a tile kernel that stored a triangle's three with its batch entry
// was measured and rejected, kernels_raster.hip) and wants of the steps only their signs, so it takes them in any arithmetic type
// -- the int32 steps as they are, unconverted.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef SPAN_SLACK_LEGACY
#define SPAN_SLACK_LEGACY 0
#endif
#ifndef SPAN_STRAIGHT
#define SPAN_STRAIGHT 0
#endif
#define SPAN_DELTA 0.015625f        // 2^-6 px
#define SPAN_NONE 8192.0f           // no bound: above n (<= 63) and above floor(4096 + delta)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPAN_HD __host__ __device__ __forceinline__
#else
#define SPAN_HD inline
#endif

// e[i]: the edge values at step 0, converted to float; t[i]: the steps per pixel (only their signs are read: float or integer);
// r[i]: the reciprocals of the steps as floats; n: the row's last step.
// Steps k0 .. k1 (k1 < k0: none) contain every covered step of 0 .. n.
template <typename Step>
SPAN_HD void span_bounds_rcp(const float (&e)[3], const Step (&t)[3], const float (&r)[3], int32_t n, int32_t& k0, int32_t& k1)
{
    float klo = 0.0f, khi = (float)n;
#if defined(__HIPCC__) || defined(__CUDACC__)
#pragma unroll
#endif
    for (int i = 0; i < 3; i++) {
        const float q = fminf(fmaxf(-e[i] * r[i], -4.0f), 4096.0f);                           // NaN (0 * inf) -> -4
#if SPAN_SLACK_LEGACY
        const float lo = floorf(q) - 1.0f, hi = floorf(q) + 1.0f;
#else
        const float lo = ceilf(q - SPAN_DELTA), hi = floorf(q + SPAN_DELTA);
#endif
#if SPAN_STRAIGHT
        const bool pos = t[i] > (Step)0, neg = t[i] < (Step)0;
        const bool out = !pos && !neg && e[i] < 0.0f;                                          // constant and outside
        klo = fmaxf(klo, pos ? lo : 0.0f);
        khi = out ? -1.0f : fminf(khi, neg ? hi : SPAN_NONE);
#else
        if (t[i] > (Step)0) klo = fmaxf(klo, lo);
        else if (t[i] < (Step)0) khi = fminf(khi, hi);
        else if (e[i] < 0.0f) khi = -1.0f;                                                     // constant and outside
#endif
    }
    k0 = (int32_t)klo; k1 = (int32_t)khi;
}

// e[i], t[i]: the edge values at step 0 and the steps per pixel, converted to float; n: the row's last step; rcp: float -> float.
template <typename Rcp>
SPAN_HD void span_bounds(const float (&e)[3], const float (&t)[3], int32_t n, Rcp rcp, int32_t& k0, int32_t& k1)
{
    const float r[3] = {rcp(t[0]), rcp(t[1]), rcp(t[2])};
    span_bounds_rcp(e, t, r, n, k0, k1);
}
