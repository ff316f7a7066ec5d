// Stand-alone check that chord_amd/csrc/span_bounds.h returns what it returned when its three cases per edge were an if / else-if
// ladder (built and run by tests/test_span_bounds_straight.py; no GPU, no python in the process).  ladder() below is a frozen copy
// of that form and the reference; for every row of the sweeps -- those of tests/span_bounds_main.cpp: the lattice of int32-kind
// triangles in a 64-px box, seeded triangles of all three kinds, raw edge values and steps up to 2^62 / 2^40 with crossings on
// pixel centres, at both clamp values and far off the row, zero steps with E <, ==, > 0, n = 0 and 63 -- and for the exact
// reciprocal and the exact one moved one ulp either way it asks for the SAME (k0, k1) of
//   span_bounds()       the helper as scan_row, scan_span_i32 and masked_rows call it
//   span_bounds_rcp()   the form that takes the reciprocals ready-made (the body of span_bounds(); no kernel calls it directly since
//                       the tile kernel variant that stored an entry's three once was rejected), with the steps as floats and as
//                       the integers they are (only their signs are read)
// Built with -DSPAN_SLACK_LEGACY=1 both sides return the earlier bounds.  Prints one line of counts; exit status 1 on a
// difference or when a case the sweep has to contain did not occur.
#include "span_bounds.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef __int128 i128;

enum Kind { K_I32 = 0, K_F64 = 1, K_I64 = 2 };

static struct {
    uint64_t rows, compared, differences;
    uint64_t onCentre, zeroNeg, zeroZero, zeroPos, farLeft, farRight, clampLo, clampHi, n0, n63, empty, assignBelow, nanQ;
    uint64_t perKind[3];
} S;

static uint64_t rngState = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17;
    return rngState;
}
static int64_t rndRange(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }
static i128 rndSigned(i128 lim) { const i128 v = (i128)(rnd() % (uint64_t)lim); return (rnd() & 1) ? -v : v; }     // |v| < lim <= 2^63

static i128 floorDiv(i128 a, i128 b)      // b > 0
{
    i128 q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

static float toFloat(Kind kind, i128 v)
{
    if (kind == K_I32) return (float)(int32_t)v;
    if (kind == K_F64) return (float)(double)(int64_t)v;
    return (float)(int64_t)v;
}

struct RcpExact { float operator()(float x) const { return 1.0f / x; } };
struct RcpUp { float operator()(float x) const { const float r = 1.0f / x; return isfinite(r) ? nextafterf(r, INFINITY) : r; } };
struct RcpDown { float operator()(float x) const { const float r = 1.0f / x; return isfinite(r) ? nextafterf(r, -INFINITY) : r; } };

// ---- the reference: span_bounds() as it stood before the selects, frozen -------------------------------------------------
template <typename Rcp>
static void ladder(const float (&e)[3], const float (&t)[3], int32_t n, Rcp rcp, int32_t& k0, int32_t& k1)
{
    float klo = 0.0f, khi = (float)n;
    for (int i = 0; i < 3; i++) {
        const float q = fminf(fmaxf(-e[i] * rcp(t[i]), -4.0f), 4096.0f);                      // NaN (0 * inf) -> -4
#if SPAN_SLACK_LEGACY
        if (t[i] > 0.0f) klo = fmaxf(klo, floorf(q) - 1.0f);
        else if (t[i] < 0.0f) khi = fminf(khi, floorf(q) + 1.0f);
#else
        if (t[i] > 0.0f) klo = fmaxf(klo, ceilf(q - 0.015625f));
        else if (t[i] < 0.0f) khi = fminf(khi, floorf(q + 0.015625f));
#endif
        else if (e[i] < 0.0f) khi = -1.0f;                                                     // constant and outside
    }
    k0 = (int32_t)klo; k1 = (int32_t)khi;
}

static void differ(const char* what, Kind kind, int r, int32_t n, int32_t k0, int32_t k1, int32_t w0, int32_t w1, const float (&e)[3], const float (&t)[3])
{
    if (S.differences++ < 8)
        fprintf(stderr, "DIFFERENT %s kind %d rcp %d n %d: k0 %d k1 %d, the ladder %d %d  e %a %a %a  t %a %a %a\n", what, (int)kind, r, n, k0, k1, w0, w1,
                e[0], e[1], e[2], t[0], t[1], t[2]);
}

template <typename Rcp>
static void compare(Kind kind, int r, const float (&e)[3], const float (&t)[3], const i128 st[3], int32_t n, Rcp rcp)
{
    int32_t w0, w1, k0, k1;
    ladder(e, t, n, rcp, w0, w1);
    span_bounds(e, t, n, rcp, k0, k1);
    if (k0 != w0 || k1 != w1) differ("span_bounds", kind, r, n, k0, k1, w0, w1, e, t);
    const float rc[3] = {rcp(t[0]), rcp(t[1]), rcp(t[2])};
    span_bounds_rcp(e, t, rc, n, k0, k1);
    if (k0 != w0 || k1 != w1) differ("span_bounds_rcp (float steps)", kind, r, n, k0, k1, w0, w1, e, t);
    if (kind == K_I32) {
        const int32_t ti[3] = {(int32_t)st[0], (int32_t)st[1], (int32_t)st[2]};
        span_bounds_rcp(e, ti, rc, n, k0, k1);
    } else {
        const int64_t ti[3] = {(int64_t)st[0], (int64_t)st[1], (int64_t)st[2]};
        span_bounds_rcp(e, ti, rc, n, k0, k1);
    }
    if (k0 != w0 || k1 != w1) differ("span_bounds_rcp (integer steps)", kind, r, n, k0, k1, w0, w1, e, t);
    S.compared += 3;
    if (w1 < w0) S.empty++;
}

static void checkRow(Kind kind, const i128 E[3], const i128 st[3], int32_t n)
{
    S.rows++; S.perKind[kind]++;
    if (n == 0) S.n0++;
    if (n == 63) S.n63++;
    bool below = false;          // an earlier edge has put the right bound below -1 ...
    for (int i = 0; i < 3; i++) {
        if (st[i] == 0) {
            if (E[i] < 0) { S.zeroNeg++; if (below) S.assignBelow++; }     // ... where the constant-and-outside case assigns -1, not min(khi, -1)
            else if (E[i] == 0) { S.zeroZero++; S.nanQ++; }
            else S.zeroPos++;
            continue;
        }
        const i128 a = st[i] < 0 ? -st[i] : st[i];
        if (E[i] % a == 0) { const i128 k = -E[i] / st[i]; if (k >= 0 && k <= n) S.onCentre++; }
        const i128 q4 = floorDiv(-E[i] * (st[i] < 0 ? -1 : 1), a);
        if (q4 < -4) S.clampLo++;
        if (q4 >= 4096) S.clampHi++;
        if (q4 < -64) S.farLeft++;
        if (q4 > (i128)n + 64) S.farRight++;
        if (st[i] < 0 && q4 < -3) below = true;
    }
    const float e[3] = {toFloat(kind, E[0]), toFloat(kind, E[1]), toFloat(kind, E[2])};
    const float t[3] = {toFloat(kind, st[0]), toFloat(kind, st[1]), toFloat(kind, st[2])};
    compare(kind, 0, e, t, st, n, RcpExact());
    compare(kind, 1, e, t, st, n, RcpUp());
    compare(kind, 2, e, t, st, n, RcpDown());
}

// A 24.8 triangle as the tile kernel sets it up (see tests/span_bounds_main.cpp): row py of the tile at pixel (ox, oy), steps 0 .. n from lx0.
static bool triangleRow(Kind kind, const int64_t X[3], const int64_t Y[3], int64_t ox, int64_t py, int64_t lx0, int32_t n)
{
    const i128 dx[3] = {X[2] - X[1], X[0] - X[2], X[1] - X[0]}, dy[3] = {Y[2] - Y[1], Y[0] - Y[2], Y[1] - Y[0]};
    const int64_t vx[3] = {X[1], X[2], X[0]}, vy[3] = {Y[1], Y[2], Y[0]};
    const i128 area2 = dx[2] * (i128)(Y[2] - Y[0]) - dy[2] * (i128)(X[2] - X[0]);
    if (area2 == 0) return false;
    const i128 s = area2 > 0 ? 1 : -1;
    const i128 cx = (i128)(ox + lx0) * 256 + 128, cy = (i128)py * 256 + 128;
    i128 E[3], st[3];
    for (int i = 0; i < 3; i++) {
        const i128 a = -s * dy[i], b = s * dx[i];
        const i128 bias = (a > 0 || (a == 0 && b > 0)) ? 0 : -1;
        E[i] = s * (dx[i] * (cy - vy[i]) - dy[i] * (cx - vx[i])) + bias;
        st[i] = a * 256;
    }
    checkRow(kind, E, st, n);
    return true;
}

static void latticeSweep()
{
    // vertices on a 12.5-px lattice inside a 64-px box: every second lattice line runs through pixel centres; vertical and
    // horizontal edges are zero steps
    const int G = 6; const int64_t pitch = 3200;
    for (int a = 0; a < G * G; a++) for (int b = 0; b < G * G; b++) for (int c = 0; c < G * G; c++) {
        const int64_t X[3] = {(a % G) * pitch, (b % G) * pitch, (c % G) * pitch}, Y[3] = {(a / G) * pitch, (b / G) * pitch, (c / G) * pitch};
        int64_t minX = X[0], maxX = X[0];
        for (int i = 1; i < 3; i++) { if (X[i] < minX) minX = X[i]; if (X[i] > maxX) maxX = X[i]; }
        const int64_t bx0 = minX >> 8, bx1 = (maxX >> 8) > 63 ? 63 : (maxX >> 8);
        for (int64_t py = 0; py < 64; py += 1 + (a + b + c) % 3) {
            if (!triangleRow(K_I32, X, Y, 0, py, bx0, (int32_t)(bx1 - bx0))) break;     // the bbox row
            if ((a + b + py) % 4 == 0) triangleRow(K_I32, X, Y, 0, py, 0, 63);           // the whole tile row
            if ((a + c + py) % 8 == 0) triangleRow(K_I32, X, Y, 0, py, 32, 31);          // the right half: crossings left of step 0
            if ((b + c + py) % 16 == 0) triangleRow(K_I32, X, Y, 0, py, (minX + maxX) >> 9, 0);   // one pixel
        }
    }
}

static void randomTriangles()
{
    for (int it = 0; it < 60000; it++) {                 // int32 kind: vertices at most 64 px apart, the tile within 64 px of them
        const int64_t bx = rndRange(-1000000, 1000000), by = rndRange(-1000000, 1000000), ext = rndRange(1, 16384);
        int64_t X[3], Y[3];
        for (int i = 0; i < 3; i++) { X[i] = bx + rndRange(0, ext); Y[i] = by + rndRange(0, ext); }
        if (it % 5 == 0) X[1] = X[0];                 // a vertical edge
        if (it % 7 == 0) Y[2] = Y[1];                 // a horizontal edge
        if (it % 11 == 0) for (int i = 0; i < 3; i++) { X[i] = (X[i] & ~255ll) | 128; Y[i] = (Y[i] & ~255ll) | 128; }   // on pixel centres
        const int64_t ox = (bx >> 8) - rndRange(0, 63), oy = (by >> 8) - rndRange(0, 63);
        for (int r = 0; r < 4; r++) {
            const int64_t lx0 = rndRange(0, 63); const int32_t n = r == 0 ? 0 : r == 1 ? 63 - (int32_t)lx0 : (int32_t)rndRange(0, 63 - lx0);
            triangleRow(K_I32, X, Y, ox, oy + rndRange(0, 63), lx0, n);
        }
    }
    for (int it = 0; it < 60000; it++) {                 // the wide kinds: vertices in +-2^24 (fp64) or +-2^29 (int64: |E| < 2^62) sub-pixels
        const Kind kind = (it & 1) ? K_F64 : K_I64;
        const int64_t lim = kind == K_F64 ? (1ll << 24) : (1ll << 29);
        int64_t X[3], Y[3];
        for (int i = 0; i < 3; i++) { X[i] = rndRange(-lim, lim); Y[i] = rndRange(-lim, lim); }
        if (it % 5 == 0) X[1] = X[0];
        if (it % 7 == 0) Y[2] = Y[1];
        if (it % 3 == 0) for (int i = 1; i < 3; i++) { X[i] = X[0] + rndRange(-60000, 60000); Y[i] = Y[0] + rndRange(-60000, 60000); }
        const int v = (int)(rnd() % 3);
        const int64_t w0 = rndRange(0, 256), w1 = rndRange(0, 256 - w0);
        int64_t px = (X[0] * w0 + X[1] * w1 + X[2] * (256 - w0 - w1)) >> 16, py = (Y[0] * w0 + Y[1] * w1 + Y[2] * (256 - w0 - w1)) >> 16;
        if (it % 4 == 0) { px = (X[v] >> 8) + rndRange(-100, 100); py = (Y[v] >> 8) + rndRange(-100, 100); }
        const int64_t ox = px - rndRange(0, 63);
        for (int r = 0; r < 4; r++) {
            const int64_t lx0 = rndRange(0, 63); const int32_t n = r == 0 ? 0 : r == 1 ? 63 - (int32_t)lx0 : (int32_t)rndRange(0, 63 - lx0);
            triangleRow(kind, X, Y, ox, py + r, lx0, n);
        }
    }
}

static void syntheticRows()
{
    // edge values and steps straight from their ranges: |E| up to 2^31 / 2^53 / 2^62, |step| up to 2^22 / 2^40 / 2^40 (a multiple of
    // 256), crossings on a step, beside one, far left, far right, at both clamp values; zero steps with E < 0, == 0, > 0
    for (int it = 0; it < 300000; it++) {
        const Kind kind = (Kind)(it % 3);
        const int eBits = kind == K_I32 ? 30 : kind == K_F64 ? 52 : 62, aBits = kind == K_I32 ? 14 : 32;
        const int32_t n = it % 13 == 0 ? 0 : it % 13 == 1 ? 63 : (int32_t)rndRange(0, 63);
        i128 E[3], st[3];
        for (int i = 0; i < 3; i++) {
            const i128 eLim = (i128)1 << rndRange(1, eBits);
            const int64_t aLim = 1ll << rndRange(0, aBits);
            const int mode = (int)(rnd() % 12);
            i128 a = rndRange(1, aLim);
            if (rnd() & 1) a = -a;
            const i128 bias = (rnd() & 1) ? -1 : 0;
            i128 e;
            if (mode == 0) a = 0;
            const i128 sA = a * 256;
            if (mode == 0) e = (rnd() % 3 == 0) ? 0 : rndSigned(eLim);
            else if (mode <= 3) e = -(i128)rndRange(-8, 72) * sA + (mode == 1 ? 0 : mode == 2 ? -bias : rndRange(-3, 3));     // on / beside a step
            else if (mode == 4) e = -(i128)(rnd() & 1 ? -4 : 4096) * sA + rndRange(-2, 2);                                 // at a clamp value
            else if (mode == 5) e = -(i128)rndRange(-200000, 200000) * sA + rndRange(-255, 255);                           // far left / right
            else if (mode == 6) e = 0;
            else e = rndSigned(eLim);
            const i128 cap = ((i128)1 << eBits) - 1;
            if (e > cap) e = cap;
            if (e < -cap) e = -cap;
            E[i] = e; st[i] = sA;
            if (kind == K_I32 && (E[i] + 64 * st[i] > cap * 2 || E[i] + 64 * st[i] < -cap * 2)) E[i] = 5;
        }
        checkRow(kind, E, st, n);
    }
}

int main()
{
    latticeSweep();
    randomTriangles();
    syntheticRows();
    printf("rows %llu compared %llu kinds %llu %llu %llu differences %llu empty %llu on_centre %llu zero_neg %llu zero_zero %llu zero_pos %llu "
           "assign_below %llu nan_q %llu far_left %llu far_right %llu clamp_lo %llu clamp_hi %llu n0 %llu n63 %llu\n",
           (unsigned long long)S.rows, (unsigned long long)S.compared, (unsigned long long)S.perKind[0], (unsigned long long)S.perKind[1],
           (unsigned long long)S.perKind[2], (unsigned long long)S.differences, (unsigned long long)S.empty, (unsigned long long)S.onCentre,
           (unsigned long long)S.zeroNeg, (unsigned long long)S.zeroZero, (unsigned long long)S.zeroPos, (unsigned long long)S.assignBelow,
           (unsigned long long)S.nanQ, (unsigned long long)S.farLeft, (unsigned long long)S.farRight, (unsigned long long)S.clampLo,
           (unsigned long long)S.clampHi, (unsigned long long)S.n0, (unsigned long long)S.n63);
    const bool complete = S.perKind[0] && S.perKind[1] && S.perKind[2] && S.empty && S.onCentre && S.zeroNeg && S.zeroZero && S.zeroPos &&
                          S.assignBelow && S.farLeft && S.farRight && S.clampLo && S.clampHi && S.n0 && S.n63;
    if (!complete) fprintf(stderr, "a case the sweep has to contain did not occur\n");
    return (S.differences || !complete) ? 1 : 0;
}
