// Stand-alone check of chord_amd/csrc/span_bounds.h on the host (built and run by tests/test_span_bounds.py; no GPU, no python
// in the process).  For every row it is given -- three exact integer edge values at step 0, three integer steps, the last step n --
// it computes the covered steps from the integers alone and asks of span_bounds(), with the exact reciprocal and with the exact
// one moved one ulp either way (v_rcp_f32 is a 1-ulp approximation; the host's division is not that instruction):
//   safe    k0 <= first covered step and k1 >= last covered step
//   tight   the loop k0 .. k1 is at most 2 steps longer than the interval the integer crossings give, at most 1 at either end
// Built with -DSPAN_SLACK_LEGACY=1 the second condition is not asked (the earlier bounds are 1 - 2 steps wide at either end).
// Prints one line of counts; exit status 1 on a violation or when a case the sweep has to contain did not occur.
#include "span_bounds.h"

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef __int128 i128;

enum Kind { K_I32 = 0, K_F64 = 1, K_I64 = 2 };

static struct {
    uint64_t rows, coveredRows, violations, loose;
    uint64_t onCentreBiased, onCentreUnbiased, zeroNeg, zeroZero, zeroPos, zeroAtStart, farLeft, farRight, clampLo, clampHi, n0, n63;
    uint64_t perKind[3];
    int64_t maxExcess;
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
static i128 ceilDiv(i128 a, i128 b) { return -floorDiv(-a, b); }

static float toFloat(Kind kind, i128 v)
{
    if (kind == K_I32) return (float)(int32_t)v;
    if (kind == K_F64) return (float)(double)(int64_t)v;      // |v| < 2^53: the double is exact, one rounding to float
    return (float)(int64_t)v;
}

struct RcpExact { float operator()(float x) const { return 1.0f / x; } };
struct RcpUp { float operator()(float x) const { const float r = 1.0f / x; return isfinite(r) ? nextafterf(r, INFINITY) : r; } };
struct RcpDown { float operator()(float x) const { const float r = 1.0f / x; return isfinite(r) ? nextafterf(r, -INFINITY) : r; } };

// unbiased[i]: the edge value without its top-left bias (E[i] or E[i] + 1); only for the counts of crossings on a pixel centre
static void checkRow(Kind kind, const i128 E[3], const i128 st[3], const i128 unbiased[3], int32_t n)
{
    // the covered steps, from the integers: by definition ...
    int32_t first = -1, last = -1;
    for (int32_t k = 0; k <= n; k++) {
        bool in = true;
        for (int i = 0; i < 3; i++) in = in && (E[i] + (i128)k * st[i] >= 0);
        if (in) { if (first < 0) first = k; last = k; }
    }
    // ... and as the interval of the integer crossings (what the bounds estimate); lo / hi are clamped only to stay small numbers
    i128 lo = 0, hi = n;
    for (int i = 0; i < 3; i++) {
        if (st[i] > 0) { const i128 c = ceilDiv(-E[i], st[i]); if (c > lo) lo = c; }
        else if (st[i] < 0) { const i128 f = floorDiv(E[i], -st[i]); if (f < hi) hi = f; }
        else if (E[i] < 0) hi = -1;
    }
    if (lo > 100000) lo = 100000;
    if (hi < -100000) hi = -100000;
    if (lo <= hi) {
        if (first != (int32_t)lo || last != (int32_t)hi) { fprintf(stderr, "reference disagrees with itself\n"); exit(2); }
    } else if (first >= 0) { fprintf(stderr, "reference disagrees with itself (empty)\n"); exit(2); }
    const int64_t span = lo <= hi ? (int64_t)(hi - lo + 1) : 0;

    S.rows++; S.perKind[kind]++;
    if (first >= 0) S.coveredRows++;
    if (n == 0) S.n0++;
    if (n == 63) S.n63++;
    for (int i = 0; i < 3; i++) {
        if (st[i] == 0) { if (E[i] < 0) S.zeroNeg++; else if (E[i] == 0) S.zeroZero++; else S.zeroPos++; continue; }
        if (E[i] == 0) S.zeroAtStart++;
        const i128 a = st[i] < 0 ? -st[i] : st[i];
        if (E[i] % a == 0) { const i128 k = -E[i] / st[i]; if (k >= 0 && k <= n) S.onCentreBiased++; }
        if (unbiased[i] % a == 0) { const i128 k = -unbiased[i] / st[i]; if (k >= 0 && k <= n) S.onCentreUnbiased++; }
        // the crossing as a real number, against the row and against the clamp of q to [-4, 4096]
        const i128 q4 = floorDiv(-E[i] * (st[i] < 0 ? -1 : 1), a);
        if (q4 < -4) S.clampLo++;
        if (q4 >= 4096) S.clampHi++;
        if (q4 < -64) S.farLeft++;
        if (q4 > (i128)n + 64) S.farRight++;
    }

    const float e[3] = {toFloat(kind, E[0]), toFloat(kind, E[1]), toFloat(kind, E[2])};
    const float t[3] = {toFloat(kind, st[0]), toFloat(kind, st[1]), toFloat(kind, st[2])};
    for (int r = 0; r < 3; r++) {
        int32_t k0, k1;
        if (r == 0) span_bounds(e, t, n, RcpExact(), k0, k1);
        else if (r == 1) span_bounds(e, t, n, RcpUp(), k0, k1);
        else span_bounds(e, t, n, RcpDown(), k0, k1);
        bool bad = k0 < 0 || k1 > n;                                   // the loop stays inside the row
        if (first >= 0) bad = bad || k0 > first || k1 < last;          // ... and cuts no covered step
        if (bad) {
            if (S.violations++ < 8)
                fprintf(stderr, "UNSAFE kind %d rcp %d n %d: k0 %d k1 %d covered %d..%d  e %a %a %a  t %a %a %a\n", (int)kind, r, n, k0, k1,
                        first, last, e[0], e[1], e[2], t[0], t[1], t[2]);
        }
#if !SPAN_SLACK_LEGACY
        const int64_t scanned = k1 >= k0 ? (int64_t)k1 - k0 + 1 : 0;
        bool loose = scanned > span + 2;
        if (lo <= hi) loose = loose || (int64_t)lo - k0 > 1 || k1 - (int64_t)hi > 1;
        if (scanned - span > S.maxExcess) S.maxExcess = scanned - span;
        if (loose) {
            if (S.loose++ < 8)
                fprintf(stderr, "LOOSE kind %d rcp %d n %d: k0 %d k1 %d crossings %lld..%lld  e %a %a %a  t %a %a %a\n", (int)kind, r, n, k0, k1,
                        (long long)lo, (long long)hi, e[0], e[1], e[2], t[0], t[1], t[2]);
        }
#endif
    }
}

// A 24.8 triangle as the tile kernel sets it up (entry_store / entry_unit, scan_row): edge i opposite vertex i, the orientation
// folded in, the top-left bias folded in, steps of 256 sub-pixels.  Row py of the tile at pixel (ox, oy), steps 0 .. n from pixel lx0.
static bool triangleRow(Kind kind, const int64_t X[3], const int64_t Y[3], int64_t ox, int64_t py, int64_t lx0, int32_t n)
{
    const i128 dx[3] = {X[2] - X[1], X[0] - X[2], X[1] - X[0]}, dy[3] = {Y[2] - Y[1], Y[0] - Y[2], Y[1] - Y[0]};
    const int64_t vx[3] = {X[1], X[2], X[0]}, vy[3] = {Y[1], Y[2], Y[0]};
    const i128 area2 = dx[2] * (i128)(Y[2] - Y[0]) - dy[2] * (i128)(X[2] - X[0]);
    if (area2 == 0) return false;
    const i128 s = area2 > 0 ? 1 : -1;
    const i128 cx = (i128)(ox + lx0) * 256 + 128, cy = (i128)py * 256 + 128;
    i128 E[3], st[3], U[3];
    i128 sum = 0;
    for (int i = 0; i < 3; i++) {
        const i128 a = -s * dy[i], b = s * dx[i];
        const i128 bias = (a > 0 || (a == 0 && b > 0)) ? 0 : -1;
        U[i] = s * (dx[i] * (cy - vy[i]) - dy[i] * (cx - vx[i]));
        E[i] = U[i] + bias;
        st[i] = a * 256;
        sum += U[i];
    }
    if (sum <= 0) { fprintf(stderr, "orientation\n"); exit(2); }     // the three unbiased edge values sum to twice the area
    checkRow(kind, E, st, U, n);
    return true;
}

static void latticeSweep()
{
    // vertices on a 12.5-px lattice inside a 64-px box (0, 12.5, 25, ... 62.5 px): every second lattice line runs through pixel
    // centres, so edges cross rows exactly on centres, with both bias values; vertical and horizontal edges are zero steps
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
    // int32 kind: vertices at most 64 px apart, the tile anywhere within 64 px of them
    for (int it = 0; it < 60000; it++) {
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
    // the wide kinds: vertices anywhere in +-2^24 (fp64 kind) or +-2^29 (int64 kind: |E| < 2^62) sub-pixels, the tile on or near the triangle
    for (int it = 0; it < 60000; it++) {
        const Kind kind = (it & 1) ? K_F64 : K_I64;
        const int64_t lim = kind == K_F64 ? (1ll << 24) : (1ll << 29);
        int64_t X[3], Y[3];
        for (int i = 0; i < 3; i++) { X[i] = rndRange(-lim, lim); Y[i] = rndRange(-lim, lim); }
        if (it % 5 == 0) X[1] = X[0];
        if (it % 7 == 0) Y[2] = Y[1];
        if (it % 3 == 0) for (int i = 1; i < 3; i++) { X[i] = X[0] + rndRange(-60000, 60000); Y[i] = Y[0] + rndRange(-60000, 60000); }   // a few hundred px
        const int v = (int)(rnd() % 3);
        const int64_t w0 = rndRange(0, 256), w1 = rndRange(0, 256 - w0);          // a point of the triangle (or, every 4th, anywhere near)
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
    // 256), crossings placed on purpose: exactly on a step (with and without the bias), just beside one, far left, far right, at
    // both clamp values; zero steps with E < 0, == 0, > 0
    for (int it = 0; it < 300000; it++) {
        const Kind kind = (Kind)(it % 3);
        const int eBits = kind == K_I32 ? 30 : kind == K_F64 ? 52 : 62, aBits = kind == K_I32 ? 14 : 32;
        const int32_t n = it % 13 == 0 ? 0 : it % 13 == 1 ? 63 : (int32_t)rndRange(0, 63);
        i128 E[3], st[3], U[3];
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
            U[i] = e - bias; E[i] = e; st[i] = sA;
            if (kind == K_I32 && (E[i] + 64 * st[i] > cap * 2 || E[i] + 64 * st[i] < -cap * 2)) { E[i] = U[i] = 5; }
        }
        checkRow(kind, E, st, U, n);
    }
}

int main()
{
    latticeSweep();
    randomTriangles();
    syntheticRows();
    printf("rows %llu covered %llu kinds %llu %llu %llu violations %llu loose %llu max_excess %lld on_centre_biased %llu on_centre_unbiased %llu "
           "zero_neg %llu zero_zero %llu zero_pos %llu zero_at_start %llu far_left %llu far_right %llu clamp_lo %llu clamp_hi %llu n0 %llu n63 %llu\n",
           (unsigned long long)S.rows, (unsigned long long)S.coveredRows, (unsigned long long)S.perKind[0], (unsigned long long)S.perKind[1],
           (unsigned long long)S.perKind[2], (unsigned long long)S.violations, (unsigned long long)S.loose, (long long)S.maxExcess,
           (unsigned long long)S.onCentreBiased, (unsigned long long)S.onCentreUnbiased, (unsigned long long)S.zeroNeg,
           (unsigned long long)S.zeroZero, (unsigned long long)S.zeroPos, (unsigned long long)S.zeroAtStart, (unsigned long long)S.farLeft,
           (unsigned long long)S.farRight, (unsigned long long)S.clampLo, (unsigned long long)S.clampHi, (unsigned long long)S.n0,
           (unsigned long long)S.n63);
    const bool complete = S.coveredRows && S.perKind[0] && S.perKind[1] && S.perKind[2] && S.onCentreBiased && S.onCentreUnbiased && S.zeroNeg &&
                          S.zeroZero && S.zeroPos && S.zeroAtStart && S.farLeft && S.farRight && S.clampLo && S.clampHi && S.n0 && S.n63;
    if (!complete) fprintf(stderr, "a case the sweep has to contain did not occur\n");
    return (S.violations || S.loose || !complete) ? 1 : 0;
}
