// box_ray_check.cpp — the f32 box-ray setup of scheme-raytrace_amd/csrc/rt_boxray.h (1/d from the f32-rounded
// direction within an ulp, clamped at +-1e30; o/d as one f32 product) must stay a conservative cull: whenever
// the exact slab interval of a ray against an f64 box meets [0, t], the f32 slab test of the BVH walks
// (node_hit, rt_kernels.hip: t = fma(plane, 1/d, -o/d), near <= far within [0, f32_up(t)]) on the box as
// commit stores it (widened by 2^EXP R, planes rounded outward: flatten_bvh2) must report a hit.
//
//   exact    long double, on the unwidened f64 box; a zero direction component: the slab is all t if the
//            origin is inside it (planes included), else empty
//   f32      three times: the host's reciprocal as computed, then moved one ulp up and one ulp down on all
//            axes (the host's 1.0f / x is not the device's v_rcp_f32, which is within one ulp)
//   inputs   2^20 seeded triples of box, origin and direction per R, and adversarial families:
//            direction components +-0, subnormal (f64 and f32), 2^-126, 1e-30 and 1e30; origins on box
//            planes; origins at |o| = R; boxes at +-R; rays through a box corner or an edge point
//   R        1000 (a cover scene) and 555 sqrt(3) (a Cornell scene)
// usage: box_ray_check [EXP = -21]; prints per R "R cases hits culled", then "cases hits culled"; exit status 1
// if any hit was culled.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../scheme-raytrace_amd/csrc/rt_boxray.h"

using rtamd::BoxRay;

static uint64_t g_state = 0x5EED0B0Cull;
static uint64_t rnd() {                                    // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(rnd() >> 11) * 0x1p-53; }            // [0, 1)
static double sym() { return 2.0 * uni() - 1.0; }                           // [-1, 1)
static int pick(const int n) { return (int)(rnd() % (uint64_t)n); }

static float f32_down(const double x) { float f = (float)x; return (double)f > x ? nextafterf(f, -INFINITY) : f; }
static float f32_up(const double x) { float f = (float)x; return (double)f < x ? nextafterf(f, INFINITY) : f; }

struct Case { double lo[3], hi[3], o[3], d[3], t; };

static bool exact_hit(const Case& c) {
    long double tn = 0.0L, tf = (long double)c.t;
    for (int k = 0; k < 3; ++k) {
        if (c.d[k] == 0.0) {
            if (c.o[k] < c.lo[k] || c.o[k] > c.hi[k]) return false;
            continue;
        }
        const long double a = ((long double)c.lo[k] - c.o[k]) / c.d[k], b = ((long double)c.hi[k] - c.o[k]) / c.d[k];
        tn = fmaxl(tn, fminl(a, b));
        tf = fminl(tf, fmaxl(a, b));
    }
    return tn <= tf;
}

// node_hit's test of one box (rt_kernels.hip), on the widened f32 planes wl, wh
static bool f32_hit(const float* wl, const float* wh, const BoxRay& r, const float tcap) {
    const float tx0 = fmaf(wl[0], r.ix, -r.px), tx1 = fmaf(wh[0], r.ix, -r.px);
    const float ty0 = fmaf(wl[1], r.iy, -r.py), ty1 = fmaf(wh[1], r.iy, -r.py);
    const float tz0 = fmaf(wl[2], r.iz, -r.pz), tz1 = fmaf(wh[2], r.iz, -r.pz);
    const float tn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), 0.0f));
    const float tf = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fminf(fmaxf(tz0, tz1), tcap));
    return tn <= tf;
}

static long cases = 0, hits = 0, culled = 0;

static void check(const Case& c, const double margin, const char* family) {
    ++cases;
    if (!exact_hit(c)) return;
    ++hits;
    float wl[3], wh[3];
    for (int k = 0; k < 3; ++k) { wl[k] = f32_down(c.lo[k] - margin); wh[k] = f32_up(c.hi[k] + margin); }
    const float tcap = f32_up(c.t);
    for (int move = 0; move < 3; ++move) {
        float i[3];
        for (int k = 0; k < 3; ++k) {
            float r = rtamd::box_rcp((float)c.d[k]);
            if (move == 1) r = nextafterf(r, INFINITY);
            if (move == 2) r = nextafterf(r, -INFINITY);
            i[k] = rtamd::box_clamp(r);
        }
        const BoxRay br = rtamd::box_ray_inv(c.o[0], c.o[1], c.o[2], i[0], i[1], i[2]);
        if (!f32_hit(wl, wh, br, tcap)) {
            if (culled < 8)
                printf("culled (%s, reciprocal %s): box [%.17g %.17g %.17g] [%.17g %.17g %.17g] o %.17g %.17g %.17g "
                       "d %.17g %.17g %.17g t %.17g\n", family, move == 0 ? "as computed" : move == 1 ? "+1 ulp" : "-1 ulp",
                       c.lo[0], c.lo[1], c.lo[2], c.hi[0], c.hi[1], c.hi[2], c.o[0], c.o[1], c.o[2], c.d[0], c.d[1],
                       c.d[2], c.t);
            ++culled;
            return;
        }
    }
}

// a box inside [-lim, lim]^3, half sizes from 1e-3 up to lim / 2 (log-uniform)
static void random_box(Case& c, const double lim) {
    for (int k = 0; k < 3; ++k) {
        const double h = fmin(1e-3 * pow(lim / 2e-3, uni()), lim / 2), m = sym() * (lim - h);
        c.lo[k] = m - h; c.hi[k] = m + h;
    }
}
// an origin with |o| <= R: a point of the ball, or near the box
static void random_origin(Case& c, const double R) {
    double n2;
    do { n2 = 0; for (int k = 0; k < 3; ++k) { c.o[k] = sym() * R; n2 += c.o[k] * c.o[k]; } } while (n2 > R * R);
    if (pick(4) == 0)                                      // within two box sizes of the box (kept inside R)
        for (int k = 0; k < 3; ++k) {
            const double v = 0.5 * (c.lo[k] + c.hi[k]) + sym() * 2.5 * (c.hi[k] - c.lo[k]);
            if (fabs(v) < R / 2) c.o[k] = v;
        }
}
static void point_in_box(const Case& c, double* p) { for (int k = 0; k < 3; ++k) p[k] = c.lo[k] + uni() * (c.hi[k] - c.lo[k]); }
// a direction towards p (exactly p - o), or just past the box; scaled by 2^-40 .. 2^40; t: no cap, t-max,
// or either side of the distance to p
static void aim(Case& c, const double* p, const bool exactly) {
    const double s = ldexp(1.0, pick(81) - 40);
    for (int k = 0; k < 3; ++k) {
        c.d[k] = p[k] - c.o[k];
        if (!exactly) c.d[k] += sym() * 0.75 * (c.hi[k] - c.lo[k]);
    }
    for (int k = 0; k < 3; ++k) c.d[k] *= s;
    const int w = pick(4);
    c.t = w == 0 ? INFINITY : w == 1 ? 999999999999.0 : (1.0 / s) * (w == 2 ? 1.0 + sym() * 0x1p-20 : 0.5 + uni());
}

static void run(const double R, const int exp2) {
    const double margin = ldexp(R, exp2);
    const long c0 = cases, h0 = hits, b0 = culled;
    double p[3];
    // 2^20 seeded triples: boxes where commit puts them (inside R / 4: scene_radius is 4 x the geometry's) and,
    // for a quarter of the triples, anywhere inside R
    for (long n = 0; n < (1L << 20); ++n) {
        Case c;
        random_box(c, n % 4 == 3 ? R : R / 4);
        random_origin(c, R);
        point_in_box(c, p);
        aim(c, p, n % 2 == 0);
        check(c, margin, "random");
    }
    static const double tiny[] = {0.0, 4.9406564584124654e-324, 1e-310, 1e-40, 0x1p-126, 1e-30};
    for (long n = 0; n < (1L << 17); ++n) {
        Case c;
        // direction components +-0, subnormal, 2^-126, 1e-30 (one or two axes), origin inside or outside that slab
        random_box(c, R / 4); random_origin(c, R); point_in_box(c, p); aim(c, p, true);
        for (int j = 0, na = 1 + pick(2); j < na; ++j) {
            const int k = pick(3);
            c.d[k] = (pick(2) ? -1.0 : 1.0) * tiny[pick(6)];
            if (pick(2)) c.o[k] = p[k];
            if (pick(4) == 0) c.o[k] = pick(2) ? c.lo[k] : c.hi[k];
        }
        check(c, margin, "tiny direction component");
        // ... and 1e30 (the other components as aimed, or as large)
        random_box(c, R / 4); random_origin(c, R); point_in_box(c, p); aim(c, p, true);
        {
            int k = pick(3);
            const bool all = pick(2) == 0;                // the whole direction scaled: its largest component at 1e30
            if (all) for (int a = 0; a < 3; ++a) if (fabs(c.d[a]) > fabs(c.d[k])) k = a;
            const double big = (c.d[k] < 0 ? -1e30 : 1e30);
            if (all && c.d[k] != 0.0) { const double s = big / c.d[k]; for (int a = 0; a < 3; ++a) c.d[a] *= s; c.t = INFINITY; }
            c.d[k] = big;
        }
        check(c, margin, "1e30 direction component");
        // origins on box planes (one to three of them), heading in, out or along
        random_box(c, R / 4); random_origin(c, R); point_in_box(c, p);
        for (int k = 0; k < 3; ++k) c.o[k] = p[k];
        for (int j = 0, na = 1 + pick(3); j < na; ++j) { const int k = pick(3); c.o[k] = pick(2) ? c.lo[k] : c.hi[k]; }
        point_in_box(c, p);
        if (pick(2)) for (int k = 0; k < 3; ++k) p[k] += sym() * (c.hi[k] - c.lo[k]);
        aim(c, p, true);
        if (pick(3) == 0) c.d[pick(3)] = pick(2) ? 0.0 : -0.0;
        check(c, margin, "origin on a box plane");
        // origins at |o| = R
        random_box(c, R / 4);
        {
            double u[3], n2 = 0;
            for (int k = 0; k < 3; ++k) { u[k] = sym(); n2 += u[k] * u[k]; }
            if (pick(4) == 0) { const int k = pick(3); for (int a = 0; a < 3; ++a) u[a] = a == k ? (u[a] < 0 ? -1 : 1) : 0; n2 = 1; }
            for (int k = 0; k < 3; ++k) c.o[k] = R * u[k] / sqrt(n2);
        }
        point_in_box(c, p); aim(c, p, pick(2) == 0);
        check(c, margin, "|o| = R");
        // boxes at +-R: a plane (or the whole box) pushed out to the radius
        random_box(c, R); random_origin(c, R);
        for (int j = 0, na = 1 + pick(3); j < na; ++j) {
            const int k = pick(3);
            const double w = c.hi[k] - c.lo[k];
            if (pick(2)) { c.hi[k] = R; if (pick(2)) c.lo[k] = R - w; }
            else { c.lo[k] = -R; if (pick(2)) c.hi[k] = -R + w; }
        }
        point_in_box(c, p); aim(c, p, pick(2) == 0);
        check(c, margin, "box at +-R");
        // grazing: through a corner, or through a point of an edge (the ray's exact interval is one t, or none)
        random_box(c, pick(4) == 3 ? R : R / 4); random_origin(c, R);
        {
            const int free_axis = pick(2) ? pick(3) : -1;
            for (int k = 0; k < 3; ++k) p[k] = k == free_axis ? c.lo[k] + uni() * (c.hi[k] - c.lo[k]) : pick(2) ? c.lo[k] : c.hi[k];
        }
        aim(c, p, true);
        if (pick(2)) c.t = pick(2) ? INFINITY : 999999999999.0;
        check(c, margin, "grazing an edge or a corner");
    }
    printf("%.17g %ld %ld %ld\n", R, cases - c0, hits - h0, culled - b0);
}

int main(int argc, char** argv) {
    const int exp2 = argc > 1 ? atoi(argv[1]) : -21;
    run(1000.0, exp2);
    run(555.0 * sqrt(3.0), exp2);
    printf("%ld %ld %ld\n", cases, hits, culled);
    return culled ? 1 : 0;
}
