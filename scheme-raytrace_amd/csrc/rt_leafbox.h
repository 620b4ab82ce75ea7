// rt_leafbox.h — world-space bounding boxes of flattened leaves for the world BVH (rt_build.cpp): the
// primitive's own box taken through its instance chain.  Host code only (no device code, no HIP):
// tests/csrc/bvh_generic_check.cpp compiles it with g++.
#pragma once
#include <algorithm>
#include <cmath>

#include "rt_device.h"

namespace rtamd {

// What a leaf's box depends on: a sphere (c0, r), a moving sphere (c0, c1, r, t0, t1) or an axis rect
// (a0..a1 x b0..b1 at k; XY: k on z, XZ: k on y, YZ: k on x), or a triangle (its vertices v0, v1, v2).
struct LeafGeom {
    int type;                          // LeafType
    double c0[3], c1[3], r, t0, t1;
    double a0, a1, b0, b1, k;
    double v[9];                       // LEAF_TRI
};

// The primitive's own box in its local frame.  A moving sphere is bounded over the times [tlo, thi] a
// ray can carry (the camera shutter and 0; tlo = thi = 0 for the time-0 tree); a degenerate shutter
// gives an unbounded box.
inline void leaf_local_box(const LeafGeom& g, const double tlo, const double thi, double* lo, double* hi) {
    const double rad = std::fabs(g.r);
    if (g.type == LEAF_SPHERE) {
        for (int k = 0; k < 3; ++k) { lo[k] = g.c0[k] - rad; hi[k] = g.c0[k] + rad; }
    } else if (g.type == LEAF_MSPHERE) {
        const double den = g.t1 - g.t0;
        if (!(den != 0.0) || !std::isfinite(den)) {
            for (int k = 0; k < 3; ++k) { lo[k] = -1e300; hi[k] = 1e300; }
        } else {
            const double f0 = (tlo - g.t0) / den, f1 = (thi - g.t0) / den;
            for (int k = 0; k < 3; ++k) {
                const double dc = g.c1[k] - g.c0[k];
                const double a = g.c0[k] + dc * f0, b = g.c0[k] + dc * f1;
                lo[k] = std::min(a, b) - rad; hi[k] = std::max(a, b) + rad;
            }
        }
    } else if (g.type == LEAF_TRI) {
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(g.v[k], std::min(g.v[3 + k], g.v[6 + k]));
            hi[k] = std::max(g.v[k], std::max(g.v[3 + k], g.v[6 + k]));
        }
    } else {
        const int ia = g.type == LEAF_RECT_YZ ? 1 : 0, ib = g.type == LEAF_RECT_XY ? 1 : 2;
        const int ik = 3 - ia - ib;
        lo[ia] = std::min(g.a0, g.a1); hi[ia] = std::max(g.a0, g.a1);
        lo[ib] = std::min(g.b0, g.b1); hi[ib] = std::max(g.b0, g.b1);
        lo[ik] = hi[ik] = g.k;
    }
}

// A local point out of the instance chain, innermost op first (chain_hit's order and operations).
inline void chain_point(const ChainOpRec* ops, const int n, double* p) {
    for (int k = n - 1; k >= 0; --k) {
        const ChainOpRec& op = ops[k];
        if (op.op == OP_TRANSLATE) {
            p[0] += op.x; p[1] += op.y; p[2] += op.z;
        } else {
            const double sn = op.x, cs = op.y;
            const double x = cs * p[0] + sn * p[2], z = (-sn) * p[0] + cs * p[2];
            p[0] = x; p[2] = z;
        }
    }
}

// The box of a local box's 8 corners taken out of the chain.  (The library's own conservative box: the
// reference's rotate-y keeps a wrong minimum, geometry.scm:489-510, which is not reproduced.)  A box
// that encloses its corners encloses the convex body between them, so rects are bounded exactly and
// spheres by their local box's image.
inline void chain_box(const ChainOpRec* ops, const int n, double* lo, double* hi) {
    if (n <= 0) return;
    double wlo[3] = {INFINITY, INFINITY, INFINITY}, whi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int c = 0; c < 8; ++c) {
        double p[3] = {(c & 1) ? hi[0] : lo[0], (c & 2) ? hi[1] : lo[1], (c & 4) ? hi[2] : lo[2]};
        chain_point(ops, n, p);
        for (int k = 0; k < 3; ++k) {
            bad = bad || std::isnan(p[k]);
            wlo[k] = std::min(wlo[k], p[k]); whi[k] = std::max(whi[k], p[k]);
        }
    }
    for (int k = 0; k < 3; ++k) { lo[k] = bad ? NAN : wlo[k]; hi[k] = bad ? NAN : whi[k]; }
}

// A leaf's world-space box, widened by pad (relative 1e-8 of its largest coordinate, pad_box's rule, which
// also covers the rounding of the chain's operations).  Returns false — "not a tree leaf" — when the box is
// not finite (or too large for the pad to be finite): such a leaf stays in its brute-force group.
inline bool leaf_world_box(const LeafGeom& g, const ChainOpRec* ops, const int n_ops, const double tlo,
                           const double thi, double* lo, double* hi) {
    // (std::min / std::max drop a NaN operand: the primitive's own numbers are checked first)
    bool fin = true;
    if (g.type == LEAF_SPHERE || g.type == LEAF_MSPHERE) {
        for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(g.c0[k]) && (g.type == LEAF_SPHERE || std::isfinite(g.c1[k]));
        fin = fin && std::isfinite(g.r) && (g.type == LEAF_SPHERE || (std::isfinite(g.t0) && std::isfinite(g.t1)));
    } else if (g.type == LEAF_TRI) {
        for (int k = 0; k < 9; ++k) fin = fin && std::isfinite(g.v[k]);
    } else {
        fin = std::isfinite(g.a0) && std::isfinite(g.a1) && std::isfinite(g.b0) && std::isfinite(g.b1) && std::isfinite(g.k);
    }
    if (!fin) return false;
    if (g.type == LEAF_TRI && n_ops > 0) {
        // a triangle is the convex hull of its vertices: the box of the three taken out of the chain (as a
        // rect's box is that of its corners), tighter under a rotation than the image of its local box
        for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
        for (int i = 0; i < 3; ++i) {
            double p[3] = {g.v[3 * i], g.v[3 * i + 1], g.v[3 * i + 2]};
            chain_point(ops, n_ops, p);
            for (int k = 0; k < 3; ++k) {
                if (std::isnan(p[k])) return false;
                lo[k] = std::min(lo[k], p[k]); hi[k] = std::max(hi[k], p[k]);
            }
        }
    } else {
        leaf_local_box(g, tlo, thi, lo, hi);
        chain_box(ops, n_ops, lo, hi);
    }
    double m = 1.0;
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k]) || !(lo[k] <= hi[k])) return false;
        m = std::max(m, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
    }
    if (!(m < 1e290)) return false;
    const double pad = 1e-8 * m;
    for (int k = 0; k < 3; ++k) { lo[k] -= pad; hi[k] += pad; }
    return true;
}

}  // namespace rtamd
