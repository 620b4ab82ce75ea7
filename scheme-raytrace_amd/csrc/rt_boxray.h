// rt_boxray.h — a ray's constants for the f32 slab test of the BVH walks: per axis 1/d and o/d, so that
// a box plane B is crossed at t = fma(B, 1/d, -o/d).
//
// Plain C++ for the device and the host alike (tests/csrc/box_ray_check.cpp compiles it with g++ and
// passes its own reciprocal, the host's moved an ulp each way).
//
// All of it is f32: the direction and the origin are rounded to f32, the reciprocal is the hardware's
// (v_rcp_f32, 1 ulp), the product o * (1/d) is one f32 multiply.  (The f64 form it replaces, three IEEE
// divisions, f64 clamps and six conversions, was about 65 wave instructions per ray for three numbers
// the slab test then uses in f32.)  The test is only a cull, so all that matters is that its rounding
// stays inside the margin the boxes were widened by at commit (rt_build.cpp world_tree):
//
//   u = 2^-24 (half an f32 ulp, relative).  Per axis, exactly: t* = (B - o) / d.  Computed:
//     df = d (1 + e1)                    |e1| <= u / m      d = +-m 2^k, m in [1, 2)
//     i  = (1 / df) (1 + e2)             |e2| <= u m        one ulp of a result with mantissa 2 / m
//     of = o (1 + e3)                    |e3| <= u
//     p  = of i (1 + e4)                 |e4| <= u
//     t  = (B i - p) (1 + e5)            |e5| <= u          (the node test's fma)
//   so  t = ((B - o) / d) (1 + e1' + e2 + e5) - (o / d) (e3 + e4) + O(u^2), and
//     |t - t*| |d| <= |B - o| (1 / m + m + 1) u + |o| 2 u <= 3.5 u |B - o| + 2 u |o|.
//   With every origin inside the scene radius, |o| <= R, and every box inside a quarter of it (R = 4 x
//   the geometry's radius + 1, scene_radius; the margin itself is 2^-21 R), |B - o| <= 1.25 R + 2^-21 R:
//     |t - t*| |d| <= (3.5 x 1.25 + 2) u R = 6.4 u R < 8 u R = 2^-21 R, the margin: 1.25x above the bound
//   (the f64 form's bound was 2 u (|B| + |o|) = 2.5 u R).  With the reciprocal another ulp off, as the
//   host check moves it, the first factor is 1 / m + 1.5 m + 1 <= 4.5 u and the bound 7.6 u R.
//   The planes themselves are rounded outward after the margin is added (flatten_bvh2).
//
// A component too small for its reciprocal (zero, subnormal, below 1e-30) takes +-1e30 with the
// component's sign, as before (slab_off reads the sign): the slab of an origin inside it then spans
// (-m 1e30, m 1e30) for the margin m, beyond any t a walk is asked for (kTmax = 1e12).
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define RT_BOXRAY_FN __host__ __device__ __forceinline__
#else
#define RT_BOXRAY_FN inline
#endif

namespace rtamd {

struct BoxRay { float ix, iy, iz, px, py, pz; };     // 1/d and o/d

// the reciprocal of an f32 component within one ulp: v_rcp_f32 on the device (a subnormal component
// gives +-inf or a number above the clamp, either way +-1e30 below)
RT_BOXRAY_FN float box_rcp(const float d) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_rcpf(d);
#else
    return 1.0f / d;
#endif
}
// a reciprocal kept within +-1e30; +-inf (a +-0 component) keeps its sign, and a NaN component gives
// +1e30 as the f64 form's fmax(fmin()) did (minNum: a ray with a NaN in dir still has to answer as the
// list does), which is why this is not one v_med3_f32
RT_BOXRAY_FN float box_clamp(const float i) { return fmaxf(fminf(i, 1e30f), -1e30f); }
// the box ray from the clamped reciprocals of the f32-rounded direction
RT_BOXRAY_FN BoxRay box_ray_inv(const double ox, const double oy, const double oz, const float ix, const float iy,
                                const float iz) {
    BoxRay b;
    b.ix = ix; b.iy = iy; b.iz = iz;
    b.px = (float)ox * ix; b.py = (float)oy * iy; b.pz = (float)oz * iz;
    return b;
}
RT_BOXRAY_FN BoxRay box_ray_f32(const double ox, const double oy, const double oz, const double dx, const double dy,
                                const double dz) {
    return box_ray_inv(ox, oy, oz, box_clamp(box_rcp((float)dx)), box_clamp(box_rcp((float)dy)),
                       box_clamp(box_rcp((float)dz)));
}

}  // namespace rtamd
