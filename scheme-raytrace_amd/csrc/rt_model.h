// rt_model.h — the object model behind the scene handles of include/rt.h: what the scene builder
// (rt_scene.cpp) records and the scene build (rt_build.cpp) reads.  Host code only (no device code, no
// HIP): tests/csrc/commit_check.cpp fills a SceneDesc directly.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "rt_device.h"

namespace rtamd {

enum ObjType { O_SPHERE, O_MSPHERE, O_RECT, O_FLIP, O_BOX, O_TRANSLATE, O_ROTATE_Y, O_LIST, O_BVH, O_BEZIER, O_MEDIUM, O_KLEIN, O_TRI };

struct Obj {
    ObjType type;
    int mat = -1, child = -1, axis = 0;
    std::vector<int> kids;
    double c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
    double r = 0, t0 = 0, t1 = 0;
    double a0 = 0, a1 = 0, b0 = 0, b1 = 0, k = 0;
    double sin_t = 0, cos_t = 1;
    double cp[12] = {0};       // O_BEZIER control points a, b, c, d; O_TRI: cp[0..8] = v0, v1, v2
    double width = 0;
    double uv[6] = {0};        // O_TRI: u0, u1, u2, v0, v1, v2 of its vertices (has_uv)
    bool has_uv = false;
    double nrm[9] = {0};       // O_TRI: the unit shading normals n0, n1, n2 of its vertices (has_nrm)
    bool has_nrm = false;
};

// A triangle's unit geometric normal (include/rt.h, "triangles"): n = cross(v1 - v0, v2 - v0) scaled by
// 1 / sqrt((nx nx + ny ny) + nz nz), in that order.  False: the cross product's length is zero or not finite.
inline bool tri_normal(const double* v0, const double* v1, const double* v2, double* n) {
    const double e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const double c[3] = {e1[1] * e2[2] - e2[1] * e1[2], e1[2] * e2[0] - e2[2] * e1[0], e1[0] * e2[1] - e2[0] * e1[1]};
    const double len = std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    if (!(len > 0.0) || !std::isfinite(len)) return false;
    const double k = 1.0 / len;
    for (int i = 0; i < 3; ++i) n[i] = c[i] * k;
    return true;
}

struct SceneDesc {
    std::vector<DevTexture> texs;
    std::vector<uint32_t> teximg;     // the image textures' texels (rt_add_texture_image), as DevScene::teximg
    std::vector<DevMaterial> mats;
    std::vector<Obj> objs;
    double cam[RT_CAMERA_DOUBLES] = {0};
    bool have_cam = false;
    int sky = RT_SKY_GRADIENT;
    int light = -1;                   // rt_set_light_sampling target (-1: off)
    std::vector<int> lights;          // rt_set_light_list's object ids (empty: none; set: light is -1)
    std::vector<double> ranvec;
    std::vector<int32_t> perm;
    bool have_perlin = false;
};

}  // namespace rtamd
