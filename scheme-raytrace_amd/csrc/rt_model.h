// rt_model.h — the object model behind the scene handles of include/rt.h: what the scene builder
// (rt_scene.cpp) records and the scene build (rt_build.cpp) reads.  Host code only (no device code, no
// HIP): tests/csrc/commit_check.cpp fills a SceneDesc directly.
#pragma once
#include <cstdint>
#include <vector>

#include "rt_device.h"

namespace rtamd {

enum ObjType { O_SPHERE, O_MSPHERE, O_RECT, O_FLIP, O_BOX, O_TRANSLATE, O_ROTATE_Y, O_LIST, O_BVH, O_BEZIER, O_MEDIUM, O_KLEIN };

struct Obj {
    ObjType type;
    int mat = -1, child = -1, axis = 0;
    std::vector<int> kids;
    double c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
    double r = 0, t0 = 0, t1 = 0;
    double a0 = 0, a1 = 0, b0 = 0, b1 = 0, k = 0;
    double sin_t = 0, cos_t = 1;
    double cp[12] = {0};       // O_BEZIER control points a, b, c, d
    double width = 0;
};

struct SceneDesc {
    std::vector<DevTexture> texs;
    std::vector<uint32_t> teximg;     // the image textures' texels (rt_add_texture_image), as DevScene::teximg
    std::vector<DevMaterial> mats;
    std::vector<Obj> objs;
    double cam[RT_CAMERA_DOUBLES] = {0};
    bool have_cam = false;
    int sky = RT_SKY_GRADIENT;
    int light = -1;                   // rt_set_light_sampling target (-1: off)
    std::vector<double> ranvec;
    std::vector<int32_t> perm;
    bool have_perlin = false;
};

}  // namespace rtamd
