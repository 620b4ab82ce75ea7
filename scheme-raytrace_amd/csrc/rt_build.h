// rt_build.h — the host half of a scene commit (rt_build.cpp): the object graph of a SceneDesc flattened
// into grouped leaves, the BVH builds (rt_bvh.h) and every record array of the device scene, in host
// memory.  Host code only (no device code, no HIP): tests/csrc/commit_check.cpp compiles rt_build.cpp with
// g++ and checks its decisions; rt_commit.cpp uploads the result.
#pragma once
#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

#include "rt_bvh.h"
#include "rt_device.h"
#include "rt_model.h"

namespace rtamd {

// -DRT_COMMIT_PROFILE: a commit's phases print the time since its start (commit_scene sets commit_t0())
#ifdef RT_COMMIT_PROFILE
inline std::chrono::steady_clock::time_point& commit_t0() {
    thread_local std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    return t0;
}
#define COMMIT_MARK(tag) std::fprintf(stderr, "commit %-12s %9.1f ms\n", tag, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - rtamd::commit_t0()).count())
#else
#define COMMIT_MARK(tag) ((void)0)
#endif

// What a build takes from the environment (from_env is the only reader) and a test sets directly.
struct BuildOptions {
    size_t bvh_min = 16;              // RTAMD_BVH_MIN: fewest tree leaves a world tree is built for
    // RTAMD_BVH_GENERIC_MIN: fewest generic leaves (rects, instanced spheres) a scene needs for them to join
    // the world tree: below the crossover a handful of uniform group loops beats a per-lane walk (DESIGN.md
    // §4.8: the default is the measured crossover, 48 leaves, and never below 32; any count for measurements
    // and tests)
    size_t generic_min = 48;
    int sweep_max = 1 << 16;          // RTAMD_BVH_SWEEP: BvhBuild::sweep_max (rt_bvh.h)
    bool no_bvh0 = false;             // RTAMD_NO_BVH0: no time-0 tree
    bool no_solo = false;             // RTAMD_NO_SOLO: DevScene::bvh_solo stays 0
    int threads = 1;                  // host threads (from_env: build_threads())
    static BuildOptions from_env();
};
static_assert(BuildOptions{}.generic_min >= 32, "every scene with fewer generic leaves keeps its groups");

struct LeafTmp {
    int type;          // LeafType
    int chain;         // -1 = world
    int flip;
    int obj;           // source object
    int aux = -1;      // LEAF_MEDIUM: index into Flattener::bounds
};

// The object graph under the world object as leaves in hit-obj-list (depth-first) order
struct Flattener {
    const SceneDesc* s;
    std::string* err;                              // walk's failure text
    std::vector<std::vector<ChainOpRec>> chains;   // unique chains
    std::vector<LeafTmp> leaves;                   // DFS order
    std::vector<std::vector<LeafTmp>> bounds;      // per constant medium: its boundary's leaves
    std::vector<ChainOpRec> cur;
    int depth_guard = 0;
    bool in_boundary = false;
    int chain_id();
    int walk(int id, int flip);
};

// Shade-side records per type as the record arrays grow, and each list position's (type, index in the
// type's array), -1 for media: what the leaf ids are derived from
struct LeafLists {
    HostVec<LeafInfo> sph, msph, bez;              // (filled by threads after a resize: rt_bvh.h, NoInit)
    std::vector<LeafInfo> rect, klein, med, tri;
    std::vector<int32_t> ord_type, ord_local;
};

struct HostScene {
    // the arrays of DevScene, by its members' names
    HostVec<SphereRec> sph;
    HostVec<MSphereRec> msph;
    std::vector<RectRec> rect;
    HostVec<BezierRec> bez;
    std::vector<KleinRec> klein;
    std::vector<MediumRec> med;
    std::vector<TriRec> tri;                         // triangles, in tree order, their texture coordinates and
    std::vector<TriUv> triuv;                        // their vertices' shading normals, one of each per triangle
    std::vector<TriNrm> trinrm;
    std::vector<Group> groups, bgroups;
    HostVec<BvhNode2> bvh2, fbvh2, g0bvh2;           // the world tree; the time-0 tree, sphere form / generic form
    HostVec<BvhLeaf> bleaf, fbleaf, g0bleaf;
    HostVec<BvhNode4> bvh4;                          // curve trees (k_extend_curves)
    std::vector<SphereRec> fsph;
    std::vector<int32_t> fid, order, gleaf, leaf_pos;
    std::vector<RotEntry> rot;
    std::vector<DevLightRec> lights;                 // the light list's records (empty: none, or one rect / sphere in d.light)
    std::vector<Chain> chains;
    HostVec<LeafInfo> leaves;
    std::vector<uint8_t> leaf_cls;
    // every count, root, flag, the camera, the light and leaf_base; every pointer null, and what depends on
    // the device (lds4, ring_waves, ovf_lanes) zero
    DevScene d{};
    bool generic = false;             // the world tree holds generic leaves (gleaf, leaf_pos, rot)
    bool forest = false;              // a media forest: one generic tree per segment; implies generic
    rt_tree_info tree{};
    double sah_ms = 0.0;              // the SAH builds' wall time, on `threads` host threads
    int threads = 1;
    // scratch, kept so that the caller can free it off its own thread
    Flattener f{};
    std::vector<PrimRef> refs;        // the world tree's leaves in tree order (PrimRef::leaf = list position)
    std::vector<BvhNode> bvh_nodes;
    LeafLists ll;
};

// A light list (include/rt.h, "light lists") flattened: the ids of its m lights (rects, spheres, triangles;
// flips looked through, lists and meshes opened), in order.  Returns 0, or 1 with the refusal's text in err:
// a null objs with n > 0, n < 0, a bad id, a kind that cannot be a light, m = 0, m > RT_MAX_LIGHTS.
int flatten_lights(const SceneDesc& sd, const int* objs, int n, std::vector<int>& out, std::string& err);

// The host scene of the object graph under object `world`.  Returns 0, or 1 with the failure's text in err.
int build_scene(const SceneDesc& sd, int world, const BuildOptions& opt, HostScene& h, std::string& err);

}  // namespace rtamd
