// bvh_media_check.cpp — media forests: build_scene (rt_build.cpp) on scenes with constant media
// filled directly into a SceneDesc, checked against what the list itself says: the segments, which leaves
// each segment's tree and groups reach, the boxes, the time-0 twins, the list order with the media in it.
// Host code with its own main, compiled with g++ under ASan / UBSan beside rt_build.cpp
// (tests/test_bvh_media_host.py).  Prints one JSON object: per scene its failed checks (none expected) and
// the counts the test pins.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../scheme-raytrace_amd/csrc/rt_build.h"

using namespace rtamd;

namespace {
std::vector<std::string> g_fail;                     // the current scene's failed checks
#define CHECK(cond) do { if (!(cond)) g_fail.push_back(std::string(#cond) + " @" + std::to_string(__LINE__)); } while (0)

// ---------------------------------------------------------------- scene construction
struct Builder {
    SceneDesc s;
    Builder() {
        s.have_cam = true;
        s.cam[9] = 0; s.cam[10] = 1; s.cam[11] = 8;  // origin
        s.cam[22] = 0.0; s.cam[23] = 1.0;            // shutter
        DevTexture t{}; t.type = TEX_CONSTANT; t.r = 0.5; t.g = 0.25; t.bl = 0.125;
        s.texs.push_back(t);
        for (int m = 0; m < 3; ++m) { DevMaterial M{}; M.type = m; M.tex = 0; M.fuzz = 0.1; M.ref_idx = 1.5; s.mats.push_back(M); }
    }
    int add(Obj o) { s.objs.push_back(std::move(o)); return (int)s.objs.size() - 1; }
    int sphere(double x, double y, double z, double r, int mat = 0) {
        Obj o; o.type = O_SPHERE; o.mat = mat; o.c0[0] = x; o.c0[1] = y; o.c0[2] = z; o.r = r; return add(o);
    }
    int msphere(double x, double y, double z, double r, double t0, double t1, int mat = 1) {
        Obj o; o.type = O_MSPHERE; o.mat = mat; o.c0[0] = x; o.c0[1] = y; o.c0[2] = z;
        o.c1[0] = x + 0.3; o.c1[1] = y + 0.5; o.c1[2] = z - 0.2; o.r = r; o.t0 = t0; o.t1 = t1; return add(o);
    }
    int rect(int axis, double a0, double a1, double b0, double b1, double k, int mat = 0) {
        Obj o; o.type = O_RECT; o.axis = axis; o.mat = mat; o.a0 = a0; o.a1 = a1; o.b0 = b0; o.b1 = b1; o.k = k; return add(o);
    }
    int unary(ObjType t, int child) { Obj o; o.type = t; o.child = child; o.mat = s.objs[child].mat; return add(o); }
    int flip(int child) { return unary(O_FLIP, child); }
    int translate(int child, double x, double y, double z) {
        const int id = unary(O_TRANSLATE, child);
        s.objs[id].c0[0] = x; s.objs[id].c0[1] = y; s.objs[id].c0[2] = z; return id;
    }
    int rotate_y(int child, double deg) {
        const int id = unary(O_ROTATE_Y, child);
        s.objs[id].sin_t = std::sin(deg * kPi / 180); s.objs[id].cos_t = std::cos(deg * kPi / 180); return id;
    }
    int list(std::vector<int> kids, ObjType t = O_LIST) { Obj o; o.type = t; o.kids = std::move(kids); return add(o); }
    int box(double x0, double y0, double z0, double x1, double y1, double z1, int mat = 0) {
        return list({rect(0, x0, x1, y0, y1, z1, mat), flip(rect(0, x0, x1, y0, y1, z0, mat)), rect(1, x0, x1, z0, z1, y1, mat),
                     flip(rect(1, x0, x1, z0, z1, y0, mat)), rect(2, y0, y1, z0, z1, x1, mat), flip(rect(2, y0, y1, z0, z1, x0, mat))}, O_BOX);
    }
    int medium(int child, double density) {
        DevMaterial M{}; M.type = MAT_LAMBERTIAN; M.tex = 0; s.mats.push_back(M);
        Obj o; o.type = O_MEDIUM; o.child = child; o.r = density; o.mat = (int)s.mats.size() - 1; return add(o);
    }
    int klein(double x, double y, double z) { Obj o; o.type = O_KLEIN; o.mat = 0; o.c0[0] = x; o.c0[1] = y; o.c0[2] = z; return add(o); }
};
double frand(uint32_t& st) { st = st * 1664525u + 1013904223u; return (st >> 8) * (1.0 / 16777216.0); }

// "The Next Week"'s closing scene at 6 x 6 boxes and a cluster of 60, its two media where the book lists them:
// segments of 216 box faces + 6 leaves, none, and 60 instanced spheres + 2 leaves
int next_week_small_media(Builder& b) {
    uint32_t st = 7u;
    std::vector<int> boxes, small;
    const double w = 2000.0 / 6;
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j)
            boxes.push_back(b.box(-1000 + i * w, 0, -1000 + j * w, -1000 + (i + 1) * w, 100 * (frand(st) + 0.01), -1000 + (j + 1) * w));
    for (int k = 0; k < 60; ++k)
        small.push_back(b.translate(b.rotate_y(b.sphere(165 * frand(st), 165 * frand(st), 165 * frand(st), 10), 15), -100, 270, 395));
    return b.list({b.list(boxes, O_BVH), b.flip(b.rect(1, 123, 423, 147, 412, 554)), b.msphere(400, 400, 200, 50, 0, 1),
                   b.sphere(260, 150, 45, 50, 2), b.sphere(0, 150, 145, 50, 1), b.sphere(360, 150, 145, 70, 2),
                   b.medium(b.sphere(360, 150, 145, 70, 2), 0.2), b.medium(b.sphere(0, 0, 0, 5000, 2), 0.0001),
                   b.sphere(400, 200, 400, 100), b.sphere(220, 280, 300, 80), b.list(small, O_BVH)});
}
// Three media, four segments: a tree (3 x 3 boxes and 6 spheres under one chain), 5 rects in groups, a tree
// that is not the first with a world-level moving sphere and a rect of segment 0 listed again, nothing
int media_mix(Builder& b, const bool with_klein = false) {
    uint32_t st = 11u;
    std::vector<int> seg0, seg2;
    int again = -1;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int bx = b.box(-1.5 + i, 0, -1.5 + j, -0.5 + i, 0.3 + frand(st), -0.5 + j);
            if (i == 1 && j == 1) again = b.s.objs[bx].kids[2];          // its top face
            seg0.push_back(b.translate(bx, 1, 0, 0.5));
        }
    for (int k = 0; k < 6; ++k) seg0.push_back(b.translate(b.sphere(-1 + 0.4 * k, 1.8, 0.3 * k - 0.5, 0.25, k % 3), 1, 0, 0.5));
    for (int k = 0; k < 50; ++k)
        seg2.push_back(b.translate(b.rotate_y(b.sphere(2 * frand(st), 2 * frand(st), 2 * frand(st), 0.1, k % 3), 25), -3, 0.2, -2));
    std::vector<int> world = {
        b.list(seg0, O_BVH),
        b.medium(b.translate(b.rotate_y(b.box(0, 0, 0, 1, 1.2, 1), -18), -2.5, 0, 1), 0.8),
        b.rect(1, -6, 6, -6, 6, -0.01), b.rect(0, -4, 4, 0, 3, -4), b.rect(2, 0, 3, -4, 4, -5), b.rect(2, 0, 3, -4, 4, 5),
        b.flip(b.rect(1, -1, 1, -1, 1, 5, 0)),
        b.medium(b.sphere(2.5, 1, -1, 0.8), 1.5),
        b.list(seg2, O_BVH), b.msphere(0, 2.6, 0, 0.3, 0, 1), b.translate(again, 1, 0, 0.5),
        b.medium(b.sphere(0, 1, 0, 100), 0.002)};
    if (with_klein) world.push_back(b.klein(0, 30, 0));
    return b.list(world);
}
// nine segments of 48 instanced spheres each, a medium after each of the first eight
int nine_segments(Builder& b) {
    uint32_t st = 13u;
    std::vector<int> world;
    for (int sgm = 0; sgm < 9; ++sgm) {
        for (int k = 0; k < 48; ++k)
            world.push_back(b.translate(b.sphere(frand(st), frand(st), frand(st), 0.05), 2.0 * sgm - 8, 0, 0));
        if (sgm < 8) world.push_back(b.medium(b.sphere(2.0 * sgm - 7.5, 0.5, 0.5, 0.4), 1.0));
    }
    return b.list(world);
}

// ---------------------------------------------------------------- the list itself
void to_world(const std::vector<ChainOpRec>& ops, double* p) {      // outermost op first: apply the last first
    for (size_t k = ops.size(); k-- > 0;) {
        if (ops[k].op == OP_TRANSLATE) { p[0] += ops[k].x; p[1] += ops[k].y; p[2] += ops[k].z; }
        else { const double x = ops[k].y * p[0] + ops[k].x * p[2], z = -ops[k].x * p[0] + ops[k].y * p[2]; p[0] = x; p[2] = z; }
    }
}
// Points and a radius: a box that holds every point grown by the radius holds the primitive.
// time0: a moving sphere where it is at time 0, else over the shutter.
double hull_points(const SceneDesc& s, const LeafTmp& L, const std::vector<ChainOpRec>& ops, bool time0, std::vector<double>& pts) {
    const Obj& o = s.objs[L.obj];
    pts.clear();
    auto push = [&](double x, double y, double z) { double p[3] = {x, y, z}; to_world(ops, p); pts.insert(pts.end(), p, p + 3); };
    if (L.type == LEAF_SPHERE) { push(o.c0[0], o.c0[1], o.c0[2]); return std::fabs(o.r); }
    if (L.type == LEAF_MSPHERE) {
        const double tlo = std::min(std::min(s.cam[22], s.cam[23]), 0.0), thi = std::max(std::max(s.cam[22], s.cam[23]), 0.0);
        for (const double t : {time0 ? 0.0 : tlo, time0 ? 0.0 : thi}) {
            const double f = (t - o.t0) / (o.t1 - o.t0);
            push(o.c0[0] + (o.c1[0] - o.c0[0]) * f, o.c0[1] + (o.c1[1] - o.c0[1]) * f, o.c0[2] + (o.c1[2] - o.c0[2]) * f);
        }
        return std::fabs(o.r);
    }
    for (const double a : {o.a0, o.a1})
        for (const double bb : {o.b0, o.b1}) {
            if (L.type == LEAF_RECT_XY) push(a, bb, o.k);
            else if (L.type == LEAF_RECT_XZ) push(a, o.k, bb);
            else push(o.k, a, bb);
        }
    return 0.0;
}

struct Fnv {
    uint64_t x = 1469598103934665603ull;
    void bytes(const void* p, size_t n) { for (size_t k = 0; k < n; ++k) x = (x ^ ((const uint8_t*)p)[k]) * 1099511628211ull; }
};
template <class V> void arr(Fnv& f, const V& v) {
    const size_t n = v.size();
    f.bytes(&n, sizeof n);
    if (n) f.bytes(v.data(), n * sizeof(v[0]));
}
uint64_t digest(const HostScene& h) {
    Fnv f;
    arr(f, h.sph); arr(f, h.msph); arr(f, h.rect); arr(f, h.med); arr(f, h.groups); arr(f, h.bgroups); arr(f, h.bvh2);
    arr(f, h.bleaf); arr(f, h.g0bvh2); arr(f, h.g0bleaf); arr(f, h.order); arr(f, h.gleaf); arr(f, h.leaf_pos);
    arr(f, h.rot); arr(f, h.leaves); arr(f, h.leaf_cls);
    f.bytes(&h.tree, sizeof h.tree);
    return f.x;
}

// One tree from its root: the leaf ids it reaches (each once), every primitive inside the box its parent
// holds for it; bounded by the arrays
template <class VN, class VL>
void walk_tree(const SceneDesc& s, const HostScene& h, const VN& nodes, const VL& leaves, const int32_t root, const bool time0,
               std::vector<int>& ids) {
    struct Item { int32_t ref; float lo[3], hi[3]; bool boxed; };
    std::vector<Item> stack{{root, {0, 0, 0}, {0, 0, 0}, false}};
    size_t steps = 0;
    std::vector<double> pts;
    while (!stack.empty() && ++steps < 10000000) {
        const Item it = stack.back();
        stack.pop_back();
        if (it.ref >= 0) {
            CHECK((size_t)it.ref < nodes.size());
            if ((size_t)it.ref >= nodes.size()) return;
            const BvhNode2& M = nodes[(size_t)it.ref];
            for (int side = 0; side < 2; ++side) {
                Item c{side ? M.r : M.l, {0, 0, 0}, {0, 0, 0}, true};
                for (int k = 0; k < 3; ++k) { c.lo[k] = M.b[2 * k + side]; c.hi[k] = M.b[6 + 2 * k + side]; }
                stack.push_back(c);
            }
            continue;
        }
        CHECK((size_t)~it.ref < leaves.size());
        if ((size_t)~it.ref >= leaves.size()) return;
        const BvhLeaf& L = leaves[(size_t)~it.ref];
        CHECK(L.sn == 0 && L.mn == 0 && L.bn == 0 && L.gn > 0 && L.gb >= 0 && (size_t)(L.gb + L.gn) <= h.gleaf.size());
        for (int g = L.gb; g < L.gb + L.gn && (size_t)g < h.gleaf.size(); ++g) {
            const int id = h.gleaf[(size_t)g];
            ids.push_back(id);
            const int pos = h.leaf_pos[(size_t)id];
            const LeafTmp& lt = h.f.leaves[(size_t)pos];
            const std::vector<ChainOpRec> none;
            const double r = hull_points(s, lt, lt.chain >= 0 ? h.f.chains[(size_t)lt.chain] : none, time0, pts);
            bool in = true;
            for (size_t i = 0; it.boxed && i < pts.size(); i += 3)
                for (int k = 0; k < 3; ++k)
                    in = in && (double)it.lo[k] <= pts[i + k] - r && pts[i + k] + r <= (double)it.hi[k];
            CHECK(in);
        }
    }
}

struct Result { int segments = 0, trees = 0, twins = 0, tree_leaves = 0, group_leaves = 0, n_order = 0, gleaf = 0, rot = 0; uint64_t dig = 0; };

// A forest's commit against the list
Result check_forest(const SceneDesc& s, const HostScene& h) {
    Result r;
    const Flattener& f = h.f;
    const DevScene& d = h.d;
    const size_t n = f.leaves.size();
    r.n_order = d.n_order; r.gleaf = (int)h.gleaf.size(); r.rot = (int)h.rot.size(); r.dig = digest(h);
    r.segments = h.tree.segments; r.trees = h.tree.segment_trees;
    CHECK(h.forest && h.generic);
    // order / leaf_pos are the list, the media at their positions
    CHECK(h.order.size() == n && d.n_order == (int)n && h.leaf_pos.size() == h.leaves.size());
    if (h.order.size() != n || h.leaf_pos.size() != h.leaves.size()) return r;
    std::vector<int> seg(n, 0);
    int nseg = 1;
    for (size_t i = 0; i < n; ++i) {
        seg[i] = nseg - 1;
        const int id = h.order[i];
        CHECK(id >= 0 && (size_t)id < h.leaves.size());
        if (id < 0 || (size_t)id >= h.leaves.size()) return r;
        const LeafInfo& li = h.leaves[(size_t)id];
        const LeafTmp& L = f.leaves[i];
        const Obj& o = s.objs[L.obj];
        CHECK(li.type == L.type && li.chain == L.chain && li.flip == L.flip && li.mat == o.mat);
        CHECK(h.leaf_pos[(size_t)id] == (int32_t)i);
        CHECK(id == d.leaf_base[L.type] + li.local);
        if (L.type == LEAF_SPHERE) CHECK(h.sph[(size_t)li.local].cx == o.c0[0] && h.sph[(size_t)li.local].rr == o.r * o.r);
        else if (L.type == LEAF_MSPHERE) CHECK(h.msph[(size_t)li.local].c0x == o.c0[0] && h.msph[(size_t)li.local].den == o.t1 - o.t0);
        else if (L.type == LEAF_MEDIUM) CHECK(h.med[(size_t)li.local].neg_inv_density == -(1 / o.r));
        else CHECK(h.rect[(size_t)li.local].k == o.k && h.rect[(size_t)li.local].a0 == o.a0 && h.rect[(size_t)li.local].b1 == o.b1);
        if (L.type == LEAF_MEDIUM) ++nseg;
    }
    CHECK(h.tree.segments == nseg);
    // groups: segment by segment [tree] [groups] [medium]
    std::vector<int> reached(h.leaves.size(), 0);
    int sg = 0, trees = 0, twins = 0, tree_leaves = 0, group_leaves = 0;
    bool seen_tree = false, seen_group = false;
    for (const Group& G : h.groups) {
        if (G.type == GROUP_BVH) {
            CHECK(!seen_tree && !seen_group);
            seen_tree = true;
            ++trees;
            std::vector<int> ids, ids0;
            walk_tree(s, h, h.bvh2, h.bleaf, G.begin, false, ids);
            bool moving = false;
            for (const int id : ids) {
                CHECK(seg[(size_t)h.leaf_pos[(size_t)id]] == sg);            // no tree reaches another segment's leaf
                ++reached[(size_t)id];
                moving = moving || h.leaves[(size_t)id].type == LEAF_MSPHERE;
            }
            tree_leaves += (int)ids.size();
            CHECK((G.end != kNoTwin) == moving);                              // a twin exactly where a sphere moves
            if (G.end != kNoTwin) {
                ++twins;
                walk_tree(s, h, h.g0bvh2, h.g0bleaf, G.end, true, ids0);
                std::sort(ids.begin(), ids.end());
                std::sort(ids0.begin(), ids0.end());
                CHECK(ids == ids0);
            }
        } else if (G.type == LEAF_MEDIUM) {
            CHECK(G.end == G.begin + 1);
            const int id = d.leaf_base[LEAF_MEDIUM] + G.begin;
            CHECK(seg[(size_t)h.leaf_pos[(size_t)id]] == sg);
            ++reached[(size_t)id];
            ++sg;
            seen_tree = seen_group = false;
        } else {
            seen_group = true;
            for (int k = G.begin; k < G.end; ++k) {
                const int id = d.leaf_base[G.type] + k;
                CHECK(h.leaves[(size_t)id].chain == G.chain && h.leaves[(size_t)id].type == G.type);
                CHECK(seg[(size_t)h.leaf_pos[(size_t)id]] == sg);
                ++reached[(size_t)id];
                ++group_leaves;
            }
        }
    }
    CHECK(sg == nseg - 1);
    for (size_t i = 0; i < n; ++i) CHECK(reached[(size_t)h.order[i]] == 1);  // by exactly one of its tree or its groups
    std::set<int> listed(h.order.begin(), h.order.end());
    for (size_t id = 0; id < h.leaves.size(); ++id)
        if (!listed.count((int)id)) CHECK(reached[id] == 0);                  // (boundary leaves: in bgroups only)
    r.twins = twins; r.tree_leaves = tree_leaves; r.group_leaves = group_leaves;
    // rt_tree_info
    const rt_tree_info& t = h.tree;
    CHECK(t.segment_trees == trees && trees <= 8);
    CHECK(t.sphere_leaves + t.generic_leaves == tree_leaves && t.curve_leaves == 0);
    CHECK(t.group_leaves == (int)h.leaves.size() - tree_leaves);
    CHECK(t.nodes == (int)h.bvh2.size() && t.nodes0 == (int)h.g0bvh2.size() && (t.nodes0 > 0) == (twins > 0));
    CHECK(t.depth > 0 && t.depth <= kLaneStack && t.depth0 <= kLaneStack && d.lane_stack == std::max(t.depth, t.depth0));
    CHECK(t.rot_entries == (int)h.rot.size() && d.n_rot == t.rot_entries && d.n_gleaf == (int)h.gleaf.size());
    CHECK(d.n_med == nseg - 1 && d.n_groups == (int)h.groups.size());
    return r;
}

// a commit without forests: what every scene with media got before them
void check_plain(const HostScene& h) {
    int tree_groups = 0;
    for (const Group& G : h.groups) tree_groups += G.type == GROUP_BVH;
    CHECK(!h.forest && !h.generic && h.d.n_order == 0 && h.order.empty() && h.gleaf.empty() && h.leaf_pos.empty() && h.rot.empty());
    CHECK(tree_groups <= 1 && h.tree.segments == 0 && h.tree.segment_trees == 0 && h.tree.generic_leaves == 0);
    CHECK(h.g0bvh2.empty() && h.g0bleaf.empty());
}

void report(const char* name, const Result& r, const bool same, bool& first) {
    std::printf("%s\"%s\": {\"fail\": [", first ? "" : ", ", name);
    for (size_t i = 0; i < g_fail.size() && i < 8; ++i) std::printf("%s\"%s\"", i ? ", " : "", g_fail[i].c_str());
    std::printf("], \"segments\": %d, \"trees\": %d, \"twins\": %d, \"tree_leaves\": %d, \"group_leaves\": %d, \"n_order\": %d, "
                "\"gleaf\": %d, \"rot\": %d, \"threads_same\": %s}", r.segments, r.trees, r.twins, r.tree_leaves,
                r.group_leaves, r.n_order, r.gleaf, r.rot, same ? "true" : "false");
    g_fail.clear();
    first = false;
}
}  // namespace

int main() {
    bool first = true;
    std::printf("{");
    auto forest_case = [&](const char* name, auto make) {
        Builder b;
        const int world = make(b);
        Result r1{}, r8{};
        for (const int threads : {1, 8}) {
            HostScene h;
            std::string err;
            BuildOptions opt;
            opt.threads = threads;
            const int rc = build_scene(b.s, world, opt, h, err);
            CHECK(rc == 0);
            if (rc) { std::fprintf(stderr, "%s: %s\n", name, err.c_str()); continue; }
            (threads == 1 ? r1 : r8) = check_forest(b.s, h);
        }
        report(name, r1, r1.dig == r8.dig && r1.dig != 0, first);
        // the threshold above every segment's count: the commit without forests
        HostScene h;
        std::string err;
        BuildOptions opt;
        opt.generic_min = 1000000;
        CHECK(build_scene(b.s, world, opt, h, err) == 0);
        check_plain(h);
        Result rp{};
        rp.n_order = h.d.n_order; rp.gleaf = (int)h.gleaf.size();
        report((std::string(name) + "_groups").c_str(), rp, true, first);
    };
    forest_case("next_week_small_media", [](Builder& b) { return next_week_small_media(b); });
    forest_case("media_mix", [](Builder& b) { return media_mix(b); });
    forest_case("nine_segments", [](Builder& b) { return nine_segments(b); });
    {   // a Klein set beside the media: no forest
        Builder b;
        const int world = media_mix(b, true);
        HostScene h;
        std::string err;
        CHECK(build_scene(b.s, world, BuildOptions{}, h, err) == 0);
        check_plain(h);
        Result rp{};
        rp.n_order = h.d.n_order; rp.gleaf = (int)h.gleaf.size();
        report("media_mix_klein", rp, true, first);
    }
    std::printf("}\n");
    return 0;
}
