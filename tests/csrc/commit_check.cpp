// commit_check.cpp — build_scene (rt_build.cpp) on small scenes filled directly into a SceneDesc, its
// decisions checked against brute force written here: a flattening of its own, primitive bounds computed
// from the objects, coverage counts.  Host code with its own main, compiled with g++ under ASan / UBSan
// beside rt_build.cpp (tests/test_commit_host.py).  Prints one JSON object: per scene its failed checks
// (none expected) and a few counts the test pins.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <pthread.h>
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
    int bezier(double x, double y, double z, double w, int mat = 0) {
        Obj o; o.type = O_BEZIER; o.mat = mat; o.width = w;
        const double cp[12] = {x, y, z, x + 0.2, y + 0.4, z, x - 0.1, y + 0.8, z + 0.1, x + 0.1, y + 1.2, z};
        std::memcpy(o.cp, cp, sizeof cp); return add(o);
    }
    int medium(int child, double density) {
        DevMaterial M{}; M.type = MAT_LAMBERTIAN; M.tex = 0; s.mats.push_back(M);
        Obj o; o.type = O_MEDIUM; o.child = child; o.r = density; o.mat = (int)s.mats.size() - 1; return add(o);
    }
    int klein(double x, double y, double z) { Obj o; o.type = O_KLEIN; o.mat = 0; o.c0[0] = x; o.c0[1] = y; o.c0[2] = z; return add(o); }
};

// ---------------------------------------------------------------- brute force: the flattened list
struct Flat { int type, obj, flip; std::vector<ChainOpRec> ops; int bound = -1; };   // bound: a medium's boundary list
struct FlatScene { std::vector<Flat> world; std::vector<std::vector<Flat>> bounds; };
void flatten(const SceneDesc& s, int id, int flip, std::vector<ChainOpRec>& ops, FlatScene& fs, std::vector<Flat>& out) {
    const Obj& o = s.objs[id];
    switch (o.type) {
    case O_SPHERE: out.push_back({LEAF_SPHERE, id, flip, ops}); break;
    case O_MSPHERE: out.push_back({LEAF_MSPHERE, id, flip, ops}); break;
    case O_RECT: out.push_back({LEAF_RECT_XY + o.axis, id, flip, ops}); break;
    case O_BEZIER: out.push_back({LEAF_BEZIER, id, flip, ops}); break;
    case O_KLEIN: out.push_back({LEAF_KLEIN, id, flip, ops}); break;
    case O_MEDIUM: {
        std::vector<Flat> b;
        flatten(s, o.child, 0, ops, fs, b);
        fs.bounds.push_back(b);
        Flat m{LEAF_MEDIUM, id, flip, ops};
        m.bound = (int)fs.bounds.size() - 1;
        out.push_back(m);
        break;
    }
    case O_FLIP: flatten(s, o.child, flip ^ 1, ops, fs, out); break;
    case O_BOX: case O_LIST: case O_BVH: for (int k : o.kids) flatten(s, k, flip, ops, fs, out); break;
    case O_TRANSLATE: case O_ROTATE_Y: {
        ChainOpRec op{};
        if (o.type == O_TRANSLATE) { op.op = OP_TRANSLATE; op.x = o.c0[0]; op.y = o.c0[1]; op.z = o.c0[2]; }
        else { op.op = OP_ROTATE_Y; op.x = o.sin_t; op.y = o.cos_t; }
        ops.push_back(op);
        flatten(s, o.child, flip, ops, fs, out);
        ops.pop_back();
        break;
    }
    }
}

// a local point out of a chain (outermost op first in ops: apply the innermost, the last, first)
void to_world(const std::vector<ChainOpRec>& ops, double* p) {
    for (size_t k = ops.size(); k-- > 0;) {
        if (ops[k].op == OP_TRANSLATE) { p[0] += ops[k].x; p[1] += ops[k].y; p[2] += ops[k].z; }
        else { const double x = ops[k].y * p[0] + ops[k].x * p[2], z = -ops[k].x * p[0] + ops[k].y * p[2]; p[0] = x; p[2] = z; }
    }
}
double center0(const Obj& o, int k) { const double dc = o.c1[k] - o.c0[k]; return o.c0[k] + dc * ((0.0 - o.t0) / (o.t1 - o.t0)); }

// Points whose hull holds the primitive, shrunk by nothing: a box that holds them all (less `r`, returned) holds it.
// time0: a moving sphere where it is at time 0, else over [tlo, thi].
double hull_points(const SceneDesc& s, const Flat& L, bool time0, std::vector<double>& pts) {
    const Obj& o = s.objs[L.obj];
    pts.clear();
    auto push = [&](double x, double y, double z) { double p[3] = {x, y, z}; to_world(L.ops, p); pts.insert(pts.end(), p, p + 3); };
    if (L.type == LEAF_SPHERE) { push(o.c0[0], o.c0[1], o.c0[2]); return std::fabs(o.r); }
    if (L.type == LEAF_MSPHERE) {
        if (time0) { push(center0(o, 0), center0(o, 1), center0(o, 2)); return std::fabs(o.r); }
        const double tlo = std::min(std::min(s.cam[22], s.cam[23]), 0.0), thi = std::max(std::max(s.cam[22], s.cam[23]), 0.0);
        for (const double t : {tlo, thi}) {
            const double f = (t - o.t0) / (o.t1 - o.t0);
            push(o.c0[0] + (o.c1[0] - o.c0[0]) * f, o.c0[1] + (o.c1[1] - o.c0[1]) * f, o.c0[2] + (o.c1[2] - o.c0[2]) * f);
        }
        return std::fabs(o.r);
    }
    if (L.type == LEAF_BEZIER) { for (int i = 0; i < 4; ++i) push(o.cp[3 * i], o.cp[3 * i + 1], o.cp[3 * i + 2]); return std::fabs(o.width / 2); }
    for (const double a : {o.a0, o.a1})
        for (const double b : {o.b0, o.b1}) {
            if (L.type == LEAF_RECT_XY) push(a, b, o.k);
            else if (L.type == LEAF_RECT_XZ) push(a, o.k, b);
            else push(o.k, a, b);
        }
    return 0.0;
}
bool inside(const std::vector<double>& pts, double r, const float* lo, const float* hi) {
    for (size_t i = 0; i < pts.size(); i += 3)
        for (int k = 0; k < 3; ++k)
            if (!((double)lo[k] <= pts[i + k] - r && pts[i + k] + r <= (double)hi[k])) return false;
    return true;
}

// ---------------------------------------------------------------- digests
struct Fnv {
    uint64_t x = 1469598103934665603ull;
    void bytes(const void* p, size_t n) { for (size_t k = 0; k < n; ++k) x = (x ^ ((const uint8_t*)p)[k]) * 1099511628211ull; }
    template <class T> void val(const T& v) { bytes(&v, sizeof v); }
    template <class... T> void vals(const T&... v) { (val(v), ...); }
};
// records without padding between or after their members (each static_assert: the members' sizes add up)
static_assert(sizeof(SphereRec) == 32 && sizeof(MSphereRec) == 96 && sizeof(RectRec) == 64 && sizeof(KleinRec) == 32, "");
static_assert(sizeof(BezierRec) == 15 * 8 + 8 && sizeof(MediumRec) == 32 && sizeof(Group) == 16 && sizeof(BvhLeaf) == 32, "");
static_assert(sizeof(BvhNode2) == 64 && sizeof(BvhNode4) == 128 && sizeof(LeafInfo) == 8 * 4 + 12 * 8, "");
static_assert(sizeof(Chain) == 8 + kMaxChain * 32 && sizeof(ChainOpRec) == 32 && sizeof(RotEntry) == 8 + kMaxChain * 16, "");
template <class V> void arr(Fnv& f, const V& v) { f.val(v.size()); if (!v.empty()) f.bytes(v.data(), v.size() * sizeof(v[0])); }
uint64_t digest(const HostScene& h) {
    Fnv f;
    arr(f, h.sph); arr(f, h.msph); arr(f, h.rect); arr(f, h.bez); arr(f, h.klein); arr(f, h.med); arr(f, h.groups);
    arr(f, h.bgroups); arr(f, h.bvh2); arr(f, h.fbvh2); arr(f, h.g0bvh2); arr(f, h.bleaf); arr(f, h.fbleaf); arr(f, h.g0bleaf);
    arr(f, h.bvh4); arr(f, h.fsph); arr(f, h.fid); arr(f, h.order); arr(f, h.gleaf); arr(f, h.leaf_pos); arr(f, h.rot);
    arr(f, h.chains); arr(f, h.leaves); arr(f, h.leaf_cls);
    const DevScene& d = h.d;                          // (padded: member by member; the pointers are checked null)
    f.vals(d.n_sph, d.n_msph, d.n_rect, d.n_bez, d.n_med, d.n_klein, d.n_bgroups, d.n_groups, d.n_bvh2, d.bvh2_root,
           d.bvh_has_bez, d.bez_groups, d.bvh_pad, d.lane_stack, d.n_bvh4, d.ring_waves, d.bvh4_root, d.stack4, d.lds4,
           d.ovf_lanes, d.fbvh2_root, d.n_fbvh2, d.n_fbleaf, d.n_fsph, d.tree0_any_time, d.n_bleaf, d.msph_shared,
           d.msph_t0, d.msph_den, d.bvh_solo, d.n_chains, d.n_leaves, d.n_mats, d.n_texs, d.has_perlin, d.has_noise_tex,
           d.sky, d.mat_mask, d.n_order, d.has_image_tex, d.n_gleaf, d.g0bvh2_root, d.n_g0bvh2, d.n_rot);
    f.bytes(d.leaf_base, sizeof d.leaf_base);
    f.bytes(&d.cam, sizeof d.cam);                    // 24 doubles
    f.vals(d.light.type, d.light.axis, d.light.a0, d.light.a1, d.light.b0, d.light.b1, d.light.k, d.light.cx, d.light.cy,
           d.light.cz, d.light.r);
    f.vals(h.tree.sphere_leaves, h.tree.curve_leaves, h.tree.generic_leaves, h.tree.group_leaves, h.tree.nodes, h.tree.depth,
           h.tree.nodes0, h.tree.depth0, h.tree.rot_entries, h.tree.generic_min);
    return f.x;
}
bool pointers_null(const DevScene& d) {
    return !d.sph && !d.msph && !d.rect && !d.bez && !d.med && !d.klein && !d.bgroups && !d.groups && !d.bvh2 && !d.bleaf &&
           !d.bvh4 && !d.bez_ring && !d.fuse_ring && !d.stk_ovf && !d.fbvh2 && !d.fbleaf && !d.fsph && !d.fid && !d.chains &&
           !d.leaves && !d.leaf_cls && !d.mats && !d.texs && !d.ranvec && !d.perm && !d.order && !d.teximg && !d.gleaf &&
           !d.leaf_pos && !d.g0bvh2 && !d.g0bleaf && !d.rot;
}

// ---------------------------------------------------------------- the checks of one built scene
struct Expect { int sphere_leaves, curve_leaves, generic_leaves, rot_entries; bool solo, any_time, direct, has_bez, shared; };

// a key that tells leaves apart: type, flip, material, chain ops and the geometry the record holds
std::string key_of(const SceneDesc& s, const Flat& L, bool boundary) {
    const Obj& o = s.objs[L.obj];
    Fnv f;
    f.vals(L.type, boundary ? 0 : L.flip, boundary ? 0 : o.mat, boundary ? (size_t)0 : L.ops.size());
    if (!boundary) for (const ChainOpRec& op : L.ops) f.vals(op.op, op.x, op.y, op.z);
    if (L.type == LEAF_SPHERE || L.type == LEAF_KLEIN) f.vals(o.c0[0], o.c0[1], o.c0[2]);
    if (L.type == LEAF_SPHERE) f.val(o.r * o.r);
    if (L.type == LEAF_MSPHERE) f.vals(o.c0[0], o.c0[1], o.c0[2], o.r * o.r, o.c1[0] - o.c0[0], o.t0, o.t1 - o.t0);
    if (L.type >= LEAF_RECT_XY && L.type <= LEAF_RECT_YZ) f.vals(o.a0, o.a1, o.b0, o.b1, o.k);
    if (L.type == LEAF_BEZIER) f.bytes(o.cp, sizeof o.cp);
    if (L.type == LEAF_MEDIUM) f.val(-(1 / o.r));
    return std::to_string(f.x);
}
std::string key_of(const HostScene& h, int id) {
    const LeafInfo& li = h.leaves[(size_t)id];
    Fnv f;
    const size_t n_ops = li.chain >= 0 ? (size_t)h.chains[(size_t)li.chain].n : 0;
    f.vals(li.type, li.flip, li.mat, n_ops);
    for (size_t k = 0; k < n_ops; ++k) { const ChainOpRec& op = h.chains[(size_t)li.chain].ops[k]; f.vals(op.op, op.x, op.y, op.z); }
    const size_t l = (size_t)li.local;
    if (li.type == LEAF_SPHERE) f.vals(h.sph[l].cx, h.sph[l].cy, h.sph[l].cz, h.sph[l].rr);
    if (li.type == LEAF_KLEIN) f.vals(h.klein[l].cx, h.klein[l].cy, h.klein[l].cz);
    if (li.type == LEAF_MSPHERE) f.vals(h.msph[l].c0x, h.msph[l].c0y, h.msph[l].c0z, h.msph[l].rr, h.msph[l].dcx, h.msph[l].t0, h.msph[l].den);
    if (li.type >= LEAF_RECT_XY && li.type <= LEAF_RECT_YZ) f.vals(h.rect[l].a0, h.rect[l].a1, h.rect[l].b0, h.rect[l].b1, h.rect[l].k);
    if (li.type == LEAF_BEZIER) f.bytes(h.bez[l].cp, sizeof h.bez[l].cp);
    if (li.type == LEAF_MEDIUM) f.val(h.med[l].neg_inv_density);
    return std::to_string(f.x);
}

// every primitive under a tree ref lies in every box above it; `seen` counts the leaf ids reached.
// ids_of(leaf record) lists a leaf's ids; pos_of[id] = the flattened leaf (list position) of a leaf id.
template <class Ids>
void walk2(const SceneDesc& s, const FlatScene& fs, const HostVec<BvhNode2>& n2, const HostVec<BvhLeaf>& lf, int32_t ref, bool time0,
           int bez_base, const std::vector<int>& pos_of, Ids ids_of, std::vector<int>& under, std::map<int, int>& seen) {
    if (ref < 0) {
        std::vector<int> ids;
        if (~ref >= kDirectCurve) ids.push_back(bez_base + (~ref - kDirectCurve));  // a single curve, by the ref itself
        else ids = ids_of(lf[(size_t)~ref]);
        for (int id : ids) { under.push_back(id); ++seen[id]; }
        return;
    }
    const BvhNode2& M = n2[(size_t)ref];
    for (int side = 0; side < 2; ++side) {
        std::vector<int> sub;
        walk2(s, fs, n2, lf, side ? M.r : M.l, time0, bez_base, pos_of, ids_of, sub, seen);
        float lo[3], hi[3];
        for (int k = 0; k < 3; ++k) { lo[k] = M.b[2 * k + side]; hi[k] = M.b[6 + 2 * k + side]; }
        std::vector<double> pts;
        for (int id : sub) {
            const double r = hull_points(s, fs.world[(size_t)pos_of[(size_t)id]], time0, pts);
            const Obj& o = s.objs[fs.world[(size_t)pos_of[(size_t)id]].obj];
            const bool unbounded = fs.world[(size_t)pos_of[(size_t)id]].type == LEAF_MSPHERE && !(o.t1 - o.t0 != 0.0);
            if (unbounded) CHECK(lo[0] <= -1e30f && hi[0] >= 1e30f);
            else CHECK(inside(pts, r, lo, hi));
        }
        under.insert(under.end(), sub.begin(), sub.end());
    }
}

void check_scene(const SceneDesc& s, int world, const BuildOptions& opt, const HostScene& h, const Expect& ex) {
    FlatScene fs;
    std::vector<ChainOpRec> ops;
    flatten(s, world, 0, ops, fs, fs.world);
    const DevScene& d = h.d;
    CHECK(pointers_null(d));
    // leaf ids: leaf_base partitions [0, n_leaves) by the flattened list's own counts
    int cnt[kLeafTypes] = {0};
    for (const Flat& L : fs.world) ++cnt[L.type];
    for (const auto& b : fs.bounds) for (const Flat& L : b) ++cnt[L.type];
    const int n_rect = cnt[LEAF_RECT_XY] + cnt[LEAF_RECT_XZ] + cnt[LEAF_RECT_YZ];
    const int want_base[kLeafTypes] = {0, cnt[0], cnt[0] + cnt[1], cnt[0] + cnt[1], cnt[0] + cnt[1], cnt[0] + cnt[1] + n_rect,
                                       cnt[0] + cnt[1] + n_rect + cnt[LEAF_BEZIER], cnt[0] + cnt[1] + n_rect + cnt[LEAF_BEZIER] + cnt[LEAF_MEDIUM]};
    CHECK(std::memcmp(want_base, d.leaf_base, sizeof want_base) == 0);
    const int n_leaves = want_base[LEAF_KLEIN] + cnt[LEAF_KLEIN];
    CHECK(d.n_leaves == n_leaves && (int)h.leaves.size() == n_leaves);
    CHECK(d.n_sph == cnt[0] && d.n_msph == cnt[1] && d.n_rect == n_rect && d.n_bez == cnt[LEAF_BEZIER] && d.n_med == cnt[LEAF_MEDIUM] && d.n_klein == cnt[LEAF_KLEIN]);
    if ((int)h.leaves.size() != n_leaves) return;
    for (int id = 0; id < n_leaves; ++id) {
        const LeafInfo& li = h.leaves[(size_t)id];
        CHECK(li.type >= 0 && li.type < kLeafTypes && id - d.leaf_base[li.type] == li.local);
        CHECK(h.leaf_cls[(size_t)id] == (uint8_t)li.mtype);
    }
    // every flattened leaf owns exactly one leaf id: the multisets of keys agree
    std::map<std::string, int> bal;
    for (const Flat& L : fs.world) ++bal[key_of(s, L, false)];
    for (const auto& b : fs.bounds) for (const Flat& L : b) ++bal[key_of(s, L, true)];
    for (int id = 0; id < n_leaves; ++id) --bal[key_of(h, id)];
    bool balanced = true;
    for (const auto& kv : bal) balanced = balanced && kv.second == 0;
    CHECK(balanced);
    // order: a permutation following list order; none with media.  pos_of: leaf id -> list position
    std::vector<int> pos_of((size_t)n_leaves, -1);
    if (cnt[LEAF_MEDIUM] > 0) {
        CHECK(h.order.empty() && d.n_order == 0);
    } else {
        CHECK((int)h.order.size() == n_leaves && d.n_order == n_leaves && fs.world.size() == (size_t)n_leaves);
        for (size_t k = 0; k < h.order.size() && k < fs.world.size(); ++k) {
            const int id = h.order[k];
            CHECK(id >= 0 && id < n_leaves && pos_of[(size_t)id] == -1);
            if (id < 0 || id >= n_leaves) return;
            pos_of[(size_t)id] = (int)k;
            CHECK(key_of(h, id) == key_of(s, fs.world[k], false));
            if (h.generic) CHECK(h.leaf_pos[(size_t)id] == (int32_t)k);
        }
    }
    if (h.generic) CHECK((int)h.leaf_pos.size() == n_leaves && d.n_gleaf == (int)h.gleaf.size() && d.n_rot == (int)h.rot.size());
    else CHECK(h.gleaf.empty() && h.leaf_pos.empty() && h.rot.empty() && h.g0bvh2.empty());
    // coverage of the record arrays: tree ranges and group ranges tile each exactly once
    std::vector<int> cov[4] = {std::vector<int>((size_t)d.n_sph, 0), std::vector<int>((size_t)d.n_msph, 0),
                               std::vector<int>((size_t)d.n_rect, 0), std::vector<int>((size_t)d.n_bez, 0)};
    auto slot = [](int type) { return type == LEAF_SPHERE ? 0 : type == LEAF_MSPHERE ? 1 : type == LEAF_BEZIER ? 3 : 2; };
    int n_tree_groups = 0;
    for (const std::vector<Group>* gs : {&h.groups, &h.bgroups})
        for (const Group& G : *gs) {
            if (G.type == GROUP_BVH) { ++n_tree_groups; continue; }
            if (G.type == LEAF_MEDIUM || G.type == LEAF_KLEIN) continue;
            CHECK(G.begin >= 0 && G.begin < G.end && G.end <= (int)cov[slot(G.type)].size());
            for (int k = G.begin; k < G.end && k < (int)cov[slot(G.type)].size(); ++k) {
                ++cov[slot(G.type)][(size_t)k];
                const int id = d.leaf_base[G.type] + k;
                CHECK(h.leaves[(size_t)id].type == G.type && (gs == &h.bgroups || h.leaves[(size_t)id].chain == G.chain));
            }
        }
    const bool use_tree = n_tree_groups == 1;
    CHECK(n_tree_groups <= 1 && use_tree == (ex.sphere_leaves + ex.curve_leaves + ex.generic_leaves > 0));
    // the trees: every leaf's box (and every box above it) holds its primitive; the leaves they reach
    std::map<int, int> seen;
    std::vector<int> under;
    if (use_tree && h.generic) {
        auto ids = [&](const BvhLeaf& L) { CHECK(L.sn == 0 && L.mn == 0 && L.bn == 0 && L.gn >= 1); return std::vector<int>(h.gleaf.begin() + L.gb, h.gleaf.begin() + L.gb + L.gn); };
        walk2(s, fs, h.bvh2, h.bleaf, d.bvh2_root, false, d.leaf_base[LEAF_BEZIER], pos_of, ids, under, seen);
        for (const auto& kv : seen) { const LeafInfo& li = h.leaves[(size_t)kv.first]; if (li.type != LEAF_BEZIER) ++cov[slot(li.type)][(size_t)li.local]; CHECK(kv.second == 1); }
        if (!h.g0bleaf.empty()) {
            std::map<int, int> seen0;
            under.clear();
            walk2(s, fs, h.g0bvh2, h.g0bleaf, d.g0bvh2_root, true, d.leaf_base[LEAF_BEZIER], pos_of, ids, under, seen0);
            CHECK(seen0 == seen && (int)h.gleaf.size() == 2 * (int)seen.size());
        } else {
            CHECK(h.gleaf.size() == seen.size());
        }
    } else if (use_tree) {
        auto ids = [&](const BvhLeaf& L) {
            std::vector<int> v;
            for (int k = 0; k < L.sn; ++k) v.push_back(d.leaf_base[LEAF_SPHERE] + L.sb + k);
            for (int k = 0; k < L.mn; ++k) v.push_back(d.leaf_base[LEAF_MSPHERE] + L.mb + k);
            for (int k = 0; k < L.bn; ++k) v.push_back(d.leaf_base[LEAF_BEZIER] + L.bb + k);
            CHECK(L.gn == 0);
            return v;
        };
        // (with media the list order is not kept: the tree's leaves are world leaves of segment 0, found by key)
        if (cnt[LEAF_MEDIUM] > 0)
            for (int id = 0; id < n_leaves; ++id)
                for (size_t k = 0; k < fs.world.size(); ++k)
                    if (pos_of[(size_t)id] < 0 && h.leaves[(size_t)id].chain == -1 && key_of(h, id) == key_of(s, fs.world[k], false)) pos_of[(size_t)id] = (int)k;
        walk2(s, fs, h.bvh2, h.bleaf, d.bvh2_root, false, d.leaf_base[LEAF_BEZIER], pos_of, ids, under, seen);
        for (const auto& kv : seen) { const LeafInfo& li = h.leaves[(size_t)kv.first]; ++cov[slot(li.type)][(size_t)li.local]; CHECK(kv.second == 1); }
    }
    for (const auto& c : cov) for (int v : c) CHECK(v == 1);
    // the sphere form of the time-0 tree: fid names the sphere fsph[k] restates, bit for bit
    if (!h.fbvh2.empty()) {
        CHECK(h.fid.size() == h.fsph.size() && d.n_fsph == (int)h.fsph.size() && d.n_fbvh2 == (int)h.fbvh2.size() && d.n_fbleaf == (int)h.fbleaf.size());
        std::map<int, int> seen0;
        under.clear();
        walk2(s, fs, h.fbvh2, h.fbleaf, d.fbvh2_root, true, d.leaf_base[LEAF_BEZIER], pos_of, [&](const BvhLeaf& L) {
            CHECK(L.mn == 0 && L.bn == 0 && L.gn == 0);
            return std::vector<int>(h.fid.begin() + L.sb, h.fid.begin() + L.sb + L.sn); }, under, seen0);
        CHECK(seen0 == seen);
        for (size_t k = 0; k < h.fsph.size() && k < h.fid.size(); ++k) {
            const LeafInfo& li = h.leaves[(size_t)h.fid[k]];
            SphereRec want{};
            if (li.type == LEAF_SPHERE) want = h.sph[(size_t)li.local];
            else {
                const MSphereRec& m = h.msph[(size_t)li.local];
                want = SphereRec{m.c0x + m.dcx * ((0 - m.t0) / m.den), m.c0y + m.dcy * ((0 - m.t0) / m.den), m.c0z + m.dcz * ((0 - m.t0) / m.den), m.rr};
                CHECK(std::memcmp(li.c, &want, 3 * sizeof(double)) == 0);
            }
            CHECK(std::memcmp(&want, &h.fsph[k], sizeof want) == 0);
        }
        bool direct = true;
        for (size_t k = 0; k < h.fbleaf.size(); ++k) direct = direct && h.fbleaf[k].sn == 1 && h.fbleaf[k].sb == (int32_t)k;
        CHECK(direct == ex.direct);
        CHECK((d.tree0_any_time != 0) == ex.any_time);
    } else {
        CHECK(!ex.direct && !ex.any_time && d.tree0_any_time == 0 && h.fsph.empty() == h.fid.empty());
    }
    // the BVH4 of a curve tree reaches the same leaves under boxes that hold them
    if (d.bvh_has_bez) {
        CHECK(!h.bvh4.empty() && d.n_bvh4 == (int)h.bvh4.size() && d.bvh4_root == 0 && d.stack4 >= 1);
        std::map<int32_t, int> refs4, refs2;
        for (const BvhNode4& N : h.bvh4) for (int j = 0; j < N.n; ++j) if (N.ref[j] < 0) ++refs4[N.ref[j]];
        for (const BvhNode2& M : h.bvh2) for (int32_t r : {M.l, M.r}) if (r < 0) ++refs2[r];
        CHECK(refs4 == refs2);
        bool direct_seen = false;
        for (const auto& kv : refs2) direct_seen = direct_seen || ~kv.first >= kDirectCurve;
        CHECK(direct_seen);
    } else {
        CHECK(h.bvh4.empty() && d.n_bvh4 == 0);
    }
    // flags and rt_tree_info
    CHECK((d.bvh_solo != 0) == ex.solo && (d.bvh_has_bez != 0) == ex.has_bez && (d.msph_shared != 0) == ex.shared);
    const rt_tree_info& t = h.tree;
    CHECK(t.sphere_leaves == ex.sphere_leaves && t.curve_leaves == ex.curve_leaves && t.generic_leaves == ex.generic_leaves);
    CHECK(t.group_leaves == n_leaves - ex.sphere_leaves - ex.curve_leaves - ex.generic_leaves);
    CHECK(t.rot_entries == ex.rot_entries && t.generic_min == (int32_t)opt.generic_min);
    CHECK(t.nodes == (int)h.bvh2.size() && t.nodes0 == (int)(h.generic ? h.g0bvh2.size() : h.fbvh2.size()));
    CHECK((int)seen.size() == ex.sphere_leaves + ex.curve_leaves + ex.generic_leaves);
    CHECK(d.lane_stack >= t.depth && d.lane_stack >= t.depth0 && d.lane_stack <= kLaneStack);
}

bool g_first = true;
void run(const char* name, Builder& b, int world, BuildOptions opt, const Expect& ex) {
    g_fail.clear();
    uint64_t dig[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        opt.threads = pass ? 8 : 1;
        HostScene h;
        std::string err;
        const int rc = build_scene(b.s, world, opt, h, err);
        CHECK(rc == 0 && err.empty());
        if (rc) break;
        dig[pass] = digest(h);
        if (pass == 0) check_scene(b.s, world, opt, h, ex);
        else CHECK(dig[0] == dig[1]);
    }
    std::printf("%s\"%s\": {\"failed\": [", g_first ? "" : ", ", name);
    for (size_t k = 0; k < g_fail.size(); ++k) std::printf("%s\"%s\"", k ? ", " : "", g_fail[k].c_str());
    std::printf("], \"digest\": \"%016llx\"}", (unsigned long long)dig[0]);
    g_first = false;
}
void run_error(const char* name, Builder& b, int world, const char* want) {
    HostScene h;
    std::string err;
    const int rc = build_scene(b.s, world, BuildOptions{}, h, err);
    std::printf(", \"%s\": {\"failed\": [%s], \"text\": \"%s\"}", name, (rc == 1 && err == want) ? "" : "\"text\"", err.c_str());
}

int spheres_ab(Builder& b, double t0b, double t1b, bool zero_den) {
    std::vector<int> kids;
    for (int i = 0; i < 24; ++i) kids.push_back(b.sphere(i % 6 - 2.5, 0.4 + (i % 3) * 0.1, i / 6 - 1.5, 0.3 + 0.01 * i, i % 3));
    for (int i = 0; i < 8; ++i) kids.push_back(b.msphere(i - 3.5, 2.0, 0.5 * i, 0.25, i < 4 ? 0.0 : t0b, i < 4 ? 1.0 : t1b));
    if (zero_den) { b.s.objs[(size_t)kids.back()].t0 = 0.5; b.s.objs[(size_t)kids.back()].t1 = 0.5; }
    return b.list(kids);
}
// (d), (e): a ground rect, n_box boxes each under translate o rotate-y (distinct angles), chained spheres, a chained
// moving sphere, a flipped rect, a rect with a non-finite bound
int generic_scene(Builder& b, int n_box, int* n_generic, int* n_rot) {
    std::vector<int> kids;
    kids.push_back(b.rect(1, -20, 20, -20, 20, 0.0));
    for (int i = 0; i < n_box; ++i) kids.push_back(b.translate(b.rotate_y(b.box(0, 0, 0, 1, 1 + 0.1 * i, 1), 5.0 + 7.0 * i), 2.0 * i - 6, 0, -3));
    for (int i = 0; i < 4; ++i) kids.push_back(b.translate(b.sphere(0, 0.5, 0, 0.5, 1), i, 0.5, 2));
    kids.push_back(b.translate(b.rotate_y(b.msphere(0, 1, 0, 0.3, 0.0, 1.0), 30), 1, 0, 4));
    kids.push_back(b.flip(b.rect(0, -1, 1, 0, 2, 6.0)));
    kids.push_back(b.rect(2, 0, INFINITY, 0, 1, -7.0));
    kids.push_back(b.sphere(0, 1, 0, 1.0, 2));
    kids.push_back(b.msphere(3, 1, 0, 0.4, 0.0, 1.0));
    const int boxes_in = std::min(n_box, kMaxRot - 1);       // the table also holds the empty rotation (ground, flipped rect)
    *n_generic = 1 + 6 * boxes_in + 4 + 1 + 1;
    *n_rot = 1 + boxes_in;
    return b.list(kids, O_BVH);
}

// (on a thread with a large stack: the cycle case recurses 10 000 levels through instrumented frames)
void* body(void*) {
    std::printf("{");
    {   // (a) two shutters
        Builder b;
        const int w = spheres_ab(b, 0.25, 0.75, false);
        run("a", b, w, BuildOptions{}, Expect{32, 0, 0, 0, true, false, true, false, false});
    }
    {   // (b) one shared shutter, and den == 0 on one sphere: not shared any more by the bits, unbounded box
        Builder b;
        const int w = spheres_ab(b, 0.0, 1.0, false);
        run("b_shared", b, w, BuildOptions{}, Expect{32, 0, 0, 0, true, false, true, false, true});
        Builder z;
        const int wz = spheres_ab(z, 0.0, 1.0, true);
        run("b_zero_den", z, wz, BuildOptions{}, Expect{32, 0, 0, 0, true, false, true, false, false});
    }
    {   // (c) below bvh_min: groups only
        Builder b;
        std::vector<int> kids;
        for (int i = 0; i < 10; ++i) kids.push_back(b.sphere(i, 0.5, 0, 0.5, i % 3));
        kids.push_back(b.msphere(0, 2, 0, 0.3, 0.0, 1.0));
        kids.push_back(b.rect(1, -5, 5, -5, 5, 0.0));
        run("c", b, b.list(kids), BuildOptions{}, Expect{0, 0, 0, 0, false, false, false, false, true});
    }
    for (const int n_box : {5, 20}) {               // (d), (e)
        Builder b;
        int n_gen = 0, n_rot = 0;
        const int w = generic_scene(b, n_box, &n_gen, &n_rot);
        BuildOptions opt;
        opt.generic_min = 8;
        run(n_box == 5 ? "d" : "e", b, w, opt, Expect{2, 0, n_gen, n_rot, false, false, false, false, true});
    }
    {   // (f) curves
        Builder b;
        std::vector<int> kids;
        for (int i = 0; i < 20; ++i) kids.push_back(b.bezier(0.5 * i - 5, 0, 0.3 * (i % 4), 0.05));
        for (int i = 0; i < 4; ++i) kids.push_back(b.sphere(2.0 * i - 3, 0.5, -2, 0.5));
        run("f", b, b.list(kids), BuildOptions{}, Expect{4, 20, 0, 0, false, false, false, true, false});
    }
    {   // (g) two media: three segments; a sphere listed twice; a Klein set
        Builder b;
        std::vector<int> kids;
        for (int i = 0; i < 18; ++i) kids.push_back(b.sphere(i % 6 - 2.5, 0.5, i / 6, 0.4, i % 3));
        const int twice = b.sphere(0, 3, 0, 0.7, 1);
        kids.push_back(twice);
        kids.push_back(b.medium(b.sphere(1, 1, 1, 2.0), 0.2));
        kids.push_back(b.rect(0, -3, 3, 0, 3, -4.0));
        kids.push_back(twice);
        kids.push_back(b.medium(b.translate(b.box(0, 0, 0, 2, 2, 2), 4, 0, 0), 0.01));
        kids.push_back(b.klein(0, 0, -6));
        kids.push_back(b.sphere(5, 0.5, 5, 0.5));
        run("g", b, b.list(kids), BuildOptions{}, Expect{19, 0, 0, 0, false, true, true, false, false});
    }
    // (h) the failures, with the commit's texts
    { Builder b; const int m = b.medium(b.medium(b.sphere(0, 0, 0, 1), 0.1), 0.1); run_error("nested", b, m, "constant media cannot be nested"); }
    { Builder b; const int m = b.medium(b.bezier(0, 0, 0, 0.1), 0.1); run_error("curve_boundary", b, m, "a constant medium's boundary may hold spheres, rects, boxes and instances only"); }
    { Builder b; int o = b.sphere(0, 0, 0, 1); for (int i = 0; i < 5; ++i) o = b.translate(o, 1, 0, 0); run_error("depth5", b, o, "instance nesting deeper than 4 transforms"); }
    { Builder b; const int l = b.list({b.sphere(0, 0, 0, 1)}); b.s.objs[(size_t)l].kids.push_back(l); run_error("cycle", b, l, "object graph too deep (cycle?)"); }
    { Builder b; b.s.have_cam = false; run_error("no_camera", b, b.sphere(0, 0, 0, 1), "rt_scene_commit: no camera set (rt_set_camera)"); }
    { Builder b; DevTexture t{}; t.type = TEX_NOISE; b.s.texs.push_back(t); run_error("noise", b, b.sphere(0, 0, 0, 1), "rt_scene_commit: noise/marble texture needs rt_set_perlin_tables"); }
    std::printf("}\n");
    return nullptr;
}
}  // namespace

int main() {
    pthread_attr_t at;
    pthread_attr_init(&at);
    pthread_attr_setstacksize(&at, (size_t)512 << 20);
    pthread_t th;
    if (pthread_create(&th, &at, body, nullptr)) return 2;
    pthread_join(th, nullptr);
    return 0;
}
