// rt_build.cpp — build_scene: the reference's object tree flattened into grouped leaves, the BVH builds
// (rt_bvh.h) and the record arrays of the device scene, stage by stage (no device code, no HIP).
#include "rt_build.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "rt_leafbox.h"

namespace rtamd {
namespace {
using Src = std::vector<std::pair<int, int>>;        // (LeafType, index in the type's array) per tree-order entry

// one primitive per leaf (measured fastest for sphere trees; for C5's curve tree, with the exact SAH sweep
// below 65 536 primitives, +1.5 % / +0.6 % over two per leaf: profiles/r02/ab_c5, profiles/r03/c5walk/ab_leaf1.log)
constexpr int kLeafMax = 1;

int fail_with(std::string* err, const char* msg) { *err = msg; return 1; }
bool is_rect(const int type) { return type >= LEAF_RECT_XY && type <= LEAF_RECT_YZ; }
// the generic tree's leaves whose records are appended in tree order (tree_records): rects and triangles
bool is_appended(const int type) { return is_rect(type) || type == LEAF_TRI; }
bool has_triangle(const Flattener& f) {
    return std::any_of(f.leaves.begin(), f.leaves.end(), [](const LeafTmp& L) { return L.type == LEAF_TRI; });
}
// what the sphere form of the world tree takes: world-level spheres and moving spheres
bool world_sphere(const LeafTmp& L) { return L.chain == -1 && (L.type == LEAF_SPHERE || L.type == LEAF_MSPHERE); }

// ------------------------------------------------------------ records
SphereRec sphere_rec(const Obj& o) { return SphereRec{o.c0[0], o.c0[1], o.c0[2], o.r * o.r}; }
MSphereRec msphere_rec(const Obj& o) {
    MSphereRec m{};
    m.c0x = o.c0[0]; m.c0y = o.c0[1]; m.c0z = o.c0[2]; m.rr = o.r * o.r;
    m.dcx = o.c1[0] - o.c0[0]; m.dcy = o.c1[1] - o.c0[1]; m.dcz = o.c1[2] - o.c0[2];
    m.t0 = o.t0; m.den = o.t1 - o.t0;
    return m;
}
// a moving sphere at center(0), by the kernel's own operations (c0 + dc * ((0 - t0) / den), IEEE f64, no
// contraction), so the plain sphere test of this record is bit for bit the moving-sphere test of a time-0 ray
SphereRec msphere_center0(const MSphereRec& m) {
    const double frac = (0.0 - m.t0) / m.den;
    return SphereRec{m.c0x + m.dcx * frac, m.c0y + m.dcy * frac, m.c0z + m.dcz * frac, m.rr};
}
RectRec rect_rec(const Obj& o) {
    RectRec r{};
    r.a0 = o.a0; r.a1 = o.a1; r.b0 = o.b0; r.b1 = o.b1; r.k = o.k;
    return r;
}
BezierRec bezier_rec(const Obj& o, const uint32_t order) {
    BezierRec b{};
    for (int k = 0; k < 12; ++k) b.cp[k] = o.cp[k];
    b.w1 = o.width / 2;                 // bezier.scm:63-65
    b.w2 = b.w1 * b.w1;
    b.eps8 = 8 * (o.width / 20);
    b.order = order;                    // the flattened list position
    return b;
}
TriRec tri_rec(const Obj& o) {
    TriRec t{};
    for (int k = 0; k < 3; ++k) { t.v0[k] = o.cp[k]; t.v1[k] = o.cp[3 + k]; t.v2[k] = o.cp[6 + k]; }
    return t;
}
TriUv tri_uv(const Obj& o) {
    TriUv q{};
    q.has = o.has_uv ? 1 : 0;
    for (int k = 0; k < 3; ++k) { q.u[k] = o.uv[k]; q.v[k] = o.uv[3 + k]; }
    return q;
}
TriNrm tri_nrm(const Obj& o) {
    TriNrm q{};
    q.has = o.has_nrm ? 1 : 0;
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) q.n[i][k] = o.nrm[3 * i + k];
    return q;
}
// the extend-side part of a leaf's LeafInfo, all but `local` (shade_fields adds the rest); a triangle's
// normal is formed here, once (tri_normal: a degenerate one, refused by the add calls, keeps 0 0 0)
LeafInfo leaf_info(const LeafTmp& L, const Obj& o) {
    LeafInfo li{};
    li.type = L.type; li.chain = L.chain; li.mat = o.mat; li.flip = L.flip;
    if (L.type == LEAF_SPHERE || L.type == LEAF_MSPHERE) li.inv_r = 1.0 / o.r;
    if (L.type == LEAF_TRI) (void)tri_normal(o.cp, o.cp + 3, o.cp + 6, li.c);
    return li;
}
LeafGeom leaf_geom(const LeafTmp& L, const Obj& o) {
    LeafGeom g{};
    g.type = L.type;
    for (int k = 0; k < 3; ++k) { g.c0[k] = o.c0[k]; g.c1[k] = o.c1[k]; }
    g.r = o.r; g.t0 = o.t0; g.t1 = o.t1;
    g.a0 = o.a0; g.a1 = o.a1; g.b0 = o.b0; g.b1 = o.b1; g.k = o.k;
    if (L.type == LEAF_TRI) for (int k = 0; k < 9; ++k) g.v[k] = o.cp[k];
    return g;
}
const ChainOpRec* chain_ops(const Flattener& f, const int ch, int& n) {
    n = ch >= 0 ? (int)f.chains[ch].size() : 0;
    return ch >= 0 ? f.chains[ch].data() : nullptr;
}

// An L2 bound on the world-space distance from the origin of every point a
// ray can start from: all leaves (instance chains applied: rotations keep the
// norm, translations add theirs), medium boundaries, the camera; x4 for the
// off-surface points curves report (Q10) and motion extrapolation.
double scene_radius(const SceneDesc& s, const Flattener& f, const int nt) {
    auto n3 = [](const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    auto chain_len = [&](int ch) {
        double t = 0;
        if (ch >= 0)
            for (const ChainOpRec& op : f.chains[ch])
                if (op.op == OP_TRANSLATE) t += std::sqrt(op.x * op.x + op.y * op.y + op.z * op.z);
        return t;
    };
    auto leaf_r = [&](const LeafTmp& L) {
        const Obj& o = s.objs[L.obj];
        double r = 0;
        switch (L.type) {
        case LEAF_SPHERE: r = n3(o.c0) + std::fabs(o.r); break;
        case LEAF_MSPHERE: r = 2 * std::max(n3(o.c0), n3(o.c1)) + std::fabs(o.r); break;
        case LEAF_BEZIER:
            for (int i = 0; i < 4; ++i) r = std::max(r, n3(o.cp + 3 * i));
            r += std::fabs(o.width);
            break;
        case LEAF_KLEIN: r = n3(o.c0) + 1200; break;
        case LEAF_MEDIUM: r = 0; break;
        case LEAF_TRI: r = std::max({n3(o.cp), n3(o.cp + 3), n3(o.cp + 6)}); break;
        default:
            r = std::sqrt(3.0) * std::max({std::fabs(o.a0), std::fabs(o.a1), std::fabs(o.b0), std::fabs(o.b1),
                                           std::fabs(o.k)});
        }
        return r + chain_len(L.chain);
    };
    double R = n3(s.cam + 9) + std::fabs(s.cam[21]);
    std::vector<double> part((size_t)nt, R);        // (max is order-free: a NaN radius never enters)
    parallel_for(f.leaves.size(), nt, [&](const size_t b, const size_t e) {
        double r = R;
        for (size_t i = b; i < e; ++i) r = std::max(r, leaf_r(f.leaves[i]));
        part[b / std::max<size_t>(1, (f.leaves.size() + (size_t)nt - 1) / (size_t)nt)] = r;
    });
    for (const double r : part) R = std::max(R, r);
    for (const auto& b : f.bounds) for (const LeafTmp& L : b) R = std::max(R, leaf_r(L));
    return 4 * R + 1;
}

// A SAH tree over refs (reordered into tree order); its build time is added to sah_ms
std::vector<BvhNode> sah_build(std::vector<PrimRef>& refs, const BuildOptions& opt, const bool singles, double& sah_ms) {
    BvhBuild bb{refs, {}};
    bb.leaf_max = kLeafMax;
    bb.sweep_max = opt.sweep_max;
    bb.singles = singles;
    bb.threads = opt.threads;
    const auto t0 = std::chrono::steady_clock::now();
    bb.build(0, (int)refs.size(), 0);
    sah_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return std::move(bb.nodes);
}

// ------------------------------------------------------------ stages
// A constant medium draws a random number inside its hit test, so its
// position in the object list matters (the draw happens only if the
// closest hit so far leaves part of its span): the leaves are cut into
// segments at each medium and evaluated segment by segment, each medium
// right after the objects that precede it.  Within a segment the order of
// the other primitives does not change the closest hit.
int cut_segments(const Flattener& f, std::vector<int>& seg) {
    seg.assign(f.leaves.size(), 0);
    int nseg = 1;
    for (size_t i = 0; i < f.leaves.size(); ++i) {
        seg[i] = nseg - 1;
        if (f.leaves[i].type == LEAF_MEDIUM) ++nseg;
    }
    return nseg;
}

// Which leaves the world tree takes.  Always the world-level (chain -1) spheres, moving spheres and curves
// of segment 0.  Generic tree leaves (include/rt.h, rt_add_bvh): rects under any chain or none and spheres /
// moving spheres under a chain, with a finite world-space box (rt_leafbox.h), in scenes of spheres, moving
// spheres and rects only.  A rect also needs its chain's rotation in the table the kernels test a ray's
// direction against (rot; at most kMaxRot).  They join the tree when there are at least opt.generic_min of
// them and the tree is built at all; else nothing differs from a build without them.
struct TreePlan {
    std::vector<int> in_tree;         // list positions, in list order
    bool generic = false;
    std::vector<char> is_gen;         // generic: by list position, a generic tree leaf
    std::vector<PrimRef> gen_ref;     // ... and its box
    bool gen(const size_t i) const { return generic && is_gen[i]; }
};
// Leaf i of the list as a generic tree leaf: its world-space box, and for a rect its chain's rotation entered
// in rot.  False: not one (a world-level sphere, a box that is not finite, a rect past a full table).
bool generic_ref(const SceneDesc& s, const Flattener& f, const size_t i, const double tlo, const double thi,
                 std::vector<RotEntry>& rot, PrimRef& r) {
    const LeafTmp& L = f.leaves[i];
    if (!is_appended(L.type) && L.chain < 0) return false;
    int n_ops = 0;
    const ChainOpRec* ops = chain_ops(f, L.chain, n_ops);
    r = PrimRef{};
    if (!leaf_world_box(leaf_geom(L, s.objs[L.obj]), ops, n_ops, tlo, thi, r.lo, r.hi)) return false;
    if (is_rect(L.type)) {
        RotEntry e{};
        for (int k = 0; k < n_ops; ++k)
            if (ops[k].op == OP_ROTATE_Y) { e.sc[e.n][0] = ops[k].x; e.sc[e.n][1] = ops[k].y; ++e.n; }
        size_t at = 0;
        while (at < rot.size() && (rot[at].n != e.n || std::memcmp(rot[at].sc, e.sc, sizeof e.sc) != 0)) ++at;
        if (at == rot.size()) {
            if (rot.size() >= (size_t)kMaxRot) return false;       // the table is full: the rect keeps its group
            rot.push_back(e);
        }
        rot[at].axes |= L.type == LEAF_RECT_YZ ? 1 : L.type == LEAF_RECT_XZ ? 2 : 4;   // the plane's normal
    }
    for (int k = 0; k < 3; ++k) r.c[k] = 0.5 * (r.lo[k] + r.hi[k]);
    r.leaf = (int)i;
    r.type = L.type;
    return true;
}
TreePlan choose_tree_leaves(const SceneDesc& s, const Flattener& f, const std::vector<int>& seg, const int nseg,
                            const BuildOptions& opt, std::vector<RotEntry>& rot) {
    TreePlan p;
    for (size_t i = 0; i < f.leaves.size(); ++i) {
        const LeafTmp& L = f.leaves[i];
        if (seg[i] == 0 && (world_sphere(L) || (L.chain == -1 && L.type == LEAF_BEZIER))) p.in_tree.push_back((int)i);
    }
    const size_t n_world = p.in_tree.size();
    const double tlo = std::min(std::min(s.cam[22], s.cam[23]), 0.0), thi = std::max(std::max(s.cam[22], s.cam[23]), 0.0);
    size_t n_gen = 0;
    bool plain = nseg == 1 && f.bounds.empty();
    for (const LeafTmp& L : f.leaves) plain = plain && L.type != LEAF_BEZIER && L.type != LEAF_KLEIN && L.type != LEAF_MEDIUM;
    // a scene with a triangle (plain: build_scene refused it otherwise) always gets the generic tree, whatever
    // its size: the tree is the only place a triangle is tested, apart from list_closest
    const bool tri = has_triangle(f);
    if (plain && (tri || f.leaves.size() >= opt.generic_min)) {
        p.gen_ref.resize(f.leaves.size());
        p.is_gen.assign(f.leaves.size(), 0);
        for (size_t i = 0; i < f.leaves.size(); ++i) {
            if (!generic_ref(s, f, i, tlo, thi, rot, p.gen_ref[i])) continue;
            p.is_gen[i] = 1;
            ++n_gen;
        }
    }
    p.generic = n_gen > 0 && (tri || (n_gen >= opt.generic_min && n_world + n_gen >= opt.bvh_min));
    if (!p.generic) { rot.clear(); return p; }
    p.in_tree.clear();
    for (size_t i = 0; i < f.leaves.size(); ++i)
        if (p.is_gen[i] || world_sphere(f.leaves[i])) p.in_tree.push_back((int)i);
    return p;
}

// Media forests (include/rt.h, rt_add_bvh).  A scene with a constant medium, no curve and no
// Klein set, in which some segment has at least opt.generic_min generic leaves: every segment is decided on
// its own by choose_tree_leaves' rule over that segment's counts, and each tree it gets is a generic one
// (also one of world-level spheres only: one walk).  The first kMaxSegTrees segments that qualify get
// trees; rot holds the rotations of all the trees' rects.  on = false: the scene commits as without forests.
constexpr int kMaxSegTrees = 8;
struct ForestPlan {
    bool on = false;
    std::vector<std::vector<int>> tree;   // per segment: the list positions its tree takes, in list order
    TreePlan leaves;                      // is_gen: by list position, in some tree; gen_ref: the generic leaves' boxes
};
ForestPlan choose_forest(const SceneDesc& s, const Flattener& f, const std::vector<int>& seg, const int nseg,
                         const BuildOptions& opt, std::vector<RotEntry>& rot) {
    ForestPlan p;
    if (f.bounds.empty()) return p;
    for (const LeafTmp& L : f.leaves)
        if (L.type == LEAF_BEZIER || L.type == LEAF_KLEIN) return p;
    const size_t n = f.leaves.size();
    const double tlo = std::min(std::min(s.cam[22], s.cam[23]), 0.0), thi = std::max(std::max(s.cam[22], s.cam[23]), 0.0);
    p.tree.resize((size_t)nseg);
    p.leaves.is_gen.assign(n, 0);
    p.leaves.gen_ref.resize(n);
    std::vector<RotEntry> table;
    int trees = 0;
    size_t i = 0;
    for (int sg = 0; sg < nseg && trees < kMaxSegTrees; ++sg) {
        const size_t b = i;
        while (i < n && seg[i] == sg) ++i;                     // [b, i): the segment's leaves, its medium last
        std::vector<RotEntry> with = table;                    // the table with this segment's rects
        std::vector<char> gen(i - b, 0);
        size_t n_gen = 0, n_world = 0;
        for (size_t j = b; j < i; ++j) {
            const LeafTmp& L = f.leaves[j];
            if (L.type == LEAF_MEDIUM) continue;
            if (world_sphere(L)) { ++n_world; continue; }
            gen[j - b] = generic_ref(s, f, j, tlo, thi, with, p.leaves.gen_ref[j]) ? 1 : 0;
            n_gen += (size_t)gen[j - b];
        }
        const bool take_gen = n_gen > 0 && n_gen >= opt.generic_min && n_world + n_gen >= opt.bvh_min;
        const bool take_world = n_world > 0 && n_world + (take_gen ? n_gen : 0) >= opt.bvh_min;
        if (take_gen) { table.swap(with); p.on = true; }
        for (size_t j = b; j < i; ++j)
            if ((take_gen && gen[j - b]) || (take_world && world_sphere(f.leaves[j]))) {
                p.tree[(size_t)sg].push_back((int)j);
                p.leaves.is_gen[j] = 1;
            }
        trees += p.tree[(size_t)sg].empty() ? 0 : 1;
    }
    if (p.on) { rot.swap(table); p.leaves.generic = true; }
    return p;
}

// The tree leaves' boxes, in list order: a moving sphere over every time a ray can carry (rt_bvh.h)
std::vector<PrimRef> prim_boxes(const SceneDesc& s, const Flattener& f, const TreePlan& p, const int threads) {
    const double tlo = std::min(std::min(s.cam[22], s.cam[23]), 0.0), thi = std::max(std::max(s.cam[22], s.cam[23]), 0.0);
    std::vector<PrimRef> refs(p.in_tree.size());
    parallel_for(p.in_tree.size(), threads, [&](const size_t jb, const size_t je) {
      for (size_t j = jb; j < je; ++j) {
        const size_t i = (size_t)p.in_tree[j];
        const LeafTmp& L = f.leaves[i];
        const Obj& o = s.objs[L.obj];
        if (p.gen(i)) { refs[j] = p.gen_ref[i]; continue; }
        PrimRef r{};
        r.leaf = (int)i;
        r.type = L.type;
        if (L.type == LEAF_BEZIER) {
            const double w1 = std::fabs(o.width / 2);
            for (int k = 0; k < 3; ++k) {
                r.lo[k] = std::min(std::min(o.cp[k], o.cp[3 + k]), std::min(o.cp[6 + k], o.cp[9 + k])) - w1;
                r.hi[k] = std::max(std::max(o.cp[k], o.cp[3 + k]), std::max(o.cp[6 + k], o.cp[9 + k])) + w1;
            }
        } else {
            leaf_local_box(leaf_geom(L, o), tlo, thi, r.lo, r.hi);
        }
        pad_box(r.lo, r.hi);
        for (int k = 0; k < 3; ++k) r.c[k] = 0.5 * (r.lo[k] + r.hi[k]);
        refs[j] = r;
      }
    });
    return refs;
}

// tree order -> sphere / moving-sphere / curve array indices: entry i counts those before tree position i
struct Prefix {
    std::vector<int> ns, nm, nb;
    int spheres() const { return ns.back(); }
    int moving() const { return nm.back(); }
    int curves() const { return nb.back(); }
};

// The world tree over h.refs: the SAH build, its traversal layout with leaves as ranges of the record
// arrays (generic: of gleaf), and for curve trees the direct curve refs and the BVH4.  Returns the f64
// margin its f32 boxes were widened by.
double world_tree(const SceneDesc& s, const BuildOptions& opt, const bool generic, HostScene& h, Prefix& pre) {
    std::vector<PrimRef>& refs = h.refs;
    DevScene& d = h.d;
    h.threads = opt.threads;
    h.bvh_nodes = sah_build(refs, opt, false, h.sah_ms);
    COMMIT_MARK("sah");
    pre.ns.assign(refs.size() + 1, 0); pre.nm.assign(refs.size() + 1, 0); pre.nb.assign(refs.size() + 1, 0);
    for (size_t i = 0; i < refs.size(); ++i) {
        pre.ns[i + 1] = pre.ns[i] + (refs[i].type == LEAF_SPHERE);
        pre.nm[i + 1] = pre.nm[i] + (refs[i].type == LEAF_MSPHERE);
        pre.nb[i + 1] = pre.nb[i] + (refs[i].type == LEAF_BEZIER);
    }
    d.bvh_has_bez = pre.curves() > 0 ? 1 : 0;
    COMMIT_MARK("prefix");
    // f32 box margin: 2^-21 x a radius bound R on everything a ray can start
    // from (x4 included, see scene_radius).  With the ray's 1/d and o/d
    // formed in f32 (rt_boxray.h, where the bound is derived) a slab end
    // carries at most (3.5 |box - o| + 2 |o|) 2^-24 of rounding; |o| <= R and
    // |box| <= R / 4 make that 6.4 x 2^-24 R, and the margin is 8 x 2^-24 R:
    // 1.25x the bound (tests/csrc/box_ray_check.cpp holds it to that).
    const double margin = std::ldexp(scene_radius(s, h.f, opt.threads), -21);
    d.bvh_pad = (float)margin;
    COMMIT_MARK("radius");
    const std::vector<int>&ns = pre.ns, &nm = pre.nm, &nb = pre.nb;
    flatten_bvh2(h.bvh_nodes, margin, [&](int b, int e) {
        if (generic) return BvhLeaf{0, 0, 0, 0, 0, 0, b, e - b};      // every leaf by its id (gleaf)
        return BvhLeaf{ns[b], ns[e] - ns[b], nm[b], nm[e] - nm[b], nb[b], nb[e] - nb[b], 0, 0};
    }, h.bvh2, h.bleaf, d.bvh2_root, d.lane_stack, opt.threads);
    h.tree.depth = d.lane_stack;
    COMMIT_MARK("flatten2");
    if (d.bvh_has_bez) {                             // single-curve leaves: direct refs (kDirectCurve)
        auto direct = [&](int32_t& ref) {
            if (ref >= 0) return;
            const BvhLeaf& L = h.bleaf[~ref];
            if (L.sn == 0 && L.mn == 0 && L.bn == 1 && L.bb < kDirectCurve) ref = ~(kDirectCurve + L.bb);
        };
        for (BvhNode2& M : h.bvh2) { direct(M.l); direct(M.r); }
        direct(d.bvh2_root);
        COMMIT_MARK("bvh2");
        int32_t stack4 = 0;
        const int32_t root4 = collapse_bvh4(h.bvh2, d.bvh2_root, h.bvh4, stack4, opt.threads);
        if (!h.bvh4.empty()) { d.n_bvh4 = (int)h.bvh4.size(); d.bvh4_root = root4; d.stack4 = stack4; }
        COMMIT_MARK("bvh4");
    }
    h.groups.push_back(Group{GROUP_BVH, -1, 0, (int)h.bvh_nodes.size()});
    return margin;
}

// Leaf L's record and LeafInfo into slot `local` of its type's arrays (sized by the caller; threads may fill
// distinct slots).  Leaf id = leaf_base[type] + local, so every record gets a LeafInfo.  pos: the leaf's list
// position; < 0 for a medium's boundary leaf, which is never a closest hit and gets a placeholder.
void put_record(const SceneDesc& s, const LeafTmp& L, const int pos, const int local, HostScene& h) {
    const Obj& o = s.objs[L.obj];
    LeafLists& ll = h.ll;
    LeafInfo li = leaf_info(L, o);
    li.local = local;
    if (pos < 0) { li.chain = -1; li.mat = 0; li.flip = 0; }
    const size_t k = (size_t)local;
    switch (L.type) {
    case LEAF_SPHERE: h.sph[k] = sphere_rec(o); ll.sph[k] = li; break;
    case LEAF_MSPHERE: h.msph[k] = msphere_rec(o); ll.msph[k] = li; break;
    case LEAF_BEZIER: h.bez[k] = bezier_rec(o, (uint32_t)std::max(pos, 0)); ll.bez[k] = li; break;   // (boundaries hold no curves)
    case LEAF_KLEIN: h.klein[k] = KleinRec{o.c0[0], o.c0[1], o.c0[2], 0.0}; ll.klein[k] = li; break;
    case LEAF_TRI: h.tri[k] = tri_rec(o); h.triuv[k] = tri_uv(o); h.trinrm[k] = tri_nrm(o); ll.tri[k] = li; break;
    default: h.rect[k] = rect_rec(o); ll.rect[k] = li;           // the three axis types share the rect array
    }
    if (pos < 0) return;
    ll.ord_type[(size_t)pos] = L.type;
    ll.ord_local[(size_t)pos] = local;
}
// one more slot at the end of a type's arrays: its index
int grow(HostScene& h, const int type) {
    auto one = [](auto& recs, auto& infos) { recs.resize(recs.size() + 1); infos.resize(recs.size()); return (int)recs.size() - 1; };
    if (type == LEAF_TRI) { h.triuv.resize(h.tri.size() + 1); h.trinrm.resize(h.tri.size() + 1); return one(h.tri, h.ll.tri); }
    return type == LEAF_SPHERE ? one(h.sph, h.ll.sph) : type == LEAF_MSPHERE ? one(h.msph, h.ll.msph)
         : type == LEAF_BEZIER ? one(h.bez, h.ll.bez) : type == LEAF_KLEIN ? one(h.klein, h.ll.klein) : one(h.rect, h.ll.rect);
}

// The tree leaves' records in tree order: tree position i is sphere ns[i] / moving sphere nm[i] / curve
// nb[i] of its type's array (the prefix counts), so the positions fill them independently, on the build's
// threads.  Generic rects follow in tree order.  Returns (generic) each tree position's (type, array index).
Src tree_records(const SceneDesc& s, const Prefix& pre, const bool generic, const int threads, HostScene& h) {
    const std::vector<PrimRef>& refs = h.refs;
    h.sph.resize((size_t)pre.spheres()); h.ll.sph.resize(h.sph.size());
    h.msph.resize((size_t)pre.moving()); h.ll.msph.resize(h.msph.size());
    h.bez.resize((size_t)pre.curves()); h.ll.bez.resize(h.bez.size());
    COMMIT_MARK("resize");
    auto slot = [&](const size_t i) { return refs[i].type == LEAF_SPHERE ? pre.ns[i] : refs[i].type == LEAF_MSPHERE ? pre.nm[i] : pre.nb[i]; };
    parallel_for(refs.size(), threads, [&](const size_t b, const size_t e) {
        for (size_t i = b; i < e; ++i)
            if (!is_appended(refs[i].type)) put_record(s, h.f.leaves[refs[i].leaf], refs[i].leaf, slot(i), h);
    });
    Src src(generic ? refs.size() : 0);
    for (size_t i = 0; i < src.size(); ++i) {
        const bool rect = is_appended(refs[i].type);          // (a rect or a triangle)
        src[i] = {refs[i].type, rect ? grow(h, refs[i].type) : slot(i)};
        if (rect) put_record(s, h.f.leaves[refs[i].leaf], refs[i].leaf, src[i].second, h);
    }
    return src;
}

// Time-0 tree.  Every scattered ray has time 0 (make-ray, ray.scm:8-9, Q4), so for those rays a moving
// sphere sits at center(0) exactly: a second tree over the same leaves bounds each moving sphere at that
// one position instead of over the whole shutter.
// Sphere form (fbvh2, fbleaf, fsph; fsrc = each fsph entry's source): a moving sphere is stored as a plain
// sphere at msphere_center0, so the test the tree runs is bit for bit the moving-sphere test.  Built for
// every sphere tree: with no moving spheres it equals the all-times tree and serves every ray
// (tree0_any_time).
// Generic form (g0bvh2, g0bleaf; gsrc gets the tree's entries appended, its leaves are ranges of those): a
// moving sphere's test at time +0.0 is the all-times one, so only the boxes differ, and there is no tree
// when no sphere moves.
// Returns tree0_direct: every leaf of the sphere form is one sphere, leaf k = fsph[k].
bool time0_tree(const SceneDesc& s, const BuildOptions& opt, const bool generic, const Prefix& pre, const double margin,
                HostScene& h, Src& gsrc, Src& fsrc) {
    const std::vector<PrimRef>& refs = h.refs;
    std::vector<PrimRef> refs0(refs);
    for (size_t i = 0; i < refs0.size(); ++i) {
        PrimRef& r = refs0[i];
        const LeafTmp& L = h.f.leaves[r.leaf];
        r.leaf = (int)i;                             // index into refs (-> gsrc / fsph, fid)
        if (r.type != LEAF_MSPHERE) continue;
        if (generic) {
            int n_ops = 0;
            const ChainOpRec* ops = chain_ops(h.f, L.chain, n_ops);
            double lo[3], hi[3];
            if (!leaf_world_box(leaf_geom(L, s.objs[L.obj]), ops, n_ops, 0.0, 0.0, lo, hi)) continue;   // keeps the all-times box
            for (int k = 0; k < 3; ++k) { r.lo[k] = lo[k]; r.hi[k] = hi[k]; }
        } else {
            const SphereRec S = msphere_center0(h.msph[(size_t)pre.nm[i]]);
            const double c[3] = {S.cx, S.cy, S.cz}, rad = std::sqrt(S.rr) * (1 + 1e-15) + 1e-300;
            const bool fin = std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]);
            for (int k = 0; k < 3; ++k) {
                r.lo[k] = fin ? c[k] - rad : -1e300;
                r.hi[k] = fin ? c[k] + rad : 1e300;
            }
            pad_box(r.lo, r.hi);
        }
        for (int k = 0; k < 3; ++k) r.c[k] = 0.5 * (r.lo[k] + r.hi[k]);
    }
    // (sphere form: direct leaves need one sphere per leaf)
    const std::vector<BvhNode> nodes = sah_build(refs0, opt, !generic && kLeafMax == 1, h.sah_ms);
    DevScene& d = h.d;
    int32_t root = 0;
    if (generic) {
        const int nr = (int)refs.size();
        flatten_bvh2(nodes, margin, [&](int b, int e) { return BvhLeaf{0, 0, 0, 0, 0, 0, nr + b, e - b}; },
                     h.g0bvh2, h.g0bleaf, root, h.tree.depth0);
        d.g0bvh2_root = root;
        d.n_g0bvh2 = (int32_t)h.g0bvh2.size();
        for (const PrimRef& r : refs0) gsrc.push_back(gsrc[(size_t)r.leaf]);
    } else {
        for (const PrimRef& r : refs0) {             // fsph in tree order; each entry remembers its source
            const int local = r.type == LEAF_SPHERE ? pre.ns[(size_t)r.leaf] : pre.nm[(size_t)r.leaf];
            h.fsph.push_back(r.type == LEAF_SPHERE ? h.sph[(size_t)local] : msphere_center0(h.msph[(size_t)local]));
            fsrc.push_back({r.type, local});
        }
        flatten_bvh2(nodes, margin, [&](int b, int e) { return BvhLeaf{b, e - b, 0, 0, 0, 0, 0, 0}; },
                     h.fbvh2, h.fbleaf, root, h.tree.depth0);
    }
    d.lane_stack = std::max(d.lane_stack, h.tree.depth0);
    if (generic) return false;
    // Direct leaves: when every time-0 leaf holds exactly one sphere, put
    // fsph (and its leaf-id map) in leaf order, so leaf k is sphere k and
    // the SOLO LDS kernels need no leaf records (DevScene::bvh_solo).
    const bool direct = std::all_of(h.fbleaf.begin(), h.fbleaf.end(), [](const BvhLeaf& L) { return L.sn == 1; });
    if (direct) {
        std::vector<SphereRec> fs2(h.fbleaf.size());
        Src src2(h.fbleaf.size());
        for (size_t k = 0; k < h.fbleaf.size(); ++k) {
            fs2[k] = h.fsph[(size_t)h.fbleaf[k].sb];
            src2[k] = fsrc[(size_t)h.fbleaf[k].sb];
            h.fbleaf[k].sb = (int32_t)k;
        }
        h.fsph.swap(fs2);
        fsrc.swap(src2);
    }
    if (!h.fbvh2.empty()) {                          // (a tree of one leaf has no node to start at: no time-0 tree)
        d.fbvh2_root = root;
        d.n_fbvh2 = (int)h.fbvh2.size(); d.n_fbleaf = (int)h.fbleaf.size(); d.n_fsph = (int)h.fsph.size();
        d.tree0_any_time = pre.moving() == 0 ? 1 : 0;
    }
    return direct;
}

// Leaves `at` of `src`, those the tree holds aside, grouped by (chain, type) in first-appearance order of
// the chains (-1 first) into `out`, their records appended.  world: src is the flattened list.
void emit_groups(const SceneDesc& s, const std::vector<LeafTmp>& src, const std::vector<int>& at, const bool world,
                 const bool skip_tree, const TreePlan& plan, HostScene& h, std::vector<Group>& out) {
    auto type_size = [&](const int type) {
        return (type == LEAF_SPHERE) ? h.sph.size() : (type == LEAF_MSPHERE) ? h.msph.size()
             : (type == LEAF_BEZIER) ? h.bez.size() : (type == LEAF_KLEIN) ? h.klein.size() : h.rect.size();
    };
    for (int ch = -1; ch < (int)h.f.chains.size(); ++ch) {
        for (int type = LEAF_SPHERE; type <= LEAF_KLEIN; ++type) {
            if (type == LEAF_MEDIUM) continue;
            if (skip_tree && ch == -1 && (type == LEAF_SPHERE || type == LEAF_MSPHERE || type == LEAF_BEZIER)) continue;
            Group g{type, ch, (int)type_size(type), 0};
            for (const int i : at) {
                const LeafTmp& L = src[(size_t)i];
                if (L.chain != ch || L.type != type) continue;
                if (world && plan.gen((size_t)i)) continue;               // in the tree
                put_record(s, L, world ? i : -1, grow(h, type), h);
            }
            g.end = (int)type_size(type);
            if (g.end > g.begin) out.push_back(g);
        }
    }
}

// Segment sg: the groups of its leaves, then its medium with the medium's boundary groups.  listed: the
// medium gets a list position of its own (media forests: DevScene::order holds it)
void segment_one(const SceneDesc& s, const std::vector<int>& seg, const int sg, const bool skip_tree, const bool listed,
                 const TreePlan& plan, HostScene& h) {
    const Flattener& f = h.f;
    std::vector<int> ls;
    const LeafTmp* medium = nullptr;
    for (size_t i = 0; i < f.leaves.size(); ++i) {
        if (seg[i] != sg) continue;
        if (f.leaves[i].type == LEAF_MEDIUM) medium = &f.leaves[i];
        else ls.push_back((int)i);
    }
    emit_groups(s, f.leaves, ls, true, skip_tree, plan, h, h.groups);
    COMMIT_MARK("emit");
    if (!medium) return;
    const Obj& o = s.objs[medium->obj];
    const std::vector<LeafTmp>& bound = f.bounds[medium->aux];
    std::vector<int> all(bound.size());
    for (size_t k = 0; k < all.size(); ++k) all[k] = (int)k;
    MediumRec m{};
    m.bg_begin = (int)h.bgroups.size();
    emit_groups(s, bound, all, false, false, plan, h, h.bgroups);
    m.bg_end = (int)h.bgroups.size();
    m.neg_inv_density = -(1 / o.r);             // (- (/ 1 density)), geometry.scm:564
    LeafInfo li = leaf_info(*medium, o);
    li.local = (int)h.med.size();
    if (listed) {
        const size_t pos = (size_t)(medium - f.leaves.data());
        h.ll.ord_type[pos] = LEAF_MEDIUM;
        h.ll.ord_local[pos] = li.local;
    }
    h.groups.push_back(Group{LEAF_MEDIUM, medium->chain, (int)h.med.size(), (int)h.med.size() + 1});
    h.med.push_back(m);
    h.ll.med.push_back(li);
}
void segment_records(const SceneDesc& s, const std::vector<int>& seg, const int nseg, const bool use_tree,
                     const TreePlan& plan, HostScene& h) {
    for (int sg = 0; sg < nseg; ++sg) segment_one(s, seg, sg, use_tree && sg == 0, false, plan, h);
}

// A media forest's trees and records, segment by segment: [its tree] [its groups] [its medium].  Every tree is
// appended to bvh2 / bleaf (flatten_bvh2's refs are absolute) with its leaves as ranges of gleaf, a time-0
// twin of a tree that holds a moving sphere to g0bvh2 / g0bleaf; the tree's GROUP_BVH group carries the
// roots (Group::begin, end).  h.refs: all trees' leaves, tree after tree.
void forest_records(const SceneDesc& s, const BuildOptions& opt, const std::vector<int>& seg, const int nseg,
                    const ForestPlan& fp, HostScene& h, Src& gsrc) {
    const Flattener& f = h.f;
    DevScene& d = h.d;
    const double tlo = std::min(std::min(s.cam[22], s.cam[23]), 0.0), thi = std::max(std::max(s.cam[22], s.cam[23]), 0.0);
    const double margin = std::ldexp(scene_radius(s, f, opt.threads), -21);     // (world_tree: the f32 box margin)
    d.bvh_pad = (float)margin;
    h.threads = opt.threads;
    h.tree.segments = nseg;
    bool first = true;
    for (int sg = 0; sg < nseg; ++sg) {
        const std::vector<int>& in = fp.tree[(size_t)sg];
        if (!in.empty()) {
            std::vector<PrimRef> refs(in.size());
            for (size_t j = 0; j < in.size(); ++j) {
                const size_t i = (size_t)in[j];
                const LeafTmp& L = f.leaves[i];
                if (!world_sphere(L)) { refs[j] = fp.leaves.gen_ref[i]; continue; }
                PrimRef r{};                                  // (prim_boxes: a world-level sphere's box)
                r.leaf = (int)i;
                r.type = L.type;
                leaf_local_box(leaf_geom(L, s.objs[L.obj]), tlo, thi, r.lo, r.hi);
                pad_box(r.lo, r.hi);
                for (int k = 0; k < 3; ++k) r.c[k] = 0.5 * (r.lo[k] + r.hi[k]);
                refs[j] = r;
            }
            const std::vector<BvhNode> nodes = sah_build(refs, opt, false, h.sah_ms);
            const int g0 = (int)gsrc.size();
            int32_t root = 0, root0 = kNoTwin;
            flatten_bvh2(nodes, margin, [&](int b, int e) { return BvhLeaf{0, 0, 0, 0, 0, 0, g0 + b, e - b}; },
                         h.bvh2, h.bleaf, root, h.tree.depth, opt.threads);
            bool moving = false;
            for (const PrimRef& r : refs) {
                const int local = grow(h, r.type);
                put_record(s, f.leaves[(size_t)r.leaf], r.leaf, local, h);
                gsrc.push_back({r.type, local});
                moving = moving || r.type == LEAF_MSPHERE;
            }
            if (moving && !opt.no_bvh0) {                    // (time0_tree, generic form)
                std::vector<PrimRef> refs0(refs);
                for (size_t j = 0; j < refs0.size(); ++j) {
                    PrimRef& r = refs0[j];
                    const LeafTmp& L = f.leaves[(size_t)r.leaf];
                    r.leaf = (int)j;                          // index into refs (-> gsrc)
                    if (r.type != LEAF_MSPHERE) continue;
                    int n_ops = 0;
                    const ChainOpRec* ops = chain_ops(f, L.chain, n_ops);
                    double lo[3], hi[3];
                    if (!leaf_world_box(leaf_geom(L, s.objs[L.obj]), ops, n_ops, 0.0, 0.0, lo, hi)) continue;
                    for (int k = 0; k < 3; ++k) { r.lo[k] = lo[k]; r.hi[k] = hi[k]; r.c[k] = 0.5 * (lo[k] + hi[k]); }
                }
                const std::vector<BvhNode> nodes0 = sah_build(refs0, opt, false, h.sah_ms);
                const int g1 = (int)gsrc.size();
                flatten_bvh2(nodes0, margin, [&](int b, int e) { return BvhLeaf{0, 0, 0, 0, 0, 0, g1 + b, e - b}; },
                             h.g0bvh2, h.g0bleaf, root0, h.tree.depth0);
                for (const PrimRef& r : refs0) gsrc.push_back(gsrc[(size_t)(g0 + r.leaf)]);
                if (d.n_g0bvh2 == 0) d.g0bvh2_root = root0;
                d.n_g0bvh2 = (int32_t)h.g0bvh2.size();
            }
            if (first) d.bvh2_root = root;
            first = false;
            h.groups.push_back(Group{GROUP_BVH, -1, root, root0});
            h.refs.insert(h.refs.end(), refs.begin(), refs.end());
            ++h.tree.segment_trees;
        }
        segment_one(s, seg, sg, false, true, fp.leaves, h);
    }
    d.lane_stack = std::max(h.tree.depth, h.tree.depth0);
    COMMIT_MARK("forest");
}

// Leaf ids: spheres, moving spheres, then all rects (the three axis types share the rect array: leaf id =
// rect base + local), curves, media, Klein sets, triangles; h.leaves in that order
int assign_leaf_ids(const int threads, HostScene& h, std::string& err) {
    const LeafLists& ll = h.ll;
    if (ll.sph.size() != h.sph.size() || ll.msph.size() != h.msph.size() || ll.bez.size() != h.bez.size() ||
        ll.klein.size() != h.klein.size() || ll.rect.size() != h.rect.size() || ll.tri.size() != h.tri.size() ||
        h.triuv.size() != h.tri.size() || h.trinrm.size() != h.tri.size())
        return fail_with(&err, "internal: leaf records and leaf infos out of step");
    int32_t* base = h.d.leaf_base;
    base[LEAF_SPHERE] = 0;
    base[LEAF_MSPHERE] = base[LEAF_SPHERE] + (int32_t)ll.sph.size();
    base[LEAF_RECT_XY] = base[LEAF_RECT_XZ] = base[LEAF_RECT_YZ] = base[LEAF_MSPHERE] + (int32_t)ll.msph.size();
    base[LEAF_BEZIER] = base[LEAF_RECT_XY] + (int32_t)ll.rect.size();
    base[LEAF_MEDIUM] = base[LEAF_BEZIER] + (int32_t)ll.bez.size();
    base[LEAF_KLEIN] = base[LEAF_MEDIUM] + (int32_t)ll.med.size();
    const int32_t tri_base = base[LEAF_KLEIN] + (int32_t)ll.klein.size();
    base[LEAF_TRI] = ll.tri.empty() ? 0 : tri_base;          // (a scene without triangles keeps the word 0, as memset left it)
    h.leaves.resize((size_t)tri_base + ll.tri.size());
    auto put = [&](const LeafInfo* src, const size_t n, const int32_t at) {
        parallel_for(n, threads, [&](const size_t b, const size_t e) { std::copy(src + b, src + e, h.leaves.data() + at + b); });
    };
    put(ll.sph.data(), ll.sph.size(), base[LEAF_SPHERE]);
    put(ll.msph.data(), ll.msph.size(), base[LEAF_MSPHERE]);
    put(ll.rect.data(), ll.rect.size(), base[LEAF_RECT_XY]);
    put(ll.bez.data(), ll.bez.size(), base[LEAF_BEZIER]);
    put(ll.med.data(), ll.med.size(), base[LEAF_MEDIUM]);
    put(ll.klein.data(), ll.klein.size(), base[LEAF_KLEIN]);
    put(ll.tri.data(), ll.tri.size(), tri_base);
    return 0;
}

// the shade-side fields: material, texture shortcut, sphere centre (LeafInfo); and the leaves' classes
void shade_fields(const SceneDesc& s, const int threads, HostScene& h) {
    parallel_for(h.leaves.size(), threads, [&](const size_t lb, const size_t le) {
      for (size_t lk = lb; lk < le; ++lk) {
        LeafInfo& li = h.leaves[lk];
        if (li.mat < 0 || li.mat >= (int)s.mats.size()) continue;     // boundary placeholders
        const DevMaterial& m = s.mats[li.mat];
        li.mtype = m.type;
        li.tex = m.tex;
        li.mparam = (m.type == MAT_METAL) ? m.fuzz : m.ref_idx;
        li.tex_kind = TK_GENERIC;
        auto constant = [&](int t) { return t >= 0 && t < (int)s.texs.size() && s.texs[t].type == TEX_CONSTANT; };
        if (constant(m.tex)) {
            const DevTexture& T = s.texs[m.tex];
            li.tex_kind = TK_CONSTANT;
            li.albedo[0] = T.r; li.albedo[1] = T.g; li.albedo[2] = T.bl;
        } else if (m.tex >= 0 && m.tex < (int)s.texs.size() && s.texs[m.tex].type == TEX_CHECKER &&
                   constant(s.texs[m.tex].a) && constant(s.texs[m.tex].b)) {
            const DevTexture& E = s.texs[s.texs[m.tex].a];       // even (texture.scm:20-23)
            const DevTexture& O = s.texs[s.texs[m.tex].b];       // odd
            li.tex_kind = TK_CHECKER_CONST;
            li.albedo[0] = E.r; li.albedo[1] = E.g; li.albedo[2] = E.bl;
            li.albedo2[0] = O.r; li.albedo2[1] = O.g; li.albedo2[2] = O.bl;
        }
        if (li.type == LEAF_SPHERE || li.type == LEAF_MSPHERE) {  // a moving sphere's centre: at time 0
            const SphereRec S = li.type == LEAF_SPHERE ? h.sph[(size_t)li.local] : msphere_center0(h.msph[(size_t)li.local]);
            li.c[0] = S.cx; li.c[1] = S.cy; li.c[2] = S.cz;
        }
      }
    });
    h.chains.clear();
    for (const auto& cv : h.f.chains) {
        Chain c{};
        c.n = (int)cv.size();
        for (size_t k = 0; k < cv.size(); ++k) c.ops[k] = cv[k];
        h.chains.push_back(c);
    }
    h.leaf_cls.assign((h.leaves.size() + 15) / 16 * 16 + 16, 0);
    for (size_t k = 0; k < h.leaves.size(); ++k) h.leaf_cls[k] = (uint8_t)h.leaves[k].mtype;
}

// The world's leaf ids in list order (list_closest; none for scenes with media, which keep the grouped
// scan, unless they are media forests: then the whole list, media included); the leaf ids of the tree entries (fid: of fsph's, gleaf: of the generic tree's) and every leaf's
// list position
int list_order(const bool generic, const Src& fsrc, const Src& gsrc, HostScene& h, std::string& err) {
    const int32_t* base = h.d.leaf_base;
    const LeafLists& ll = h.ll;
    if (!h.fbvh2.empty())
        for (const auto& sl : fsrc) h.fid.push_back(base[sl.first] + sl.second);
    if (h.med.empty() || h.forest) {
        h.order.reserve(h.f.leaves.size());
        for (size_t i = 0; i < h.f.leaves.size(); ++i)
            if (ll.ord_type[i] >= 0) h.order.push_back(base[ll.ord_type[i]] + ll.ord_local[i]);
        // (a forest's media have boundary leaves, which are records outside the list)
        if (h.order.size() != (h.forest ? h.f.leaves.size() : h.leaves.size()))
            return fail_with(&err, "internal: list order and leaf records out of step");
    }
    h.d.n_order = (int32_t)h.order.size();
    if (!generic) return 0;
    h.gleaf.reserve(gsrc.size());
    for (const auto& tl : gsrc) h.gleaf.push_back(base[tl.first] + tl.second);
    h.leaf_pos.assign(h.leaves.size(), 0);
    for (size_t k = 0; k < h.order.size(); ++k) h.leaf_pos[(size_t)h.order[k]] = (int32_t)k;
    h.d.n_gleaf = (int32_t)h.gleaf.size();
    h.d.n_rot = (int32_t)h.rot.size();
    return 0;
}

// rt_get_tree_info's record (nodes, depths: as the trees were built)
void tree_info(const BuildOptions& opt, const bool use_tree, const bool generic, HostScene& h) {
    rt_tree_info& ti = h.tree;
    if (use_tree) {
        for (const PrimRef& r : h.refs) {
            if (r.type == LEAF_BEZIER) ++ti.curve_leaves;
            else if (r.type == LEAF_TRI) ++ti.tri_leaves;
            else if (world_sphere(h.f.leaves[(size_t)r.leaf])) ++ti.sphere_leaves;
            else ++ti.generic_leaves;
        }
        ti.nodes = (int32_t)h.bvh2.size();
        ti.nodes0 = (int32_t)(generic ? h.g0bvh2.size() : h.fbvh2.size());
    }
    ti.group_leaves = (int32_t)h.leaves.size() - ti.sphere_leaves - ti.curve_leaves - ti.generic_leaves - ti.tri_leaves;
    ti.rot_entries = (int32_t)h.rot.size();
    ti.generic_min = (int32_t)opt.generic_min;
}

// rt_set_light_sampling's target as DevLight (a rect or a sphere, flips looked through)
void single_light(const Obj& L, DevLight& dl) {
    if (L.type == O_RECT) {
        dl.type = LIGHT_RECT; dl.axis = L.axis;
        dl.a0 = L.a0; dl.a1 = L.a1; dl.b0 = L.b0; dl.b1 = L.b1; dl.k = L.k;
    } else {
        dl.type = LIGHT_SPHERE;
        dl.cx = L.c0[0]; dl.cy = L.c0[1]; dl.cz = L.c0[2]; dl.r = L.r;
    }
}
// The light list's records (include/rt.h, "light lists"), from its flattened ids.  One rect or sphere is the
// single light: d.light as rt_set_light_sampling fills it, no record.
void light_records(const SceneDesc& s, const std::vector<int>& ids, HostScene& h) {
    if (ids.size() == 1 && s.objs[ids[0]].type != O_TRI) { single_light(s.objs[ids[0]], h.d.light); return; }
    h.d.light.type = LIGHT_LIST;
    h.lights.reserve(ids.size());
    for (const int id : ids) {
        const Obj& o = s.objs[id];
        DevLightRec r{};
        if (o.type == O_RECT) {
            r.type = LIGHT_RECT; r.axis = o.axis;
            r.t.v0[0] = o.a0; r.t.v0[1] = o.a1; r.t.v0[2] = o.b0; r.t.v1[0] = o.b1; r.t.v1[1] = o.k;
        } else if (o.type == O_SPHERE) {
            r.type = LIGHT_SPHERE;
            for (int k = 0; k < 3; ++k) r.t.v0[k] = o.c0[k];
            r.t.v1[0] = o.r;
        } else {
            r.type = LIGHT_TRI;
            h.d.lights_tri = 1;
            r.t = tri_rec(o);
            const double* v0 = o.cp, *v1 = o.cp + 3, *v2 = o.cp + 6;
            const double e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
            const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            r.t.pad0 = 0.5 * std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);    // area
            (void)tri_normal(v0, v1, v2, r.nu);
        }
        h.lights.push_back(r);
    }
    h.d.n_lights = (int32_t)h.lights.size();
}

// the counts and scene-wide flags of DevScene, the light and the camera
void scene_fields(const SceneDesc& s, const BuildOptions& opt, const bool tree0_direct, const std::vector<int>& lights,
                  HostScene& h) {
    DevScene& d = h.d;
    d.n_sph = (int)h.sph.size(); d.n_msph = (int)h.msph.size(); d.n_rect = (int)h.rect.size();
    d.n_bez = (int)h.bez.size(); d.n_klein = (int)h.klein.size(); d.n_med = (int)h.med.size();
    d.n_tri = (int)h.tri.size();
    for (const TriNrm& q : h.trinrm) if (q.has) { d.tri_smooth = 1; break; }
    d.n_groups = (int)h.groups.size(); d.n_bgroups = (int)h.bgroups.size();
    d.n_chains = (int)h.chains.size(); d.n_leaves = (int)h.leaves.size();
    d.n_bvh2 = (int)h.bvh2.size(); d.n_bleaf = (int)h.bleaf.size();
    for (const Group& G : h.groups) d.bez_groups += G.type == LEAF_BEZIER ? 1 : 0;
    if (!h.msph.empty()) {
        bool same = true;
        for (const MSphereRec& m : h.msph)
            same = same && std::memcmp(&m.t0, &h.msph[0].t0, sizeof(double)) == 0 &&
                   std::memcmp(&m.den, &h.msph[0].den, sizeof(double)) == 0;
        if (same) { d.msph_shared = 1; d.msph_t0 = h.msph[0].t0; d.msph_den = h.msph[0].den; }
    }
    d.bvh_solo = (h.groups.size() == 1 && h.groups[0].type == GROUP_BVH && !d.bvh_has_bez && tree0_direct &&
                  !opt.no_solo) ? 1 : 0;
    d.n_mats = (int)s.mats.size(); d.n_texs = (int)s.texs.size();
    d.has_perlin = s.have_perlin ? 1 : 0;
    for (const auto& t : s.texs) {
        if (t.type == TEX_NOISE || t.type == TEX_MARBLE) d.has_noise_tex = 1;
        if (t.type == TEX_IMAGE) d.has_image_tex = 1;
    }
    d.sky = s.sky;
    if (!lights.empty()) {
        light_records(s, lights, h);
    } else if (s.light >= 0) {
        const Obj* L = &s.objs[s.light];
        while (L->type == O_FLIP) L = &s.objs[L->child];
        single_light(*L, d.light);
    }
    for (const auto& m : s.mats) d.mat_mask |= 1 << m.type;
    static_assert(sizeof d.cam == sizeof s.cam, "rt_make_camera's doubles are DevCamera's members, in order");
    std::memcpy(&d.cam, s.cam, sizeof d.cam);
}
}  // namespace

// ------------------------------------------------------------ flattening
int Flattener::chain_id() {
    if (cur.empty()) return -1;
    for (size_t i = 0; i < chains.size(); ++i) {
        if (chains[i].size() == cur.size() &&
            std::memcmp(chains[i].data(), cur.data(), cur.size() * sizeof(ChainOpRec)) == 0)
            return (int)i;
    }
    chains.push_back(cur);
    return (int)chains.size() - 1;
}

int Flattener::walk(int id, int flip) {
    if (++depth_guard > 10000) return fail_with(err, "object graph too deep (cycle?)");
    const Obj& o = s->objs[id];
    int rc = 0;
    switch (o.type) {
    case O_SPHERE: leaves.push_back({LEAF_SPHERE, chain_id(), flip, id}); break;
    case O_MSPHERE: leaves.push_back({LEAF_MSPHERE, chain_id(), flip, id}); break;
    case O_RECT: leaves.push_back({LEAF_RECT_XY + o.axis, chain_id(), flip, id}); break;
    case O_TRI:
        if (in_boundary) return fail_with(err, "a triangle cannot be (part of) a constant medium's boundary");
        leaves.push_back({LEAF_TRI, chain_id(), flip, id});
        break;
    case O_BEZIER: case O_KLEIN:
        if (in_boundary) return fail_with(err, "a constant medium's boundary may hold spheres, rects, boxes and instances only");
        leaves.push_back({o.type == O_BEZIER ? LEAF_BEZIER : LEAF_KLEIN, chain_id(), flip, id});
        break;
    case O_MEDIUM: {
        if (in_boundary) return fail_with(err, "constant media cannot be nested");
        std::vector<LeafTmp> saved;
        saved.swap(leaves);
        in_boundary = true;
        rc = walk(o.child, 0);
        in_boundary = false;
        std::vector<LeafTmp> b;
        b.swap(leaves);
        leaves.swap(saved);
        if (rc) break;
        bounds.push_back(std::move(b));
        LeafTmp L{LEAF_MEDIUM, chain_id(), flip, id};
        L.aux = (int)bounds.size() - 1;
        leaves.push_back(L);
        break;
    }
    case O_FLIP: rc = walk(o.child, flip ^ 1); break;
    case O_BOX:
    case O_LIST:
    case O_BVH:
        for (int k : o.kids) { if ((rc = walk(k, flip))) break; }
        break;
    case O_TRANSLATE:
    case O_ROTATE_Y: {
        if ((int)cur.size() >= kMaxChain) return fail_with(err, "instance nesting deeper than 4 transforms");
        ChainOpRec op{};
        if (o.type == O_TRANSLATE) { op.op = OP_TRANSLATE; op.x = o.c0[0]; op.y = o.c0[1]; op.z = o.c0[2]; }
        else { op.op = OP_ROTATE_Y; op.x = o.sin_t; op.y = o.cos_t; op.z = 0; }
        cur.push_back(op);
        rc = walk(o.child, flip);
        cur.pop_back();
        break;
    }
    }
    --depth_guard;
    return rc;
}

int flatten_lights(const SceneDesc& s, const int* objs, const int n, std::vector<int>& out, std::string& err) {
    out.clear();
    if (n < 0) return fail_with(&err, "rt_set_light_list: n must be >= 0");
    if (n > 0 && !objs) return fail_with(&err, "rt_set_light_list: null object list");
    // depth-first, in order, without recursion (a list may nest to any depth); an object listed twice is two lights
    std::vector<std::pair<int, int>> stack;          // (object, the next kid to open)
    for (int k = 0; k < n; ++k) {
        stack.push_back({objs[k], 0});
        size_t flips = 0;                            // consecutive flips looked through
        while (!stack.empty()) {
            const int id = stack.back().first;
            if (id < 0 || id >= (int)s.objs.size()) {
                err = "rt_set_light_list: invalid object id " + std::to_string(id);
                return 1;
            }
            const Obj& o = s.objs[id];
            if (o.type == O_LIST) {
                const int kid = stack.back().second++;
                if (kid >= (int)o.kids.size()) { stack.pop_back(); continue; }
                if (stack.size() > s.objs.size()) return fail_with(&err, "rt_set_light_list: object graph too deep (cycle?)");
                stack.push_back({o.kids[kid], 0});
                continue;
            }
            stack.pop_back();
            if (o.type == O_FLIP) {                              // a flip does not change sampling
                // (a chain of flips longer than the scene has objects: a cycle in a description filled directly)
                if (++flips > s.objs.size()) return fail_with(&err, "rt_set_light_list: object graph too deep (cycle?)");
                stack.push_back({o.child, 0});
                continue;
            }
            flips = 0;
            if (o.type != O_RECT && o.type != O_SPHERE && o.type != O_TRI)
                return fail_with(&err, "rt_set_light_list: a light must be a rect, a sphere or a triangle (optionally "
                                       "flipped), or a list or mesh of such");
            if ((int)out.size() >= RT_MAX_LIGHTS) {
                err = "rt_set_light_list: more than RT_MAX_LIGHTS (" + std::to_string(RT_MAX_LIGHTS) + ") lights";
                return 1;
            }
            out.push_back(id);
        }
    }
    if (n > 0 && out.empty()) return fail_with(&err, "rt_set_light_list: the list holds no light");
    return 0;
}

BuildOptions BuildOptions::from_env() {
    BuildOptions o;
    if (const char* e = std::getenv("RTAMD_BVH_MIN")) o.bvh_min = (size_t)std::strtoull(e, nullptr, 10);
    if (const char* e = std::getenv("RTAMD_BVH_GENERIC_MIN")) o.generic_min = (size_t)std::strtoull(e, nullptr, 10);
    o.generic_min = std::min<size_t>(std::max<size_t>(o.generic_min, 1), (size_t)1 << 30);
    if (const char* e = std::getenv("RTAMD_BVH_SWEEP")) o.sweep_max = std::atoi(e);
    o.no_bvh0 = std::getenv("RTAMD_NO_BVH0") != nullptr;
    o.no_solo = std::getenv("RTAMD_NO_SOLO") != nullptr;
    o.threads = build_threads();
    return o;
}

int build_scene(const SceneDesc& s, const int world, const BuildOptions& opt, HostScene& h, std::string& err) {
    std::memset(&h.d, 0, sizeof h.d);                // (its padding too: the device copy is the whole struct)
    if (!s.have_cam) return fail_with(&err, "rt_scene_commit: no camera set (rt_set_camera)");
    for (const auto& t : s.texs)
        if ((t.type == TEX_NOISE || t.type == TEX_MARBLE) && !s.have_perlin)
            return fail_with(&err, "rt_scene_commit: noise/marble texture needs rt_set_perlin_tables");
    Flattener& f = h.f;
    f.s = &s;
    f.err = &err;
    f.leaves.reserve(s.objs.size());                 // (a hint: an object listed twice is two leaves)
    if (int rc = f.walk(world, 0)) return rc;
    const bool tri = has_triangle(f);
    if (tri) {                                       // (include/rt.h, "triangles": what a triangle scene may hold)
        for (const LeafTmp& L : f.leaves)
            if (L.type == LEAF_BEZIER || L.type == LEAF_KLEIN || L.type == LEAF_MEDIUM)
                return fail_with(&err, "rt_scene_commit: a scene with triangles cannot hold a curve, a Klein set or a constant medium");
    }
    if (s.light >= 0) {
        const Obj* L = &s.objs[s.light];
        while (L->type == O_FLIP) L = &s.objs[L->child];
        if (L->type == O_TRI) return fail_with(&err, "rt_scene_commit: a triangle cannot be the light-sampling target");
    }
    std::vector<int> lights;                         // the light list, flattened (rt_set_light_list checked it; a
    if (!s.lights.empty())                           // SceneDesc filled directly is checked here)
        if (flatten_lights(s, s.lights.data(), (int)s.lights.size(), lights, err)) return 1;
    std::vector<int> seg;
    const int nseg = cut_segments(f, seg);
    COMMIT_MARK("flatten");
    const ForestPlan forest = choose_forest(s, f, seg, nseg, opt, h.rot);
    h.forest = forest.on;
    const TreePlan plan = forest.on ? forest.leaves : choose_tree_leaves(s, f, seg, nseg, opt, h.rot);
    h.generic = plan.generic;
    if (tri)                                         // every triangle is a leaf of the tree: no group tests one
        for (size_t i = 0; i < f.leaves.size(); ++i)
            if (f.leaves[i].type == LEAF_TRI && !plan.gen(i))
                return fail_with(&err, "rt_scene_commit: a triangle's world-space box is not finite (its instance chain?)");
    if (!forest.on) h.refs = prim_boxes(s, f, plan, opt.threads);
    COMMIT_MARK("refs");
    h.ll.ord_type.assign(f.leaves.size(), -1);
    h.ll.ord_local.assign(f.leaves.size(), -1);
    const bool use_tree = forest.on || (!h.refs.empty() && (tri || h.refs.size() >= opt.bvh_min));
    bool tree0_direct = false;
    Src gsrc, fsrc;
    if (forest.on) {
        forest_records(s, opt, seg, nseg, forest, h, gsrc);
    } else if (use_tree) {
        Prefix pre;
        const double margin = world_tree(s, opt, plan.generic, h, pre);
        gsrc = tree_records(s, pre, plan.generic, opt.threads, h);
        if (!opt.no_bvh0 && !h.d.bvh_has_bez && (!plan.generic || pre.moving() > 0))
            tree0_direct = time0_tree(s, opt, plan.generic, pre, margin, h, gsrc, fsrc);
    }
    COMMIT_MARK("records");
    if (!forest.on) segment_records(s, seg, nseg, use_tree, plan, h);
    if (int rc = assign_leaf_ids(opt.threads, h, err)) return rc;
    COMMIT_MARK("leaves");
    shade_fields(s, opt.threads, h);
    COMMIT_MARK("groups");
    if (h.d.lane_stack > kLaneStack) return fail_with(&err, "internal: BVH deeper than the traversal stack");
    if (int rc = list_order(plan.generic, fsrc, gsrc, h, err)) return rc;
    tree_info(opt, use_tree, plan.generic, h);
    scene_fields(s, opt, tree0_direct, lights, h);
    for (const Obj& o : s.objs)
        if (o.mat >= (int)s.mats.size()) return fail_with(&err, "object refers to an unknown material");
    return 0;
}

}  // namespace rtamd
