// tri_check.cpp — build_scene (rt_build.cpp) on scenes with triangles, filled directly into a SceneDesc: a
// height-field mesh under no chain, under translate, and under rotate-y + translate, among spheres and rects.
// Checks that every triangle's vertices, taken out of its chain, lie in its tree leaf's box; that every entry
// of gleaf is reached from the root exactly once and every triangle's leaf id is among them once; that
// rt_tree_info.tri_leaves and the record counts are right; that the 1-thread, the 8-thread and a repeated
// build give the same arrays; that a scene of one triangle gets a tree (a root that is a leaf); that the
// normals kept in LeafInfo are tri_normal's; and that the commit refuses what include/rt.h says it refuses.
// Host code with its own main (no GPU), compiled with g++ beside rt_build.cpp, under ASan / UBSan.
// Prints one JSON object.  usage: tri_check [N_PER_SIDE]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../scheme-raytrace_amd/csrc/rt_build.h"
#include "../../scheme-raytrace_amd/csrc/rt_leafbox.h"

using namespace rtamd;

namespace {
struct Rand {                                        // splitmix64 -> [0, 1)
    uint64_t s;
    double operator()() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (double)((z ^ (z >> 31)) >> 11) * 0x1p-53;
    }
};

struct Builder {
    SceneDesc s;
    Builder() {
        s.have_cam = true;
        s.cam[9] = 0; s.cam[10] = 1; s.cam[11] = 8;
        s.cam[22] = 0.0; s.cam[23] = 1.0;
        DevTexture t{}; t.type = TEX_CONSTANT; t.r = 0.5; t.g = 0.25; t.bl = 0.125;
        s.texs.push_back(t);
        for (int m = 0; m < 3; ++m) { DevMaterial M{}; M.type = m; M.tex = 0; M.fuzz = 0.1; M.ref_idx = 1.5; s.mats.push_back(M); }
    }
    int add(Obj o) { s.objs.push_back(std::move(o)); return (int)s.objs.size() - 1; }
    int sphere(double x, double y, double z, double r) { Obj o; o.type = O_SPHERE; o.mat = 0; o.c0[0] = x; o.c0[1] = y; o.c0[2] = z; o.r = r; return add(o); }
    int rect(int axis, double a0, double a1, double b0, double b1, double k) {
        Obj o; o.type = O_RECT; o.axis = axis; o.mat = 0; o.a0 = a0; o.a1 = a1; o.b0 = b0; o.b1 = b1; o.k = k; return add(o);
    }
    int tri(const double* a, const double* b, const double* c) {
        Obj o; o.type = O_TRI; o.mat = 1;
        for (int k = 0; k < 3; ++k) { o.cp[k] = a[k]; o.cp[3 + k] = b[k]; o.cp[6 + k] = c[k]; }
        return add(o);
    }
    int unary(ObjType t, int child) { Obj o; o.type = t; o.child = child; o.mat = s.objs[child].mat; return add(o); }
    int translate(int child, double x, double y, double z) {
        const int id = unary(O_TRANSLATE, child);
        s.objs[id].c0[0] = x; s.objs[id].c0[1] = y; s.objs[id].c0[2] = z; return id;
    }
    int rotate_y(int child, double deg) {
        const int id = unary(O_ROTATE_Y, child);
        s.objs[id].sin_t = std::sin(deg * kPi / 180); s.objs[id].cos_t = std::cos(deg * kPi / 180); return id;
    }
    int list(std::vector<int> kids) { Obj o; o.type = O_LIST; o.kids = std::move(kids); return add(o); }
    int bezier() { Obj o; o.type = O_BEZIER; o.mat = 0; o.width = 0.1; for (int k = 0; k < 12; ++k) o.cp[k] = 0.1 * k; return add(o); }
    int klein() { Obj o; o.type = O_KLEIN; o.mat = 0; return add(o); }
    int medium(int child) {
        DevMaterial M{}; M.type = MAT_LAMBERTIAN; M.tex = 0; s.mats.push_back(M);
        Obj o; o.type = O_MEDIUM; o.child = child; o.r = 0.5; o.mat = (int)s.mats.size() - 1; return add(o);
    }
    // a side x side height field over [0, 1]^2 (2 side^2 triangles) as one list, the grid's vertices shared
    int field(int side, Rand& rr) {
        std::vector<double> h((size_t)(side + 1) * (side + 1));
        for (double& x : h) x = 0.2 * rr();
        auto vtx = [&](int i, int j, double* p) { p[0] = (double)i / side; p[1] = h[(size_t)i * (side + 1) + j]; p[2] = (double)j / side; };
        std::vector<int> kids;
        for (int i = 0; i < side; ++i)
            for (int j = 0; j < side; ++j) {
                double a[3], b[3], c[3], d[3];
                vtx(i, j, a); vtx(i + 1, j, b); vtx(i + 1, j + 1, c); vtx(i, j + 1, d);
                kids.push_back(tri(a, c, b));
                kids.push_back(tri(a, d, c));
            }
        return list(kids);
    }
};

uint64_t fnv(uint64_t x, const void* p, size_t n) {
    for (size_t k = 0; k < n; ++k) x = (x ^ static_cast<const uint8_t*>(p)[k]) * 1099511628211ull;
    return x;
}
template <class V> uint64_t fnv_vec(uint64_t x, const V& v) { return v.empty() ? x : fnv(x, v.data(), v.size() * sizeof(v[0])); }
uint64_t digest(const HostScene& h) {
    uint64_t x = 1469598103934665603ull;
    x = fnv_vec(x, h.tri); x = fnv_vec(x, h.sph); x = fnv_vec(x, h.rect); x = fnv_vec(x, h.bvh2); x = fnv_vec(x, h.bleaf);
    x = fnv_vec(x, h.gleaf); x = fnv_vec(x, h.leaf_pos); x = fnv_vec(x, h.order); x = fnv_vec(x, h.leaves); x = fnv_vec(x, h.groups);
    for (const TriUv& q : h.triuv) { x = fnv(x, q.u, sizeof q.u); x = fnv(x, q.v, sizeof q.v); x = fnv(x, &q.has, sizeof q.has); }
    x = fnv(x, &h.d.bvh2_root, sizeof h.d.bvh2_root);
    x = fnv(x, h.d.leaf_base, sizeof h.d.leaf_base);
    return x;
}

struct Result { long outside = 0, reach_bad = 0, tri_ids_bad = 0, normals_bad = 0; int tri_leaves = 0, n_tri = 0, tris = 0, n_gleaf = 0; bool ok = false; std::string err; uint64_t dig = 0; };

Result run(const SceneDesc& s, int world, int threads) {
    Result r;
    HostScene h;
    BuildOptions opt;
    opt.threads = threads;
    if (build_scene(s, world, opt, h, r.err)) return r;
    r.ok = true;
    r.dig = digest(h);
    r.tri_leaves = h.tree.tri_leaves;
    r.n_tri = h.d.n_tri;
    r.n_gleaf = h.d.n_gleaf;
    for (const LeafTmp& L : h.f.leaves) r.tris += L.type == LEAF_TRI ? 1 : 0;
    // every triangle's vertices, out of its chain, in its tree leaf's box
    for (const PrimRef& p : h.refs) {
        if (p.type != LEAF_TRI) continue;
        const LeafTmp& L = h.f.leaves[(size_t)p.leaf];
        const Obj& o = s.objs[(size_t)L.obj];
        for (int i = 0; i < 3; ++i) {
            double q[3] = {o.cp[3 * i], o.cp[3 * i + 1], o.cp[3 * i + 2]};
            if (L.chain >= 0) chain_point(h.f.chains[(size_t)L.chain].data(), (int)h.f.chains[(size_t)L.chain].size(), q);
            for (int k = 0; k < 3; ++k)
                if (!(q[k] >= p.lo[k] && q[k] <= p.hi[k])) { ++r.outside; break; }
        }
    }
    // every gleaf entry reached from the root exactly once
    std::vector<int> seen(h.gleaf.size(), 0);
    std::vector<int32_t> stack{h.d.bvh2_root};
    size_t steps = 0;
    while (!stack.empty() && ++steps < 10 * (h.bvh2.size() + h.bleaf.size() + 2)) {
        const int32_t ref = stack.back();
        stack.pop_back();
        if (ref >= 0) {
            if ((size_t)ref >= h.bvh2.size()) { ++r.reach_bad; continue; }
            stack.push_back(h.bvh2[(size_t)ref].l);
            stack.push_back(h.bvh2[(size_t)ref].r);
        } else {
            if ((size_t)~ref >= h.bleaf.size()) { ++r.reach_bad; continue; }
            const BvhLeaf& L = h.bleaf[(size_t)~ref];
            for (int g = L.gb; g < L.gb + L.gn; ++g) {
                if (g < 0 || (size_t)g >= seen.size()) ++r.reach_bad; else ++seen[(size_t)g];
            }
        }
    }
    for (const int c : seen) r.reach_bad += c == 1 ? 0 : 1;
    // every triangle's leaf id among gleaf once; its LeafInfo holds tri_normal's normal and the record its vertices
    std::vector<int> ids(h.leaves.size(), 0);
    for (const int32_t id : h.gleaf) if (id >= 0 && (size_t)id < ids.size()) ++ids[(size_t)id];
    for (int k = 0; k < h.d.n_tri; ++k) {
        const size_t id = (size_t)h.d.leaf_base[LEAF_TRI] + (size_t)k;
        if (id >= ids.size() || ids[id] != 1) { ++r.tri_ids_bad; continue; }
        const LeafInfo& li = h.leaves[id];
        const TriRec& T = h.tri[(size_t)k];
        double n[3];
        if (li.type != LEAF_TRI || li.local != k || !tri_normal(T.v0, T.v1, T.v2, n) || std::memcmp(n, li.c, sizeof n) != 0) ++r.normals_bad;
        const double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (!(std::fabs(len - 1.0) < 1e-12)) ++r.normals_bad;
    }
    return r;
}

std::string refusal(Builder& b, int world) {
    HostScene h;
    std::string err;
    BuildOptions opt;
    return build_scene(b.s, world, opt, h, err) ? err : std::string("(accepted)");
}
}  // namespace

int main(int argc, char** argv) {
    const int side = argc > 1 ? std::atoi(argv[1]) : 24;
    Rand rr{0x5EED0501};
    Builder b;
    const int plain = b.field(side, rr);
    const int moved = b.translate(b.field(side, rr), 2.0, 0.5, -1.0);
    const int turned = b.translate(b.rotate_y(b.field(side, rr), 33.0), -2.0, 0.25, 1.5);
    std::vector<int> kids{plain, b.sphere(0.5, 1.0, 0.5, 0.3), moved, b.rect(1, -4, 4, -4, 4, -0.5), turned};
    for (int i = 0; i < 20; ++i) kids.push_back(b.sphere(4 * rr() - 2, 1 + rr(), 4 * rr() - 2, 0.1 + 0.1 * rr()));
    const int world = b.list(kids);
    const Result a = run(b.s, world, 1), c = run(b.s, world, 8), again = run(b.s, world, 1);

    Builder one;                                     // a scene of one triangle: a tree whose root is a leaf
    const double p0[3] = {0, 0, 0}, p1[3] = {1, 0, 0}, p2[3] = {0, 1, 0};
    const Result single = run(one.s, one.list({one.tri(p0, p1, p2)}), 1);

    // what the commit refuses
    Builder r1; const std::string with_curve = refusal(r1, r1.list({r1.tri(p0, p1, p2), r1.bezier()}));
    Builder r2; const std::string with_klein = refusal(r2, r2.list({r2.klein(), r2.tri(p0, p1, p2)}));
    Builder r3; const std::string with_medium = refusal(r3, r3.list({r3.tri(p0, p1, p2), r3.medium(r3.sphere(0, 0, 0, 1))}));
    Builder r4; const std::string boundary = refusal(r4, r4.list({r4.medium(r4.list({r4.tri(p0, p1, p2)}))}));
    Builder r5; const int lt = r5.tri(p0, p1, p2); r5.s.light = lt; const std::string light = refusal(r5, r5.list({lt}));
    Builder r6; const std::string far = refusal(r6, r6.list({r6.translate(r6.tri(p0, p1, p2), INFINITY, 0, 0)}));

    auto esc = [](const std::string& s) { std::string o; for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; } return o; };
    std::printf("{\"ok\": %s, \"tris\": %d, \"tri_leaves\": %d, \"n_tri\": %d, \"n_gleaf\": %d, \"outside\": %ld, \"reach_bad\": %ld, "
                "\"tri_ids_bad\": %ld, \"normals_bad\": %ld, \"same_threads\": %s, \"same_again\": %s, "
                "\"single_ok\": %s, \"single_tri_leaves\": %d, \"single_n_gleaf\": %d, \"single_bad\": %ld, "
                "\"with_curve\": \"%s\", \"with_klein\": \"%s\", \"with_medium\": \"%s\", \"boundary\": \"%s\", \"light\": \"%s\", "
                "\"far\": \"%s\", \"error\": \"%s\"}\n",
                a.ok && c.ok && again.ok ? "true" : "false", a.tris, a.tri_leaves, a.n_tri, a.n_gleaf, a.outside + c.outside,
                a.reach_bad + c.reach_bad, a.tri_ids_bad + c.tri_ids_bad, a.normals_bad + c.normals_bad,
                a.dig == c.dig ? "true" : "false", a.dig == again.dig ? "true" : "false", single.ok ? "true" : "false",
                single.tri_leaves, single.n_gleaf, single.outside + single.reach_bad + single.tri_ids_bad + single.normals_bad,
                esc(with_curve).c_str(), esc(with_klein).c_str(), esc(with_medium).c_str(), esc(boundary).c_str(),
                esc(light).c_str(), esc(far).c_str(), esc(a.err + c.err + single.err).c_str());
    return 0;
}
