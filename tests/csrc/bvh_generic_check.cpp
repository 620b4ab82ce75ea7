// bvh_generic_check.cpp — the world-space boxes of generic tree leaves (scheme-raytrace_amd/csrc/rt_leafbox.h)
// and the tree built over them (rt_bvh.h), on the host (no GPU): for a box-field-like input (rects under no
// chain) and a city-like one (boxes, spheres and moving spheres under translate o rotate-y chains, one
// three-op chain among them), every leaf's box contains 1000 sampled surface points of the primitive carried
// through its chain; the serial and the 8-thread builds are the same tree bit for bit; primitives that are
// not finite are "not a tree leaf".  Prints one JSON line.  usage: bvh_generic_check [N_PER_SIDE]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../scheme-raytrace_amd/csrc/rt_bvh.h"
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
struct Leaf { LeafGeom g; std::vector<ChainOpRec> ops; };

ChainOpRec translate(double x, double y, double z) { ChainOpRec o{}; o.op = OP_TRANSLATE; o.x = x; o.y = y; o.z = z; return o; }
ChainOpRec rotate(double deg) {
    ChainOpRec o{};
    const double rad = (kPi / 180.0) * deg;
    o.op = OP_ROTATE_Y; o.x = std::sin(rad); o.y = std::cos(rad);
    return o;
}
LeafGeom rect(int type, double a0, double a1, double b0, double b1, double k) {
    LeafGeom g{};
    g.type = type; g.a0 = a0; g.a1 = a1; g.b0 = b0; g.b1 = b1; g.k = k;
    return g;
}
// g:make-box (geometry.scm:444-463): six rects
void add_box(std::vector<Leaf>& out, const double* p0, const double* p1, const std::vector<ChainOpRec>& ops) {
    out.push_back({rect(LEAF_RECT_XY, p0[0], p1[0], p0[1], p1[1], p1[2]), ops});
    out.push_back({rect(LEAF_RECT_XY, p0[0], p1[0], p0[1], p1[1], p0[2]), ops});
    out.push_back({rect(LEAF_RECT_XZ, p0[0], p1[0], p0[2], p1[2], p1[1]), ops});
    out.push_back({rect(LEAF_RECT_XZ, p0[0], p1[0], p0[2], p1[2], p0[1]), ops});
    out.push_back({rect(LEAF_RECT_YZ, p0[1], p1[1], p0[2], p1[2], p1[0]), ops});
    out.push_back({rect(LEAF_RECT_YZ, p0[1], p1[1], p0[2], p1[2], p0[0]), ops});
}
// a point of the primitive's surface in its local frame (a moving sphere: at a time in [tlo, thi])
void surface_point(const LeafGeom& g, Rand& rr, double tlo, double thi, double* p) {
    if (g.type == LEAF_SPHERE || g.type == LEAF_MSPHERE) {
        double u[3], n = 0;
        do {
            n = 0;
            for (int k = 0; k < 3; ++k) { u[k] = 2 * rr() - 1; n += u[k] * u[k]; }
        } while (n < 1e-3 || n > 1);
        n = std::sqrt(n);
        double f = 0;
        if (g.type == LEAF_MSPHERE) f = ((tlo + (thi - tlo) * rr()) - g.t0) / (g.t1 - g.t0);
        for (int k = 0; k < 3; ++k) p[k] = g.c0[k] + (g.c1[k] - g.c0[k]) * f + std::fabs(g.r) * u[k] / n;
        return;
    }
    const int ia = g.type == LEAF_RECT_YZ ? 1 : 0, ib = g.type == LEAF_RECT_XY ? 1 : 2, ik = 3 - ia - ib;
    const double fa = rr() < 0.1 ? (rr() < 0.5 ? 0.0 : 1.0) : rr(), fb = rr() < 0.1 ? (rr() < 0.5 ? 0.0 : 1.0) : rr();
    p[ia] = g.a0 + (g.a1 - g.a0) * fa;               // (edges and corners among them)
    p[ib] = g.b0 + (g.b1 - g.b0) * fb;
    p[ik] = g.k;
}

struct Built { std::vector<BvhNode> nodes; std::vector<PrimRef> refs; std::vector<BvhNode2> bvh2; std::vector<BvhLeaf> leaf; int32_t root = 0, depth = 0; };
Built build(std::vector<PrimRef> refs, int threads) {
    Built b;
    BvhBuild bb{refs, {}};
    bb.leaf_max = 1;
    bb.sweep_max = 1 << 16;
    bb.threads = threads;
    bb.build(0, (int)refs.size(), 0);
    b.nodes = bb.nodes;
    b.refs = refs;
    flatten_bvh2(b.nodes, 1e-6, [](int s, int e) { return BvhLeaf{0, 0, 0, 0, 0, 0, s, e - s}; }, b.bvh2, b.leaf, b.root,
                 b.depth, threads);
    return b;
}
template <class T> bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// the checks on one leaf set; returns the number of sampled points outside their leaf's box
long check(const char* name, const std::vector<Leaf>& leaves, double tlo, double thi, bool* same_build, size_t* n_refs) {
    Rand rr{0x5EED0406};
    std::vector<PrimRef> refs;
    long outside = 0;
    for (size_t i = 0; i < leaves.size(); ++i) {
        const Leaf& L = leaves[i];
        PrimRef r{};
        if (!leaf_world_box(L.g, L.ops.data(), (int)L.ops.size(), tlo, thi, r.lo, r.hi)) {
            std::fprintf(stderr, "%s: leaf %zu is not a tree leaf\n", name, i);
            return -1;
        }
        for (int s = 0; s < 1000; ++s) {
            double p[3];
            surface_point(L.g, rr, tlo, thi, p);
            chain_point(L.ops.data(), (int)L.ops.size(), p);
            for (int k = 0; k < 3; ++k)
                if (!(p[k] >= r.lo[k] && p[k] <= r.hi[k])) { ++outside; break; }
        }
        for (int k = 0; k < 3; ++k) r.c[k] = 0.5 * (r.lo[k] + r.hi[k]);
        r.leaf = (int)i;
        r.type = L.g.type;
        refs.push_back(r);
    }
    const Built a = build(refs, 1), b = build(refs, 8);
    bool order = a.refs.size() == b.refs.size();
    for (size_t i = 0; order && i < a.refs.size(); ++i) order = a.refs[i].leaf == b.refs[i].leaf;
    *same_build = order && same(a.nodes, b.nodes) && same(a.bvh2, b.bvh2) && same(a.leaf, b.leaf) && a.root == b.root &&
                  a.depth == b.depth;
    // every primitive in exactly one leaf range
    std::vector<int> seen(refs.size(), 0);
    for (const BvhLeaf& L : a.leaf)
        for (int g = L.gb; g < L.gb + L.gn; ++g)
            if (g >= 0 && g < (int)seen.size()) ++seen[(size_t)g];
    for (const int s : seen) *same_build = *same_build && s == 1;
    *n_refs = refs.size();
    return outside;
}
}  // namespace

int main(int argc, char** argv) {
    const int side = argc > 1 ? std::atoi(argv[1]) : 32;
    Rand rr{0x5EED0407};
    // box field: side x side boxes on [-4, 4]^2 under no chain (as many rects as the threaded build needs:
    // subtrees of at least BvhBuild::kGrain primitives go to other threads)
    std::vector<Leaf> field;
    const double w = 8.0 / side;
    for (int i = 0; i < side; ++i)
        for (int j = 0; j < side; ++j) {
            const double p0[3] = {-4 + i * w, 0, -4 + j * w}, p1[3] = {p0[0] + w, 0.2 + 0.8 * rr(), p0[2] + w};
            add_box(field, p0, p1, {});
        }
    // city: boxes, spheres and moving spheres, each under its own translate o rotate-y (outermost first, as
    // the Flattener records chains); every eighth under a three-op chain
    std::vector<Leaf> city;
    for (int i = 0; i < side * side; ++i) {
        std::vector<ChainOpRec> ops = {translate(-4.5 + 9 * rr(), 0.5 * rr(), -4.5 + 9 * rr()), rotate(-180 + 360 * rr())};
        if (i % 8 == 7) ops.push_back(translate(rr(), 0, rr()));
        const double p0[3] = {0, 0, 0}, p1[3] = {0.4 + 0.5 * rr(), 0.3 + 1.5 * rr(), 0.4 + 0.5 * rr()};
        if (i % 3 == 0) {
            add_box(city, p0, p1, ops);
            continue;
        }
        LeafGeom g{};
        g.type = i % 3 == 1 ? LEAF_SPHERE : LEAF_MSPHERE;
        for (int k = 0; k < 3; ++k) { g.c0[k] = 2 * rr(); g.c1[k] = g.c0[k] + 0.5 * rr(); }
        g.r = (i % 5 == 0 ? -1 : 1) * (0.05 + 0.3 * rr());          // (a negative radius: a hollow shell)
        g.t0 = i % 2 ? 0.0 : -0.5; g.t1 = g.t0 + 1.0 + rr();
        city.push_back({g, ops});
    }
    bool same_field = false, same_city = false;
    size_t nf = 0, nc = 0;
    const long out_field = check("field", field, 0.0, 1.0, &same_field, &nf);
    const long out_city = check("city", city, 0.0, 1.0, &same_city, &nc);
    // not tree leaves: a NaN or infinite coordinate in the primitive or in its chain, a degenerate shutter,
    // a coordinate too large to pad
    int refused = 0, asked = 0;
    auto refuse = [&](LeafGeom g, std::vector<ChainOpRec> ops) {
        double lo[3], hi[3];
        ++asked;
        refused += leaf_world_box(g, ops.data(), (int)ops.size(), 0.0, 1.0, lo, hi) ? 0 : 1;
    };
    refuse(rect(LEAF_RECT_XY, 0, 1, 0, NAN, 2), {});
    refuse(rect(LEAF_RECT_XZ, 0, INFINITY, 0, 1, 2), {});
    refuse(rect(LEAF_RECT_YZ, 0, 1, 0, 1, -INFINITY), {rotate(30)});
    refuse(rect(LEAF_RECT_YZ, 0, 1, 0, 1, 2), {translate(0, NAN, 0)});
    refuse(rect(LEAF_RECT_XY, 0, 1, 0, 1, 2), {translate(INFINITY, 0, 0), rotate(10)});
    refuse(rect(LEAF_RECT_XY, 0, 1e300, 0, 1, 2), {});
    {
        LeafGeom g{};
        g.type = LEAF_MSPHERE; g.r = 1; g.t0 = 0.5; g.t1 = 0.5; g.c1[0] = 1;     // t0 = t1: center(t) is 0/0
        refuse(g, {translate(1, 0, 0)});
        g.type = LEAF_SPHERE; g.r = NAN;
        refuse(g, {translate(1, 0, 0)});
    }
    double lo[3], hi[3];
    const bool finite_ok = leaf_world_box(rect(LEAF_RECT_XZ, -1, 1, -1, 1, 0), nullptr, 0, 0.0, 1.0, lo, hi) &&
                           lo[1] < 0 && hi[1] > 0 && lo[0] < -1 && hi[2] > 1;
    std::printf("{\"field_leaves\": %zu, \"city_leaves\": %zu, \"outside_field\": %ld, \"outside_city\": %ld, "
                "\"same_field\": %s, \"same_city\": %s, \"refused\": %d, \"asked\": %d, \"finite_ok\": %s}\n",
                nf, nc, out_field, out_city, same_field ? "true" : "false", same_city ? "true" : "false", refused, asked,
                finite_ok ? "true" : "false");
    return (out_field == 0 && out_city == 0 && same_field && same_city && refused == asked && finite_ok) ? 0 : 1;
}
