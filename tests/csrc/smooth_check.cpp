// smooth_check.cpp — build_scene (rt_build.cpp) on meshes with per-vertex shading normals, filled directly into a
// SceneDesc: an 80-triangle mesh (an icosphere of level 1) whose every corner carries a normal of its own,
// under no chain and under rotate-y + translate, beside a plain mesh without normals, among spheres and a rect.
// Checks that TriNrm follows the tree's order as TriRec does: every record's normals are those of the
// triangle whose vertices the TriRec at the same index holds (the triangle is recognised by its vertices, which
// are distinct per triangle and per mesh); that has is 0 for every triangle of the plain mesh; that
// DevScene::tri_smooth is set (and stays 0 in a scene without normals); and that 1 and 8 threads give one digest.
// Host code with its own main (no GPU), compiled with g++ beside rt_build.cpp, under ASan / UBSan.
// Prints one JSON object.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../scheme-raytrace_amd/csrc/rt_build.h"

using namespace rtamd;

namespace {
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

    // an icosphere of level 1 (80 triangles) of radius `radius`; tag >= 0: corner k of face f carries the unit
    // normal of (vertex + 0.01 * (tag + 1) * (f + 1, k + 1, 1)), distinct for every corner of every mesh;
    // tag < 0: a plain mesh
    int ball(double radius, int tag) {
        const double p = (1.0 + std::sqrt(5.0)) / 2.0;
        std::vector<std::vector<double>> vs = {{-1, p, 0}, {1, p, 0}, {-1, -p, 0}, {1, -p, 0}, {0, -1, p}, {0, 1, p}, {0, -1, -p},
                                               {0, 1, -p}, {p, 0, -1}, {p, 0, 1}, {-p, 0, -1}, {-p, 0, 1}};
        std::vector<std::vector<int>> fs = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4},
                                            {11, 10, 2}, {10, 7, 6}, {7, 1, 8}, {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8},
                                            {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
        auto unit = [](std::vector<double> q) { const double l = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]); for (double& x : q) x /= l; return q; };
        for (auto& q : vs) q = unit(q);
        std::map<std::pair<int, int>, int> mid;
        auto midpoint = [&](int a, int b) {
            const std::pair<int, int> key = a < b ? std::make_pair(a, b) : std::make_pair(b, a);
            auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            vs.push_back(unit({0.5 * (vs[a][0] + vs[b][0]), 0.5 * (vs[a][1] + vs[b][1]), 0.5 * (vs[a][2] + vs[b][2])}));
            return mid[key] = (int)vs.size() - 1;
        };
        std::vector<std::vector<int>> nxt;
        for (const auto& f : fs) {
            const int ab = midpoint(f[0], f[1]), bc = midpoint(f[1], f[2]), ca = midpoint(f[2], f[0]);
            nxt.push_back({f[0], ab, ca}); nxt.push_back({f[1], bc, ab}); nxt.push_back({f[2], ca, bc}); nxt.push_back({ab, bc, ca});
        }
        std::vector<int> kids;
        for (size_t f = 0; f < nxt.size(); ++f) {
            Obj o; o.type = O_TRI; o.mat = 1;
            for (int k = 0; k < 3; ++k) {
                const std::vector<double>& v = vs[(size_t)nxt[f][k]];
                for (int c = 0; c < 3; ++c) o.cp[3 * k + c] = radius * v[c];
                if (tag >= 0) {
                    const double e = 0.01 * (tag + 1);
                    const std::vector<double> n = unit({v[0] + e * (double)(f + 1), v[1] + e * (k + 1), v[2] + e});
                    for (int c = 0; c < 3; ++c) o.nrm[3 * k + c] = n[c];
                }
            }
            o.has_nrm = tag >= 0;
            kids.push_back(add(o));
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
    x = fnv_vec(x, h.tri); x = fnv_vec(x, h.bvh2); x = fnv_vec(x, h.bleaf); x = fnv_vec(x, h.gleaf); x = fnv_vec(x, h.leaf_pos);
    x = fnv_vec(x, h.order); x = fnv_vec(x, h.leaves);
    for (const TriNrm& q : h.trinrm) { x = fnv(x, q.n, sizeof q.n); x = fnv(x, &q.has, sizeof q.has); }
    x = fnv(x, &h.d.tri_smooth, sizeof h.d.tri_smooth);
    return x;
}

struct Result { bool ok = false; std::string err; uint64_t dig = 0; int n_tri = 0, n_nrm = 0, smooth = 0, plain = 0, tri_smooth = 0;
                long unknown = 0, mismatched = 0, plain_bad = 0, not_unit = 0; };

Result run(const SceneDesc& s, int world, int threads) {
    Result r;
    HostScene h;
    BuildOptions opt;
    opt.threads = threads;
    if (build_scene(s, world, opt, h, r.err)) return r;
    r.ok = true;
    r.dig = digest(h);
    r.n_tri = (int)h.tri.size(); r.n_nrm = (int)h.trinrm.size(); r.tri_smooth = h.d.tri_smooth;
    if (h.trinrm.size() != h.tri.size()) return r;
    for (size_t k = 0; k < h.tri.size(); ++k) {
        const TriRec& T = h.tri[k];
        const TriNrm& N = h.trinrm[k];
        const Obj* src = nullptr;                    // the triangle this record's vertices belong to
        for (const Obj& o : s.objs)
            if (o.type == O_TRI && std::memcmp(o.cp, T.v0, sizeof T.v0) == 0 && std::memcmp(o.cp + 3, T.v1, sizeof T.v1) == 0 &&
                std::memcmp(o.cp + 6, T.v2, sizeof T.v2) == 0) { src = &o; break; }
        if (!src) { ++r.unknown; continue; }
        if (src->has_nrm) {
            ++r.smooth;
            if (N.has != 1 || std::memcmp(N.n, src->nrm, sizeof N.n) != 0) ++r.mismatched;
            for (int i = 0; i < 3; ++i)
                if (!(std::fabs(std::sqrt((N.n[i][0] * N.n[i][0] + N.n[i][1] * N.n[i][1]) + N.n[i][2] * N.n[i][2]) - 1.0) < 1e-12)) ++r.not_unit;
        } else {
            ++r.plain;
            const double zero[9] = {0};
            if (N.has != 0 || std::memcmp(N.n, zero, sizeof zero) != 0) ++r.plain_bad;
        }
    }
    return r;
}
}  // namespace

int main() {
    Builder b;
    // radii differ, so a triangle's vertices name its mesh
    const int smooth = b.ball(1.0, 0);
    const int plain = b.translate(b.ball(0.75, -1), 3.0, 0.0, 0.0);
    const int turned = b.translate(b.rotate_y(b.ball(1.25, 1), 33.0), -3.0, 0.25, 1.5);
    std::vector<int> kids{smooth, b.sphere(0.5, 2.0, 0.5, 0.3), plain, b.rect(1, -6, 6, -6, 6, -1.5), turned};
    for (int i = 0; i < 20; ++i) kids.push_back(b.sphere(-5.0 + 0.5 * i, 2.5, 0.25 * i - 2.0, 0.1));
    const int world = b.list(kids);
    const Result a = run(b.s, world, 1), c = run(b.s, world, 8);

    Builder f;                                       // no normals anywhere: tri_smooth stays 0
    const Result flat = run(f.s, f.list({f.ball(1.0, -1), f.sphere(0, 3, 0, 0.5)}), 1);

    auto esc = [](const std::string& s) { std::string o; for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; } return o; };
    std::printf("{\"ok\": %s, \"n_tri\": %d, \"n_nrm\": %d, \"smooth\": %d, \"plain\": %d, \"tri_smooth\": %d, \"unknown\": %ld, "
                "\"mismatched\": %ld, \"plain_bad\": %ld, \"not_unit\": %ld, \"same_threads\": %s, \"flat_ok\": %s, "
                "\"flat_tri_smooth\": %d, \"flat_plain\": %d, \"flat_bad\": %ld, \"error\": \"%s\"}\n",
                a.ok && c.ok ? "true" : "false", a.n_tri, a.n_nrm, a.smooth, a.plain, a.tri_smooth && c.tri_smooth, a.unknown + c.unknown,
                a.mismatched + c.mismatched, a.plain_bad + c.plain_bad, a.not_unit + c.not_unit,
                a.dig == c.dig && c.smooth == a.smooth && c.plain == a.plain ? "true" : "false", flat.ok ? "true" : "false",
                flat.tri_smooth, flat.plain, flat.unknown + flat.mismatched + flat.plain_bad + (long)flat.smooth,
                esc(a.err + c.err + flat.err).c_str());
    return 0;
}
