// lights_check.cpp — the light list of include/rt.h ("light lists") through build_scene (rt_build.cpp), on a
// SceneDesc filled directly: the flattening's order and counts through nested lists and a mesh, a flip looked
// through, a known triangle's area and unit normal, one rect / one sphere filling DevLight with no record, the
// cap at RT_MAX_LIGHTS, every refusal, and one digest for repeated builds.
// Host code with its own main (no GPU), compiled with g++ beside rt_build.cpp, under ASan / UBSan.
// Prints one JSON object.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../scheme-raytrace_amd/csrc/rt_build.h"

using namespace rtamd;

namespace {
struct Builder {
    SceneDesc s;
    int world = -1;
    Builder() {
        s.have_cam = true;
        s.cam[9] = 0; s.cam[10] = 1; s.cam[11] = 8;
        s.cam[22] = 0.0; s.cam[23] = 1.0;
        DevTexture t{}; t.type = TEX_CONSTANT; t.r = 0.5; t.g = 0.25; t.bl = 0.125;
        s.texs.push_back(t);
        for (int m = 0; m < 4; ++m) { DevMaterial M{}; M.type = m; M.tex = 0; M.fuzz = 0.1; M.ref_idx = 1.5; s.mats.push_back(M); }
        world = list({sphere(0, -100, 0, 100), rect(1, -1, 1, -1, 1, 3)});   // (a light need not be in the world)
    }
    int add(Obj o) { s.objs.push_back(std::move(o)); return (int)s.objs.size() - 1; }
    int sphere(double x, double y, double z, double r) { Obj o; o.type = O_SPHERE; o.mat = 0; o.c0[0] = x; o.c0[1] = y; o.c0[2] = z; o.r = r; return add(o); }
    int msphere() { Obj o; o.type = O_MSPHERE; o.mat = 0; o.r = 1; o.t1 = 1; o.c1[0] = 1; return add(o); }
    int rect(int axis, double a0, double a1, double b0, double b1, double k) {
        Obj o; o.type = O_RECT; o.axis = axis; o.mat = 3; o.a0 = a0; o.a1 = a1; o.b0 = b0; o.b1 = b1; o.k = k; return add(o);
    }
    int tri(double ax, double ay, double az, double bx, double by, double bz, double cx, double cy, double cz) {
        Obj o; o.type = O_TRI; o.mat = 3;
        const double v[9] = {ax, ay, az, bx, by, bz, cx, cy, cz};
        for (int k = 0; k < 9; ++k) o.cp[k] = v[k];
        return add(o);
    }
    int unary(ObjType t, int child) { Obj o; o.type = t; o.child = child; o.mat = s.objs[child].mat; return add(o); }
    int list(std::vector<int> kids, ObjType t = O_LIST) { Obj o; o.type = t; o.kids = std::move(kids); return add(o); }
    int bezier() { Obj o; o.type = O_BEZIER; o.mat = 0; o.width = 0.1; for (int k = 0; k < 12; ++k) o.cp[k] = 0.1 * k; return add(o); }
    int klein() { Obj o; o.type = O_KLEIN; o.mat = 0; return add(o); }
    int medium(int child) { Obj o; o.type = O_MEDIUM; o.child = child; o.r = 0.5; o.mat = 0; return add(o); }
    int box() { return list({rect(0, 0, 1, 0, 1, 1), rect(0, 0, 1, 0, 1, 0)}, O_BOX); }
    // n triangles as one list, as rt_add_mesh makes it
    int mesh(int n) {
        std::vector<int> kids;
        for (int i = 0; i < n; ++i) kids.push_back(tri(i, 5, 0, i + 1, 5, 0, i, 5, 1));
        return list(kids);
    }
    // build with `lights` as the list: "" or the refusal's text
    std::string build(std::vector<int> lights, HostScene& h) {
        s.lights = std::move(lights);
        s.light = -1;
        std::string err;
        BuildOptions opt;
        return build_scene(s, world, opt, h, err) ? (err.empty() ? std::string("(no text)") : err) : std::string();
    }
    std::string refusal(std::vector<int> lights) { HostScene h; const std::string e = build(std::move(lights), h); return e.empty() ? "(accepted)" : e; }
};

uint64_t fnv(uint64_t x, const void* p, size_t n) {
    for (size_t k = 0; k < n; ++k) x = (x ^ static_cast<const uint8_t*>(p)[k]) * 1099511628211ull;
    return x;
}
uint64_t digest(const HostScene& h) {
    uint64_t x = 1469598103934665603ull;
    if (!h.lights.empty()) x = fnv(x, h.lights.data(), h.lights.size() * sizeof(DevLightRec));
    x = fnv(x, &h.d.light, sizeof h.d.light);
    x = fnv(x, &h.d.n_lights, sizeof h.d.n_lights);
    return x;
}
std::string esc(const std::string& s) { std::string o; for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; } return o; }
}  // namespace

int main() {
    std::string out = "{";
    auto put = [&](const char* key, const std::string& v, bool quote) {
        if (out.size() > 1) out += ", ";
        out += std::string("\"") + key + "\": " + (quote ? "\"" + esc(v) + "\"" : v);
    };
    auto flag = [&](const char* key, bool v) { put(key, v ? "true" : "false", false); };

    {   // order and counts: [rect, [sphere, flip(tri), [mesh(3)]], flip(flip(rect)), sphere] -> 8 lights
        Builder b;
        const int r0 = b.rect(1, 213, 343, 227, 332, 554), s0 = b.sphere(1, 2, 3, 0.5);
        const int t0 = b.tri(0, 0, 0, 2, 0, 0, 0, 2, 0), m3 = b.mesh(3), r1 = b.rect(2, 0, 1, 0, 2, 7), s1 = b.sphere(4, 5, 6, 2);
        const int nested = b.list({s0, b.unary(O_FLIP, t0), b.list({m3})});
        HostScene h, again;
        const std::string e = b.build({r0, nested, b.unary(O_FLIP, b.unary(O_FLIP, r1)), s1}, h);
        put("order_error", e, true);
        std::string types;
        for (const DevLightRec& r : h.lights) types += (char)('0' + r.type);
        put("types", types, true);                       // 1 rect, 2 sphere, 4 triangle
        flag("list_type", h.d.light.type == LIGHT_LIST && h.d.n_lights == 8);
        flag("tri_flag", h.d.lights_tri == 1);
        bool vals = h.lights.size() == 8;
        if (vals) {
            const DevLightRec& R0 = h.lights[0]; const DevLightRec& S0 = h.lights[1]; const DevLightRec& T0 = h.lights[2];
            const DevLightRec& M1 = h.lights[4]; const DevLightRec& R1 = h.lights[6]; const DevLightRec& S1 = h.lights[7];
            vals = vals && R0.axis == 1 && R0.t.v0[0] == 213 && R0.t.v0[1] == 343 && R0.t.v0[2] == 227 && R0.t.v1[0] == 332 && R0.t.v1[1] == 554;
            vals = vals && S0.t.v0[0] == 1 && S0.t.v0[1] == 2 && S0.t.v0[2] == 3 && S0.t.v1[0] == 0.5;
            vals = vals && T0.t.v1[0] == 2 && T0.t.v2[1] == 2;
            vals = vals && M1.t.v0[0] == 1 && M1.t.v1[0] == 2 && M1.t.v0[1] == 5;          // the mesh's second face
            vals = vals && R1.axis == 2 && R1.t.v1[1] == 7 && S1.t.v1[0] == 2;
            // the known triangle: area 2, unit normal (0, 0, 1), as tri_normal forms it
            double nu[3];
            (void)tri_normal(T0.t.v0, T0.t.v1, T0.t.v2, nu);
            flag("tri_area_nu", T0.t.pad0 == 2.0 && std::memcmp(nu, T0.nu, sizeof nu) == 0 && nu[0] == 0 && nu[1] == 0 && nu[2] == 1);
            flag("mesh_area", M1.t.pad0 == 0.5);
        }
        flag("values", vals);
        const std::string e2 = b.build(b.s.lights, again);
        flag("same_again", e2.empty() && digest(h) == digest(again));
    }
    {   // a list of one rect / one sphere (flipped, nested) is the single light: DevLight filled, no record
        Builder b;
        const int r = b.rect(1, 213, 343, 227, 332, 554), s = b.sphere(1, 2, 3, 0.5), t = b.tri(0, 0, 0, 2, 0, 0, 0, 2, 0);
        HostScene hr, hs, ht, hold;
        const std::string er = b.build({b.list({b.unary(O_FLIP, r)})}, hr), es = b.build({s}, hs), et = b.build({t}, ht);
        b.s.lights.clear();
        b.s.light = r;                                   // rt_set_light_sampling's way
        std::string err; BuildOptions opt;
        const bool old_ok = build_scene(b.s, b.world, opt, hold, err) == 0;
        flag("one_rect", er.empty() && hr.d.light.type == LIGHT_RECT && hr.d.n_lights == 0 && hr.lights.empty() &&
                             old_ok && std::memcmp(&hr.d.light, &hold.d.light, sizeof(DevLight)) == 0);
        flag("one_sphere", es.empty() && hs.d.light.type == LIGHT_SPHERE && hs.d.n_lights == 0 && hs.lights.empty() &&
                               hs.d.light.cx == 1 && hs.d.light.cy == 2 && hs.d.light.cz == 3 && hs.d.light.r == 0.5);
        flag("one_tri", et.empty() && ht.d.light.type == LIGHT_LIST && ht.d.n_lights == 1 && ht.lights.size() == 1);
        HostScene hoff;
        const std::string eo = b.build({}, hoff);
        flag("off", eo.empty() && hoff.d.light.type == LIGHT_OFF && hoff.d.n_lights == 0);
    }
    {   // the cap
        Builder b;
        const int m4096 = b.mesh(RT_MAX_LIGHTS), extra = b.tri(0, 0, 0, 1, 0, 0, 0, 1, 0);
        HostScene h;
        const std::string e = b.build({m4096}, h);
        flag("cap_4096", e.empty() && h.d.n_lights == RT_MAX_LIGHTS);
        put("cap_4097", b.refusal({m4096, extra}), true);
    }
    {   // refusals
        Builder b;
        const int s = b.sphere(0, 0, 0, 1);
        put("box", b.refusal({s, b.box()}), true);
        put("moving_sphere", b.refusal({b.msphere()}), true);
        put("translate", b.refusal({b.unary(O_TRANSLATE, s)}), true);
        put("rotate_y", b.refusal({b.list({b.unary(O_ROTATE_Y, s)})}), true);
        put("bvh", b.refusal({b.list({s}, O_BVH)}), true);
        put("curve", b.refusal({b.bezier()}), true);
        put("medium", b.refusal({b.medium(s)}), true);
        put("klein", b.refusal({b.unary(O_FLIP, b.klein())}), true);
        put("bad_id", b.refusal({s, 1 << 20}), true);
        put("negative_id", b.refusal({-1}), true);
        put("empty", b.refusal({b.list({b.list({})})}), true);
        const int f = b.unary(O_FLIP, s);                // a flip of itself: only a description filled directly can hold one
        b.s.objs[(size_t)f].child = f;
        put("flip_cycle", b.refusal({f}), true);
        std::vector<int> flat;
        std::string err;
        flag("null_objs", flatten_lights(b.s, nullptr, 2, flat, err) != 0 && err.find("null") != std::string::npos);
        err.clear();
        flag("negative_n", flatten_lights(b.s, &s, -1, flat, err) != 0 && err.find(">= 0") != std::string::npos);
        flag("zero_n", flatten_lights(b.s, nullptr, 0, flat, err) == 0 && flat.empty());
    }
    std::printf("%s}\n", out.c_str());
    return 0;
}
