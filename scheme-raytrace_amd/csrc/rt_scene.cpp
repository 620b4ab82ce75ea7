// rt_scene.cpp — the handle registry and the part of the C ABI (include/rt.h) that builds a scene:
// contexts and their options, textures, materials, objects, camera, sky, Perlin tables; and what a
// scene reports about itself (statistics, rt_get_scene_info).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rt_build.h"
#include "rt_host.h"

using namespace rtamd;

namespace {
thread_local std::string g_err;
int g_next_ctx = 1, g_next_scene = 1;
}  // namespace

namespace rtamd {
int fail(const std::string& msg) { g_err = msg; return 1; }

std::mutex g_mu;
std::map<int, std::unique_ptr<Context>> g_ctx;
std::map<int, std::unique_ptr<Scene>> g_scene;
}  // namespace rtamd

// =================================================================== C ABI
extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }
const char* rt_last_error(void) { return g_err.c_str(); }

int rt_device_count(int* out) {
    if (!out) return fail("null out pointer");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    *out = n;
    return 0;
}

int rt_context_create(int device, int* out_ctx) {
    if (!out_ctx) return fail("null out pointer");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail("device " + std::to_string(device) + " out of range (" + std::to_string(n) + " devices)");
    HIPCHK(hipSetDevice(device));
    auto c = std::make_unique<Context>();
    c->device = device;
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    std::lock_guard<std::mutex> lk(g_mu);
    int h = g_next_ctx++;
    g_ctx[h] = std::move(c);
    *out_ctx = h;
    return 0;
}

int rt_context_destroy(int ctx) {
    LOCK_CTX(c, ctx);
    for (auto it = g_scene.begin(); it != g_scene.end();) {
        if (it->second->ctx == ctx) it = g_scene.erase(it); else ++it;
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    g_ctx.erase(ctx);
    return 0;
}

int rt_context_release_pools(int ctx) {
    LOCK_CTX(c, ctx);
    HIPCHK(hipSetDevice(c->device));
    for (auto& L : c->lanes)
        if (L && L->stream) HIPCHK(hipStreamSynchronize(L->stream));
    for (auto& L : c->lanes) L.reset();
    c->pool_cap = 0;                               // the next render sizes them again
    for (DevBuf& b : c->dn_signal) b.release();   // the denoiser's scratch (sized again at its next use)
    c->dn_guide.release();
    return 0;
}

int rt_context_set_option(int ctx, int option, int64_t value) {
    LOCK_CTX(c, ctx);
    if (value < 0) return fail("option value must be >= 0 (0 = automatic)");
    switch (option) {
    case RT_OPT_LANES: {
        if (value > kLanes) return fail("RT_OPT_LANES: at most " + std::to_string(kLanes) + " render lanes");
        // more lanes than the pools were sized for: size them again for the lanes together (the next render
        // frees them first); otherwise the lanes kept hold pools of the right size, so keep them — a re-allocated pool's
        // first frame waits for the driver to clear the memory it reuses (4.7–6.6 s for C2's ~150 GB,
        // profiles/r05/ab/realloc/), which a lane-count dip (bench.py's single-lane profiling frame) need not pay
        const int64_t new_n = value > 0 ? std::min<int64_t>(value, kLanes) : 2;
        if (new_n > c->pool_lanes) c->pool_cap = 0;
        c->opt_lanes = value;
        break;
    }
    case RT_OPT_MAX_PATHS:
        if (value > ((int64_t)1 << 32)) return fail("RT_OPT_MAX_PATHS: at most 2^32 paths per pool");
        c->opt_max_paths = value;
        c->pool_cap = 0;                           // the next render sizes the pools again
        break;
    case RT_OPT_TAIL_PATHS: c->opt_tail_paths = value; break;
    case RT_OPT_TAIL_DIV: c->opt_tail_div = value; break;
    case RT_OPT_TAIL_OFF: c->wavefront_only = value != 0; break;
    case RT_OPT_EXACT_LIBM:
        if (value > RT_LIBM_DEVICE) return fail("RT_OPT_EXACT_LIBM: RT_LIBM_AUTO, RT_LIBM_EXACT or RT_LIBM_DEVICE");
        c->opt_exact_libm = value;
        break;
    default: return fail("unknown context option " + std::to_string(option));
    }
    return 0;
}

int rt_context_get_option(int ctx, int option, int64_t* out) {
    if (!out) return fail("null out pointer");
    LOCK_CTX(c, ctx);
    switch (option) {
    case RT_OPT_LANES: *out = c->opt_lanes; break;
    case RT_OPT_MAX_PATHS: *out = c->opt_max_paths; break;
    case RT_OPT_TAIL_PATHS: *out = c->opt_tail_paths; break;
    case RT_OPT_TAIL_DIV: *out = c->opt_tail_div; break;
    case RT_OPT_TAIL_OFF: *out = c->wavefront_only ? 1 : 0; break;
    case RT_OPT_EXACT_LIBM: *out = c->opt_exact_libm; break;
    default: return fail("unknown context option " + std::to_string(option));
    }
    return 0;
}

int rt_scene_begin(int ctx, int* out_scene) {
    if (!out_scene) return fail("null out pointer");
    std::lock_guard<std::mutex> lk(g_mu);
    if (!get_ctx(ctx)) return fail("invalid context handle");
    auto s = std::make_unique<Scene>();
    s->ctx = ctx;
    int h = g_next_scene++;
    g_scene[h] = std::move(s);
    *out_scene = h;
    return 0;
}

int rt_scene_destroy(int scene) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_scene.erase(scene)) return fail("invalid scene handle");
    return 0;
}

#define OUT_OR_FAIL(p) if (!(p)) return fail("null out pointer")

int rt_add_texture_constant(int scene, const double rgb[3], int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    DevTexture t{};
    t.type = TEX_CONSTANT; t.r = rgb[0]; t.g = rgb[1]; t.bl = rgb[2];
    s->texs.push_back(t);
    *out = (int)s->texs.size() - 1;
    return 0;
}
int rt_add_texture_checker(int scene, int even, int odd, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (check_tex(s, even) || check_tex(s, odd)) return 1;
    DevTexture t{};
    t.type = TEX_CHECKER; t.a = even; t.b = odd;
    s->texs.push_back(t);
    *out = (int)s->texs.size() - 1;
    return 0;
}
static int add_scaled_tex(int scene, int type, double sc, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    DevTexture t{};
    t.type = type; t.scale = sc;
    s->texs.push_back(t);
    *out = (int)s->texs.size() - 1;
    return 0;
}
int rt_add_texture_noise(int scene, double sc, int* out) { return add_scaled_tex(scene, TEX_NOISE, sc, out); }
int rt_add_texture_marble(int scene, double sc, int* out) { return add_scaled_tex(scene, TEX_MARBLE, sc, out); }
// t:image-texture (texture.scm:36-50; include/rt.h, "image textures"): the bytes packed one dword per texel
// into the scene's texel array (uploaded at commit), the texture record holding its offset and size
int rt_add_texture_image(int scene, const uint8_t* rgb, int nx, int ny, int* out) {
    // the arguments first, so they are refused whatever the handle is
    OUT_OR_FAIL(out);
    if (!rgb) return fail("rt_add_texture_image: null texel pointer");
    if (nx < 1 || ny < 1) return fail("rt_add_texture_image: nx and ny must be at least 1");
    const uint64_t n = (uint64_t)nx * (uint64_t)ny;
    if (n > (1ull << 26)) return fail("rt_add_texture_image: at most 2^26 texels per image");
    SCENE_OR_FAIL(s, scene);
    if (s->teximg.size() + n > 0x7fffffffull) return fail("rt_add_texture_image: the scene's images exceed 2^31 - 1 texels");
    DevTexture t{};
    t.type = TEX_IMAGE; t.a = nx; t.b = ny; t.off = (int32_t)s->teximg.size();
    s->teximg.resize(s->teximg.size() + (size_t)n);
    uint32_t* dst = s->teximg.data() + (size_t)t.off;
    for (size_t k = 0; k < (size_t)n; ++k)
        dst[k] = (uint32_t)rgb[3 * k] | (uint32_t)rgb[3 * k + 1] << 8 | (uint32_t)rgb[3 * k + 2] << 16;
    s->texs.push_back(t);
    *out = (int)s->texs.size() - 1;
    return 0;
}

static int add_mat(int scene, int type, int tex, double fuzz, double ref, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (type != MAT_DIELECTRIC && check_tex(s, tex)) return 1;
    DevMaterial m{};
    m.type = type; m.tex = tex; m.fuzz = fuzz; m.ref_idx = ref;
    s->mats.push_back(m);
    *out = (int)s->mats.size() - 1;
    return 0;
}
int rt_add_material_lambertian(int scene, int tex, int* out) { return add_mat(scene, MAT_LAMBERTIAN, tex, 0, 0, out); }
int rt_add_material_metal(int scene, int tex, double fuzz, int* out) { return add_mat(scene, MAT_METAL, tex, fuzz, 0, out); }
int rt_add_material_dielectric(int scene, double ref, int* out) { return add_mat(scene, MAT_DIELECTRIC, -1, 0, ref, out); }
int rt_add_material_diffuse_light(int scene, int tex, int* out) { return add_mat(scene, MAT_DIFFUSE_LIGHT, tex, 0, 0, out); }

static int push_obj(Scene* s, Obj&& o, int* out) {
    s->objs.push_back(std::move(o));
    *out = (int)s->objs.size() - 1;
    return 0;
}

int rt_add_sphere(int scene, const double c[3], double r, int mat, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (check_mat(s, mat)) return 1;
    Obj o; o.type = O_SPHERE; o.mat = mat; o.r = r;
    for (int k = 0; k < 3; ++k) o.c0[k] = c[k];
    return push_obj(s, std::move(o), out);
}
int rt_add_moving_sphere(int scene, const double c0[3], const double c1[3], double t0, double t1, double r,
                         int mat, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (check_mat(s, mat)) return 1;
    Obj o; o.type = O_MSPHERE; o.mat = mat; o.r = r; o.t0 = t0; o.t1 = t1;
    for (int k = 0; k < 3; ++k) { o.c0[k] = c0[k]; o.c1[k] = c1[k]; }
    return push_obj(s, std::move(o), out);
}
int rt_add_rect(int scene, int axis, double a0, double a1, double b0, double b1, double k, int mat, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (axis < 0 || axis > 2) return fail("rect axis must be RT_RECT_XY/XZ/YZ");
    if (check_mat(s, mat)) return 1;
    Obj o; o.type = O_RECT; o.axis = axis; o.mat = mat;
    o.a0 = a0; o.a1 = a1; o.b0 = b0; o.b1 = b1; o.k = k;
    return push_obj(s, std::move(o), out);
}
int rt_add_bezier(int scene, const double a[3], const double b[3], const double c[3], const double d[3],
                  double width, int mat, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (!a || !b || !c || !d) return fail("rt_add_bezier: null control point");
    if (check_mat(s, mat)) return 1;
    // make-bezier has no check, but a width <= 0 makes converge's depth estimate the log of a number
    // <= 0 (eps = width / 20, bezier.scm:179-192): Gauche's log returns a complex (or -inf for 0) and
    // ceiling->exact raises, so the reference fails on the first ray that tests such a curve
    if (!(width > 0.0) || !std::isfinite(width))
        return fail("rt_add_bezier: width must be positive and finite (the reference's depth estimate fails otherwise)");
    Obj o; o.type = O_BEZIER; o.mat = mat; o.width = width;
    const double* p[4] = {a, b, c, d};
    for (int i = 0; i < 4; ++i) for (int k = 0; k < 3; ++k) o.cp[3 * i + k] = p[i][k];
    return push_obj(s, std::move(o), out);
}
int rt_add_bezier_array(int scene, const double* cps, int n, double width, int mat, int* out_first) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out_first);
    if (n < 0 || (n > 0 && !cps)) return fail("rt_add_bezier_array: invalid curve array");
    if (check_mat(s, mat)) return 1;
    // make-bezier has no check, but a width <= 0 makes converge's depth estimate the log of a number
    // <= 0 (eps = width / 20, bezier.scm:179-192): Gauche's log returns a complex (or -inf for 0) and
    // ceiling->exact raises, so the reference fails on the first ray that tests such a curve
    if (!(width > 0.0) || !std::isfinite(width))
        return fail("rt_add_bezier_array: width must be positive and finite (the reference's depth estimate fails otherwise)");
    *out_first = (int)s->objs.size();
    s->objs.reserve(s->objs.size() + (size_t)n);
    for (int i = 0; i < n; ++i) {
        Obj o; o.type = O_BEZIER; o.mat = mat; o.width = width;
        for (int k = 0; k < 12; ++k) o.cp[k] = cps[(size_t)i * 12 + k];
        s->objs.push_back(std::move(o));
    }
    return 0;
}
// Triangles (include/rt.h, "triangles").  tri_obj: the arguments' checks, made before the handle is looked at
// so they are refused whatever it is; `face` names the triangle in the message (-1: rt_add_triangle's own)
static int tri_obj(const char* fn, const double* v0, const double* v1, const double* v2, const int face, Obj& o) {
    const std::string who = face < 0 ? std::string(fn) : std::string(fn) + ": face " + std::to_string(face);
    const double* p[3] = {v0, v1, v2};
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(p[i][k])) return fail(who + " has a vertex that is not finite");
            o.cp[3 * i + k] = p[i][k];
        }
    double n[3];
    if (!tri_normal(v0, v1, v2, n))
        return fail(who + " is degenerate (cross(v1 - v0, v2 - v0) has zero or non-finite length)");
    o.type = O_TRI;
    return 0;
}
int rt_add_triangle(int scene, const double v0[3], const double v1[3], const double v2[3], int mat, int* out) {
    OUT_OR_FAIL(out);
    if (!v0 || !v1 || !v2) return fail("rt_add_triangle: null vertex");
    Obj o;
    if (tri_obj("rt_add_triangle", v0, v1, v2, -1, o)) return 1;
    SCENE_OR_FAIL(s, scene);
    if (check_mat(s, mat)) return 1;
    o.mat = mat;
    return push_obj(s, std::move(o), out);
}
// rt_add_mesh and rt_add_mesh_normals (fn: the caller's name in the messages; normals = nullptr: a flat mesh)
static int add_mesh(const char* fn, int scene, const double* verts, int nv, const int32_t* faces, int nf, const double* uv,
                    const double* normals, int mat, int* out) {
    const std::string who = fn;
    OUT_OR_FAIL(out);
    if (!verts || !faces) return fail(who + ": null vertex or face array");
    if (nv < 1 || nf < 1) return fail(who + ": nv and nf must be at least 1");
    // a face's triangle: its indices checked, its vertices and texture coordinates read (tri_obj's checks)
    auto face_obj = [&](const int f, Obj& o) {
        const int32_t* ix = faces + 3 * (size_t)f;
        for (int k = 0; k < 3; ++k)
            if (ix[k] < 0 || ix[k] >= nv)
                return fail(who + ": face " + std::to_string(f) + " has vertex index " + std::to_string(ix[k]) +
                            " out of range (" + std::to_string(nv) + " vertices)");
        if (tri_obj(fn, verts + 3 * (size_t)ix[0], verts + 3 * (size_t)ix[1], verts + 3 * (size_t)ix[2], f, o)) return 1;
        if (uv) {
            o.has_uv = true;
            for (int k = 0; k < 3; ++k) { o.uv[k] = uv[2 * (size_t)ix[k]]; o.uv[3 + k] = uv[2 * (size_t)ix[k] + 1]; }
            for (int k = 0; k < 6; ++k)
                if (!std::isfinite(o.uv[k])) return fail(who + ": face " + std::to_string(f) + " has a texture coordinate that is not finite");
        }
        if (normals) {                                  // each made unit: nk = n * (1.0 / sqrt(dot(n, n)))
            o.has_nrm = true;
            for (int k = 0; k < 3; ++k) {
                const double* n = normals + 3 * (size_t)ix[k];
                if (!std::isfinite(n[0]) || !std::isfinite(n[1]) || !std::isfinite(n[2]))
                    return fail(who + ": face " + std::to_string(f) + " has a vertex normal that is not finite");
                const double len = std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
                if (!(len > 0.0) || !std::isfinite(len))
                    return fail(who + ": face " + std::to_string(f) + " has a vertex normal of zero or non-finite length");
                const double inv = 1.0 / len;
                for (int c = 0; c < 3; ++c) o.nrm[3 * k + c] = n[c] * inv;
            }
        }
        return 0;
    };
    // first pass: every face checked before the handle is looked at (and before the scene takes anything);
    // second pass: the triangles built in place, so the mesh is held once
    for (int f = 0; f < nf; ++f) {
        Obj o;
        if (face_obj(f, o)) return 1;
    }
    SCENE_OR_FAIL(s, scene);
    if (check_mat(s, mat)) return 1;
    Obj list; list.type = O_LIST;                       // the mesh: one list over its triangles, in face order
    list.kids.reserve((size_t)nf);
    s->objs.reserve(s->objs.size() + (size_t)nf + 1);
    for (int f = 0; f < nf; ++f) {
        Obj o;
        (void)face_obj(f, o);
        o.mat = mat;
        list.kids.push_back((int)s->objs.size());
        s->objs.push_back(std::move(o));
    }
    return push_obj(s, std::move(list), out);
}
int rt_add_mesh(int scene, const double* verts, int nv, const int32_t* faces, int nf, const double* uv, int mat, int* out) {
    return add_mesh("rt_add_mesh", scene, verts, nv, faces, nf, uv, nullptr, mat, out);
}
int rt_add_mesh_normals(int scene, const double* verts, int nv, const int32_t* faces, int nf, const double* uv,
                        const double* normals, int mat, int* out) {
    return add_mesh("rt_add_mesh_normals", scene, verts, nv, faces, nf, uv, normals, mat, out);
}
int rt_add_klein(int scene, const double center[3], int mat, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (!center) return fail("rt_add_klein: null centre");
    if (check_mat(s, mat)) return 1;
    Obj o; o.type = O_KLEIN; o.mat = mat;
    for (int k = 0; k < 3; ++k) o.c0[k] = center[k];
    return push_obj(s, std::move(o), out);
}
int rt_add_constant_medium(int scene, int boundary, double density, int albedo_tex, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (check_obj(s, boundary)) return 1;
    if (check_tex(s, albedo_tex)) return 1;
    if (!(density > 0.0) || !std::isfinite(density)) return fail("rt_add_constant_medium: density must be positive and finite");
    // the phase function is (m:make-lambertian a), geometry.scm:546
    DevMaterial m{};
    m.type = MAT_LAMBERTIAN; m.tex = albedo_tex;
    s->mats.push_back(m);
    Obj o; o.type = O_MEDIUM; o.child = boundary; o.r = density; o.mat = (int)s->mats.size() - 1;
    return push_obj(s, std::move(o), out);
}
int rt_set_light_sampling(int scene, int light_obj) {
    SCENE_OR_FAIL(s, scene);
    if (light_obj < 0) { s->light = -1; s->lights.clear(); return 0; }
    if (check_obj(s, light_obj)) return 1;
    const Obj* L = &s->objs[light_obj];
    while (L->type == O_FLIP) L = &s->objs[L->child];
    if (L->type != O_RECT && L->type != O_SPHERE)
        return fail("rt_set_light_sampling: the light must be a rect or a sphere (optionally flipped)");
    s->light = light_obj;
    s->lights.clear();                                  // the last of the two setters wins
    return 0;
}
int rt_set_light_list(int scene, const int* objs, int n) {
    SCENE_OR_FAIL(s, scene);
    std::vector<int> flat;
    std::string err;
    if (flatten_lights(*s, objs, n, flat, err)) return fail(err);   // (the scene is left as it was)
    s->lights.assign(objs, objs + n);
    s->light = -1;
    return 0;
}
int rt_add_flip_normals(int scene, int child, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (check_obj(s, child)) return 1;
    Obj o; o.type = O_FLIP; o.child = child; o.mat = s->objs[child].mat;
    return push_obj(s, std::move(o), out);
}
int rt_add_box(int scene, const double p0[3], const double p1[3], int mat, int* out) {
    // geometry.scm:444-463 — six rects, back faces flipped, in this order
    int r[6], tmp;
    if (rt_add_rect(scene, RT_RECT_XY, p0[0], p1[0], p0[1], p1[1], p1[2], mat, &r[0])) return 1;
    if (rt_add_rect(scene, RT_RECT_XY, p0[0], p1[0], p0[1], p1[1], p0[2], mat, &tmp)) return 1;
    if (rt_add_flip_normals(scene, tmp, &r[1])) return 1;
    if (rt_add_rect(scene, RT_RECT_XZ, p0[0], p1[0], p0[2], p1[2], p1[1], mat, &r[2])) return 1;
    if (rt_add_rect(scene, RT_RECT_XZ, p0[0], p1[0], p0[2], p1[2], p0[1], mat, &tmp)) return 1;
    if (rt_add_flip_normals(scene, tmp, &r[3])) return 1;
    if (rt_add_rect(scene, RT_RECT_YZ, p0[1], p1[1], p0[2], p1[2], p1[0], mat, &r[4])) return 1;
    if (rt_add_rect(scene, RT_RECT_YZ, p0[1], p1[1], p0[2], p1[2], p0[0], mat, &tmp)) return 1;
    if (rt_add_flip_normals(scene, tmp, &r[5])) return 1;
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    Obj o; o.type = O_BOX; o.mat = mat; o.kids.assign(r, r + 6);
    for (int k = 0; k < 3; ++k) { o.c0[k] = p0[k]; o.c1[k] = p1[k]; }
    return push_obj(s, std::move(o), out);
}
int rt_add_translate(int scene, int child, const double off[3], int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (check_obj(s, child)) return 1;
    Obj o; o.type = O_TRANSLATE; o.child = child; o.mat = s->objs[child].mat;
    for (int k = 0; k < 3; ++k) o.c0[k] = off[k];
    return push_obj(s, std::move(o), out);
}
int rt_add_rotate_y(int scene, int child, double angle, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (check_obj(s, child)) return 1;
    Obj o; o.type = O_ROTATE_Y; o.child = child; o.mat = s->objs[child].mat;
    const double radians = (kPi / 180.0) * angle;     // geometry.scm:484
    o.sin_t = std::sin(radians); o.cos_t = std::cos(radians);
    return push_obj(s, std::move(o), out);
}
int rt_add_list(int scene, const int* objs, int n, int* out) {
    SCENE_OR_FAIL(s, scene);
    OUT_OR_FAIL(out);
    if (n < 0 || (n > 0 && !objs)) return fail("invalid object list");
    Obj o; o.type = O_LIST;
    for (int i = 0; i < n; ++i) { if (check_obj(s, objs[i])) return 1; o.kids.push_back(objs[i]); }
    return push_obj(s, std::move(o), out);
}
int rt_add_bvh(int scene, const int* objs, int n, double t0, double t1, int sah, int* out) {
    (void)t0; (void)t1; (void)sah;
    if (rt_add_list(scene, objs, n, out)) return 1;
    std::lock_guard<std::mutex> lk(g_mu);
    get_scene(scene)->objs[*out].type = O_BVH;
    return 0;
}

int rt_make_camera(const double from[3], const double at[3], const double vup[3], double vfov, double aspect,
                   double aperture, double focus, double t0, double t1, double out[RT_CAMERA_DOUBLES]) {
    if (!out) return fail("null out pointer");
    // camera.scm:63-78 in the reference's evaluation order
    auto sub = [](const double* a, const double* b, double* r) { for (int k = 0; k < 3; ++k) r[k] = a[k] - b[k]; };
    auto unit = [](const double* a, double* r) {
        double d = 0.0; d += a[0] * a[0]; d += a[1] * a[1]; d += a[2] * a[2];
        const double k = 1.0 / std::sqrt(d);
        for (int i = 0; i < 3; ++i) r[i] = a[i] * k;
    };
    auto cross = [](const double* a, const double* b, double* r) {
        r[0] = a[1] * b[2] - b[1] * a[2]; r[1] = a[2] * b[0] - b[2] * a[0]; r[2] = a[0] * b[1] - b[0] * a[1];
    };
    const double theta = vfov * (kPi / 180.0);
    const double hh = std::tan(theta / 2);
    const double hw = aspect * hh;
    double w[3], u[3], v[3], tmp[3];
    sub(from, at, tmp); unit(tmp, w);
    cross(vup, w, tmp); unit(tmp, u);
    cross(w, u, v);
    for (int k = 0; k < 3; ++k) {
        double llc = from[k] - u[k] * (hw * focus);
        llc = llc - v[k] * (hh * focus);
        llc = llc - w[k] * focus;
        out[k] = llc;
        out[3 + k] = u[k] * (2 * hw * focus);
        out[6 + k] = v[k] * (2 * hh * focus);
        out[9 + k] = from[k];
        out[12 + k] = w[k]; out[15 + k] = u[k]; out[18 + k] = v[k];
    }
    out[21] = aperture / 2; out[22] = t0; out[23] = t1;
    return 0;
}

int rt_set_camera(int scene, const double cam[RT_CAMERA_DOUBLES]) {
    SCENE_OR_FAIL(s, scene);
    if (!cam) return fail("null camera");
    std::memcpy(s->cam, cam, sizeof s->cam);
    s->have_cam = true;
    return 0;
}
int rt_set_sky(int scene, int sky) {
    SCENE_OR_FAIL(s, scene);
    if (sky != RT_SKY_GRADIENT && sky != RT_SKY_BLACK) return fail("sky must be RT_SKY_GRADIENT or RT_SKY_BLACK");
    s->sky = sky;
    return 0;
}
int rt_set_perlin_tables(int scene, const double ranvec[768], const int32_t px[256], const int32_t py[256],
                         const int32_t pz[256]) {
    SCENE_OR_FAIL(s, scene);
    if (!ranvec || !px || !py || !pz) return fail("null Perlin table");
    s->ranvec.assign(ranvec, ranvec + 768);
    s->perm.resize(768);
    for (int i = 0; i < 256; ++i) {
        if (px[i] < 0 || px[i] > 255 || py[i] < 0 || py[i] > 255 || pz[i] < 0 || pz[i] > 255)
            return fail("Perlin permutation entries must be in 0..255");
        s->perm[i] = px[i]; s->perm[256 + i] = py[i]; s->perm[512 + i] = pz[i];
    }
    s->have_perlin = true;
    return 0;
}

int rt_set_profiling(int scene, int enabled) {
    LOCK_SCENE(s, scene);
    s->profiling = enabled != 0;
    return 0;
}

int rt_get_stats(int scene, rt_stats* out) {
    LOCK_SCENE(s, scene);
    if (!out) return fail("null out pointer");
    *out = s->stats;
    return 0;
}

int rt_get_scene_info(int scene, rt_scene_info* out) {
    LOCK_SCENE(s, scene);
    if (!out) return fail("null out pointer");
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    CTX_OF(c, s);
    const DevScene& d = s->dev;
    std::memset(out, 0, sizeof *out);
    out->leaves = d.n_leaves;
    out->groups = d.n_groups;
    out->bvh_nodes = d.n_bvh2;
    out->bvh0_nodes = d.n_fbvh2;
    out->tree_depth = d.lane_stack;
    out->bvh_solo = d.bvh_solo;
    out->extend_lds_bytes = (uint32_t)s->ext_lds;
    out->extend_lds_blocks = s->ext_lds_blocks;
    out->camera_lds_bytes = (uint32_t)s->cam_lds;
    out->camera_lds_blocks = s->cam_blocks;
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    out->cus = cus;
    out->curve_stack = d.bvh4 ? d.stack4 : 0;
    out->commit_ms = s->commit_ms;
    out->commit_upload_ms = s->commit_upload_ms;
    out->commit_sah_ms = s->commit_sah_ms;
    out->commit_threads = s->commit_threads;
    out->tree0_any_time = d.tree0_any_time;
    return 0;
}

int rt_get_tree_info(int scene, rt_tree_info* out) {
    LOCK_SCENE(s, scene);
    if (!out) return fail("null out pointer");
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    *out = s->tree;
    return 0;
}

}  // extern "C"
