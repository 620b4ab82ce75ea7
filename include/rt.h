/*
 * rt.h — C ABI of the MI355X wavefront path tracer (librtamd.so).
 *
 * This is the drop-in boundary for the reference's hot path: the per-pixel
 * `trace-all` → recursive `color` loop of soma-arc/scheme-raytrace
 * (main.scm:100-121, 471-491) and everything it calls through the
 * closure-vector protocol (geometry.scm:14-15, material.scm:15-22,
 * texture.scm:9-10).  Scheme closures are opaque to C, so the drop-in keeps
 * the reference's *constructor* names and arities and has each constructor
 * append a typed descriptor to a scene builder.
 *
 * Conventions
 *   - every entry point returns an int status: 0 = ok, nonzero = error, with
 *     a thread-local message from rt_last_error();
 *   - handles (contexts, scenes, object/material/texture ids) are ints;
 *   - the caller owns every host buffer; the library copies descriptors at
 *     commit time and owns all device memory it allocates;
 *   - vectors are `const double v[3]` (the reference's f64vector vec3,
 *     vec.scm:7);
 *   - one host thread per context (the reference renders on one thread,
 *     main.scm:633-634); multi-GPU = one process per GPU.
 *   - arithmetic is f64 throughout, as in the reference (Gauche flonums).
 */
#ifndef RTAMD_RT_H
#define RTAMD_RT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 7

/* Sky functions (scene slot 4, geometry.scm:30-31).  The reference stores an
 * arbitrary closure; the two it defines are sky-color (main.scm:91-95) and
 * black (main.scm:97-98). */
enum { RT_SKY_GRADIENT = 0, RT_SKY_BLACK = 1 };

/* Axis-aligned rect planes (geometry.scm:376-431). */
enum { RT_RECT_XY = 0, RT_RECT_XZ = 1, RT_RECT_YZ = 2 };

/* Number of doubles in a camera vector: the reference's 10-slot camera
 * (camera.scm:33-78) flattened = llc(3) horizontal(3) vertical(3) origin(3)
 * w(3) u(3) v(3) lens-radius time0 time1. */
#define RT_CAMERA_DOUBLES 24

/* ---- library / context ------------------------------------------------ */
int rt_abi_version(void);
const char* rt_last_error(void);
int rt_device_count(int* out_count);
/* Context on one HIP device; owns a HIP stream and all device memory.
 * The render lanes' path pools belong to the context and are shared by every
 * scene rendered on it.  They are sized at the context's first render to
 * hold up to 384Mi paths, but at most 65 % of the device memory free at that
 * moment (RT_OPT_MAX_PATHS overrides), and are kept for later renders;
 * rt_context_release_pools frees them (the next render sizes them again),
 * e.g. before the caller allocates large buffers of its own. */
int rt_context_create(int device, int* out_ctx);
int rt_context_destroy(int ctx);
int rt_context_release_pools(int ctx);

/* Render-schedule options of a context (every scene rendered on it).  Value 0
 * = the library's automatic choice (the default); negative values are refused.
 * None of them changes an image: renders are bit-identical for any lane count,
 * pool size and tail threshold (per-sample counter RNG, sample-ordered
 * accumulation).
 *   RT_OPT_LANES      render lanes (path pool + stream) kept in flight, 1..4;
 *                     auto = 2, or 1 for scenes whose world BVH holds curves
 *                     (the persistent curve kernel fills the chip by itself);
 *                     raising it above the lanes the pools were sized for
 *                     sizes them again at the next render, lowering it keeps
 *                     the pools as they are (each lane then holds the smaller
 *                     per-lane share of the larger count; RT_OPT_MAX_PATHS or
 *                     rt_context_release_pools resizes them)
 *   RT_OPT_MAX_PATHS  paths per pool (chunk of samples), >= 1024; auto = 384Mi,
 *                     at most 65 % of free device memory for the lanes together
 *                     (setting it makes the next render size the pools again)
 *   RT_OPT_TAIL_PATHS a chunk with at most max(TAIL_PATHS, B / TAIL_DIV) live
 *   RT_OPT_TAIL_DIV   paths (B = the chunk's camera samples) finishes in the
 *                     persistent tail kernel; with neither set the threshold
 *                     follows the render: one chunk max(32768,
 *                     min(B / 4, 524288), B / 256), else
 *                     max(32768, min(B / 64, 262144), B / 256) (curve-kernel
 *                     scenes: max(32768, B / 256)); either set: the other's
 *                     auto value is 32768 / 256
 *   RT_OPT_TAIL_OFF   nonzero: no tail kernel, every depth in the wavefront
 *                     kernels (tests and A/B runs)
 * One option selects arithmetic, not the schedule:
 *   RT_OPT_EXACT_LIBM the sin / cos of the lambertian bounce directions
 *                     (random-cosine-direction, util.scm:37-44, and the light
 *                     mixture's sphere sampler): RT_LIBM_EXACT = the reference
 *                     runtime's C library bit for bit (glibc's algorithm,
 *                     restated on the device), RT_LIBM_DEVICE = the device
 *                     library (within 1 ulp, ~1.4 % faster on the cover scene),
 *                     RT_LIBM_AUTO (0) = exact in scenes with curves (where an
 *                     ulp of a bounce direction changes which ribbon a grazing
 *                     ray hits) or noise / marble textures (C3: 0.8 % of the
 *                     horizon rows' pixels moved by > 1e-9 otherwise; exact
 *                     costs it 1.7 %), the device library elsewhere (the cover
 *                     scene: 0.3 % of those pixels, exact would cost 1.4 %).
 *                     The marble texture's sin is exact in every mode. */
enum { RT_OPT_LANES = 1, RT_OPT_MAX_PATHS = 2, RT_OPT_TAIL_PATHS = 3, RT_OPT_TAIL_DIV = 4, RT_OPT_TAIL_OFF = 5,
       RT_OPT_EXACT_LIBM = 6 };
enum { RT_LIBM_AUTO = 0, RT_LIBM_EXACT = 1, RT_LIBM_DEVICE = 2 };
int rt_context_set_option(int ctx, int option, int64_t value);
int rt_context_get_option(int ctx, int option, int64_t* out_value);

/* ---- scene building (replaces the closure-vector constructors) ---------- */
int rt_scene_begin(int ctx, int* out_scene);
int rt_scene_destroy(int scene);

/* textures — texture.scm:12-34 */
int rt_add_texture_constant(int scene, const double rgb[3], int* out_tex);     /* t:constant-texture :12 */
int rt_add_texture_checker(int scene, int even_tex, int odd_tex, int* out_tex); /* t:checker-texture :16 */
int rt_add_texture_noise(int scene, double scale, int* out_tex);               /* t:noise-texture :25 */
int rt_add_texture_marble(int scene, double scale, int* out_tex);              /* t:marble-texture :30 */

/* materials — material.scm:24-111 */
int rt_add_material_lambertian(int scene, int albedo_tex, int* out_mat);            /* m:make-lambertian :24 */
int rt_add_material_metal(int scene, int albedo_tex, double fuzz, int* out_mat);    /* m:make-metal :45 */
int rt_add_material_dielectric(int scene, double ref_idx, int* out_mat);            /* m:make-dielectric :76 */
int rt_add_material_diffuse_light(int scene, int emit_tex, int* out_mat);           /* m:make-diffuse-light :103 */

/* hitables — geometry.scm / bezier.scm.  Objects may be shared and nested. */
int rt_add_sphere(int scene, const double center[3], double radius, int mat, int* out_obj);   /* g:make-sphere :146 */
int rt_add_moving_sphere(int scene, const double center0[3], const double center1[3],
                         double time0, double time1, double radius, int mat, int* out_obj);     /* g:make-moving-sphere :177 */
/* axis: RT_RECT_XY (a=x,b=y,k=z), RT_RECT_XZ (a=x,b=z,k=y), RT_RECT_YZ (a=y,b=z,k=x) */
int rt_add_rect(int scene, int axis, double a0, double a1, double b0, double b1, double k,
                int mat, int* out_obj);                                                          /* g:make-{xy,xz,yz}-rect :376-431 */
/* cubic Bezier curve a,b,c,d of the given width (b:make-bezier bezier.scm:61); hit t is the distance
 * along unit(dir) and the normal is -dir (bezier.scm:176-214).  width: positive and finite (for width
 * <= 0 the reference's depth estimate takes the log of a number <= 0 and raises on the first hit test) */
int rt_add_bezier(int scene, const double a[3], const double b[3], const double c[3], const double d[3],
                  double width, int mat, int* out_obj);
/* n curves at once (bezier->objs points.scm:45-53 over points->bezier output): cps holds n*12 doubles
 * (a,b,c,d per curve); the curves get the consecutive object ids *out_first .. *out_first + n - 1 */
int rt_add_bezier_array(int scene, const double* cps, int n, double width, int mat, int* out_first);
int rt_add_flip_normals(int scene, int obj, int* out_obj);                                       /* g:flip-normals :433 */
/* g:make-constant-medium boundary density a (geometry.scm:545): a volume of the given density inside
 * `boundary` (spheres / rects / boxes / instances); the phase function is a lambertian material with
 * texture albedo_tex, created by this call.  Its hit test draws one random number (like the reference),
 * so media are evaluated in object-list order relative to the objects before them. */
int rt_add_constant_medium(int scene, int boundary, double density, int albedo_tex, int* out_obj);
/* g:make-klein center mat (geometry.scm:645): Kleinian limit set, sphere traced (no bounding box) */
int rt_add_klein(int scene, const double center[3], int mat, int* out_obj);
int rt_add_box(int scene, const double p0[3], const double p1[3], int mat, int* out_obj);       /* g:make-box :444 */
int rt_add_translate(int scene, int obj, const double offset[3], int* out_obj);                 /* g:translate :465 */
int rt_add_rotate_y(int scene, int obj, double angle_deg, int* out_obj);                        /* g:rotate-y :483 */
/* An object list (make-scene's obj-list, geometry.scm:52; a nested list). */
int rt_add_list(int scene, const int* objs, int n, int* out_obj);
/* g:make-bvh-node :226 / g:make-bvh-with-sah :294.  Closest-hit over the children, which are flattened into
 * the world's list like any nested list: the node itself builds nothing.  At rt_scene_commit the library
 * builds one tree of its own over leaves of the whole world (whether or not they were under an rt_add_bvh):
 *   - world-level spheres and moving spheres (under no rt_add_translate / rt_add_rotate_y) listed before the
 *     first constant medium, when there are at least RTAMD_BVH_MIN of them (environment, default 16), and
 *     world-level curves with them;
 *   - with RT_HAS_GENERIC_BVH, also rects (box faces included) under any instance chain or none, and spheres
 *     and moving spheres under an instance chain, whose world-space box is finite — when the scene has at
 *     least RTAMD_BVH_GENERIC_MIN such leaves (environment, read at commit; default 48) and
 *     holds no curve, no constant medium (so no medium boundary) and no Klein set.  Rects under more than 16
 *     distinct rotations: the rects of the 17th rotation on stay outside the tree.
 *   - with RT_HAS_MEDIA_BVH, a scene with constant media and no curve and no Klein set is a media forest
 *      when some segment of its list (the leaves between two media, a medium closing its
 *     segment) has at least RTAMD_BVH_GENERIC_MIN such leaves.  Each segment is then decided on its own by the
 *     two rules above over its own counts and gets a tree of its own, the first 8 segments that qualify;
 *     rt_tree_info.segments / segment_trees report it.  Medium boundaries stay outside every tree.
 *     Every other scene with a curve, a medium or a Klein set is committed exactly as without
 *     RT_HAS_GENERIC_BVH.
 * Every other leaf is tested one by one for every ray segment, grouped by instance chain and type
 * (rt_tree_info.group_leaves counts them).  Whatever the tree takes, the closest hit is hit-obj-list's
 * (geometry.scm:33-50) over the flattened list, ties at one t included. */
int rt_add_bvh(int scene, const int* objs, int n, double time0, double time1, int sah, int* out_obj);

/* ---- triangles (an extension: the reference has none) --------------------
 * Opt-in: nothing above changes.  RT_ABI_VERSION stays 7; test RT_HAS_TRIANGLES for these entry points.
 *
 * rt_add_triangle: the triangle v0 v1 v2 with material mat, two-sided.
 * rt_add_mesh: nf triangles over nv vertices (verts = nv x {x, y, z}; faces = nf x 3 vertex indices; uv =
 * nv x {u, v} texture coordinates, or NULL: the hit records' u = v = 0).  *out_obj = one list object over the
 * triangles, in face order, so the mesh can go under rt_add_translate / rt_add_rotate_y / rt_add_flip_normals /
 * rt_add_bvh like any object.
 * Refused by the add call: a null pointer (uv excepted), nv < 1 or nf < 1, a vertex or a texture coordinate
 * of a face that is not finite, a face index outside 0 .. nv - 1, a triangle whose cross(v1 - v0, v2 - v0) has
 * zero or non-finite length (the message names the face), an invalid material, a committed scene.  The
 * arguments are checked before the scene handle, and a refused mesh leaves the scene as it was.
 * Refused by rt_scene_commit: a triangle in a scene with a curve, a Klein set or a constant
 * medium; a triangle in a medium's boundary or as the light-sampling target; a triangle whose instance chain
 * leaves it no finite world-space box.
 *
 * The tree.  A scene with a triangle always gets the world tree of RT_HAS_GENERIC_BVH (rt_add_bvh above),
 * whatever RTAMD_BVH_MIN and RTAMD_BVH_GENERIC_MIN say: every triangle is a leaf of it (its box: the box of
 * its three vertices taken out of its instance chain), and every other leaf that qualifies with them.
 * rt_tree_info.tri_leaves counts them.  Such a scene walks device memory only (rt_hit_rays_walk refuses the
 * LDS walks).
 *
 * The hit test is the watertight test of Woop, Benthin and Wald (2013): an edge shared by two triangles gets
 * the same edge value, with opposite sign, from both, so no ray slips between them.  All arithmetic is IEEE
 * f64 in exactly this order, no operation contracted into an FMA.  On the instance-local ray (o, d), i.e. the
 * ray taken into the triangle's instance chain (translate: o - offset; rotate-y: (c x - s z, y, s x + c z) on
 * o and d, outermost first), with v[k] the k-th component (0 x, 1 y, 2 z):
 *     kz = 0;  if |d[1]| > |d[kz]| kz = 1;  if |d[2]| > |d[kz]| kz = 2
 *     kx = (kz + 1) % 3;  ky = (kx + 1) % 3;  if d[kz] < 0 swap(kx, ky)
 *     Sx = d[kx] / d[kz];  Sy = d[ky] / d[kz];  Sz = 1.0 / d[kz]
 *     A = v0 - o;  B = v1 - o;  C = v2 - o                      (componentwise)
 *     Ax = A[kx] - Sx * A[kz];  Ay = A[ky] - Sy * A[kz]          (Bx, By, Cx, Cy alike)
 *     U = Cx * By - Cy * Bx;  V = Ax * Cy - Ay * Cx;  W = Bx * Ay - By * Ax
 *     miss if (U < 0 || V < 0 || W < 0) && (U > 0 || V > 0 || W > 0)
 *     det = (U + V) + W;  miss if det == 0
 *     T = (U * (Sz * A[kz]) + V * (Sz * B[kz])) + W * (Sz * C[kz]);  t = T / det
 *     hit iff 0.001 < t && t < closest
 * Both sides are hit; edges and vertices are inclusive.  The comparisons are written so that a NaN passes
 * none: a ray in the triangle's plane (det == 0, or 0/0) and a ray with a component that is not finite miss.
 * Ties.  A triangle ties like a sphere: of the leaves of the flattened list at the smallest t the last rect
 * wins, and if none of them is a rect, the first leaf in list order.
 *
 * The hit record.  With dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z and cross(a, b) = (a.y b.z - a.z b.y,
 * a.z b.x - a.x b.z, a.x b.y - a.y b.x):
 *   - the point is o + d * t on the instance-local ray, as for every leaf;
 *   - the normal is the geometric one, formed once at the commit: e1 = v1 - v0, e2 = v2 - v0, n = cross(e1, e2),
 *     normal = n * (1.0 / sqrt(dot(n, n))).  rt_add_flip_normals negates it; the instance chain takes point and
 *     normal back out as for rects.  A mesh with vertex normals replaces it (shading normals, below);
 *   - u, v (read by image textures only): with texture coordinates (u0, v0), (u1, v1), (u2, v2) of the vertices,
 *     w = pt - v0, b1 = dot(cross(w, e2), n) / dot(n, n), b2 = dot(cross(e1, w), n) / dot(n, n),
 *     b0 = (1.0 - b1) - b2, u = (b0 * u0 + b1 * u1) + b2 * u2, and v alike.  Without texture coordinates
 *     u = v = 0, as for curves.
 *
 * Shading normals (RT_HAS_SMOOTH_NORMALS).  rt_add_mesh_normals is rt_add_mesh with one normal per vertex
 * (normals = nv x {x, y, z}); with normals = NULL it is rt_add_mesh, bit for bit.  At the add call each normal
 * is made unit: nk = n * (1.0 / sqrt(dot(n, n))).  Refused there, as rt_add_mesh refuses (before the handle
 * is looked at, the scene left as it was, the message naming the face): a normal of a face's vertex that is not
 * finite, or whose length is zero or not finite.
 * For a hit at the local point pt on a triangle with unit vertex normals n0, n1, n2, componentwise and in IEEE
 * f64 in exactly this order, no operation contracted into an FMA:
 *     w = pt - v0;  b1 = dot(cross(w, e2), n) / dot(n, n);  b2 = dot(cross(e1, w), n) / dot(n, n)
 *                                                    (the barycentrics of u, v above: formed once per record)
 *     s = (n0 + (n1 - n0) * b1) + (n2 - n0) * b2
 *     q = dot(s, s)
 *     normal = s * (1.0 / sqrt(q)) if q > 0 and q is finite, else the geometric normal
 * The difference form gives n0 back exactly where the three normals are equal.  The shading normal replaces the
 * geometric normal in the hit record and nowhere else: the hit test, the leaf boxes, the ties and a triangle
 * light's density and area (light lists, below) keep the geometric triangle.  rt_add_flip_normals negates the
 * shading normal and the instance chain takes it out as it takes any normal out; it is neither renormalised
 * nor turned to face the ray: the vertex normals say which side is outside, as the winding does for a flat
 * triangle.  Two consequences: a diffuse_light emits on the shading normal's side (dot(normal, d) < 0), which
 * near a silhouette is not the geometric side; and a lambertian bounce, drawn about the shading normal, may
 * start below the geometric surface (and then hits the mesh again from inside, or leaves through it).
 * rt_add_triangle has no normals argument.
 * rtamd.mesh restates all of this in NumPy (hit, normal, uv, shading_normal). */
#define RT_HAS_TRIANGLES 1
#define RT_HAS_SMOOTH_NORMALS 1
int rt_add_triangle(int scene, const double v0[3], const double v1[3], const double v2[3], int mat, int* out_obj);
int rt_add_mesh(int scene, const double* verts, int nv, const int32_t* faces, int nf, const double* uv, int mat,
                int* out_obj);
int rt_add_mesh_normals(int scene, const double* verts, int nv, const int32_t* faces, int nf, const double* uv,
                        const double* normals /* nv x 3, nullable */, int mat, int* out_obj);

/* camera — cam:make-camera (camera.scm:63-78) evaluated on the host side;
 * the 24 doubles are the 10 slots the reference's get-ray reads. */
int rt_make_camera(const double lookfrom[3], const double lookat[3], const double vup[3],
                   double vfov_deg, double aspect, double aperture, double focus_dist,
                   double time0, double time1, double out_cam[RT_CAMERA_DOUBLES]);
int rt_set_camera(int scene, const double cam[RT_CAMERA_DOUBLES]);
/* Extension (pdf.scm:18-41): lambertian bounces sample the mixture of
 * (hitable-pdf light p) and (cosine-pdf normal), with g:pdf-value / g:random defined for an axis rect
 * or a sphere as in "The Rest of Your Life".  light_obj = a rect or sphere object (flips allowed),
 * -1 = off (the reference's own cosine sampling).  The reference never wires pdf.scm, so this path
 * is checked against the oracle's restatement only. */
int rt_set_light_sampling(int scene, int light_obj);
/* ---- light lists (an extension of the extension: "The Rest of Your Life" gives a list of hitables a pdf) ----
 * Opt-in: nothing above changes.  RT_ABI_VERSION stays 7; test RT_HAS_LIGHT_LIST for these entry points.
 *
 * rt_set_light_list: the lambertian bounces' mixture samples a list of lights instead of one.
 * Flattening.  Each objs[k] is a rect, a sphere, a triangle, an rt_add_flip_normals of one of these, or a list
 * of such: an rt_add_list or the object rt_add_mesh returns, nested to any depth.  They flatten in order to m
 * lights L_0 .. L_{m-1}, 1 <= m <= RT_MAX_LIGHTS.  n == 0 turns sampling off.  A light need not be a member of
 * the world list.  A flip does not change sampling (the densities use |cosine|).  rt_set_light_list and
 * rt_set_light_sampling each replace the other's setting: the last call wins.
 * Refused by the call, with a message and the scene left as it was: a box, a moving sphere, a translate, a
 * rotate-y, an rt_add_bvh, a curve, a medium or a Klein set anywhere in the list; a bad id; m = 0 from a
 * non-empty objs; m > RT_MAX_LIGHTS; a null objs with n > 0; n < 0; a committed scene.  (rt_scene_commit keeps
 * refusing a triangle handed to rt_set_light_sampling.)
 *
 * The densities.  All arithmetic is IEEE f64 in exactly this order, no operation contracted into an FMA;
 * next() is the path's stream; dot and cross as in the triangle section.
 *   pdf_value(o, v):  w = 1.0 / (double)m;  s = 0.0;  for i = 0 .. m-1: s = s + w * pdf_i(o, v)
 *   random(o):        if m > 1: r = next(); i = (int)(r * (double)m); if (i > m - 1) i = m - 1
 *                     if m == 1: no draw, i = 0
 *                     then random_i(o)
 * A list of one light is that light (the book's hitable_list::random always draws; this one does not): with
 * it rt_set_light_list(&obj, 1) on a rect or sphere commits and renders exactly as rt_set_light_sampling(obj),
 * bit for bit.  The index clamp keeps the record read in range.
 *   rect, sphere:  pdf_i and random_i are rt_set_light_sampling's (the sphere sampler evaluates
 *                  random-to-sphere three times, 6 draws, with the libm mode of the render: RT_OPT_EXACT_LIBM).
 *   triangle pdf_i(o, v):  the watertight test of the triangle section on the ray (o, v) with
 *                  closest = 999999999999; a miss gives 0; a hit at t gives distance_squared / (cosine * area),
 *                  distance_squared = (t * t) * dot(v, v), cosine = fabs(dot(v, nu) / sqrt(dot(v, v))),
 *                  area = 0.5 * sqrt(dot(n, n)) with n = cross(v1 - v0, v2 - v0), nu the unit normal as the
 *                  hit record's (n * (1.0 / sqrt(dot(n, n)))); area and nu are formed once at the commit.
 *   triangle random_i(o):  r1 = next(); r2 = next(); su = sqrt(r1); b1 = su * (1.0 - r2); b2 = su * r2;
 *                  pnt = v0 + (e1 * b1 + e2 * b2) componentwise, e1 = v1 - v0, e2 = v2 - v0; the result is pnt - o.
 * The mixture is rt_set_light_sampling's: the choice draw first, 0.5 * pdf_value + 0.5 * cosine density, and
 * !(pdf > 0) ends the path.  The light loop has the fixed trip count m: no new waiting loop, no new fault bit.
 *
 * rt_light_probe (a test probe, as rt_hit_rays_stream is one): for point k, on the stream of (seed, pixel k,
 * sample 0) from its first number: out_dir = random(point), out_pdf = pdf_value(point, out_dir),
 * out_pdf_dirs = pdf_value(point, dirs[k]) (dirs and out_pdf_dirs nullable together), out_draws = the numbers
 * consumed.  For a single light and for a list, through the device functions the shading uses; the sphere
 * sampler takes the libm mode the scene's renders take.  Refused before any device work: a scene without light
 * sampling, a scene not committed, null or negative arguments.
 * rtamd.lights restates all of this in NumPy. */
#define RT_HAS_LIGHT_LIST 1
#define RT_MAX_LIGHTS 4096
int rt_set_light_list(int scene, const int* objs, int n);
int rt_light_probe(int scene, int n, const double* points /* n x 3 */, const double* dirs /* n x 3, nullable */,
                   uint64_t seed, double* out_dir /* n x 3 */, double* out_pdf /* n */,
                   double* out_pdf_dirs /* n, nullable with dirs */, int32_t* out_draws /* n */);
int rt_set_sky(int scene, int sky);
/* Perlin tables (perlin.scm:32-36): the reference draws them from the global
 * RNG at module load; here they are data.  ranvec: 256 unit vec3, perm: 256
 * entries each (a permutation of 0..255). */
int rt_set_perlin_tables(int scene, const double ranvec[256 * 3], const int32_t perm_x[256],
                         const int32_t perm_y[256], const int32_t perm_z[256]);
/* Fix the world (make-scene's obj-list) and upload the scene to the device. */
int rt_scene_commit(int scene, int world_list_obj);

/* ---- rendering -------------------------------------------------------- */
/* One call = `spp_count` successive trace-all passes (main.scm:471-491) with
 * pass indices spp_begin+1 .. spp_begin+spp_count: for every pixel j = y*nx+x
 * (y = 0 is the bottom row) the per-sample colours are added to accum[3j..3j+2]
 * in sample order, exactly the `*raw-data*` running sum.  Random numbers come
 * from a counter-based stream keyed by (seed, pixel, sample), so results do
 * not depend on launch geometry, batching or sharding.
 *
 * rt_render: accum is a caller-owned HOST buffer (nx*ny*3 doubles), copied to
 * the device and back (PCIe-inclusive).
 * rt_render_device: accum is caller-owned DEVICE memory on the context's GPU
 * (e.g. a torch tensor's data_ptr); stream is a hipStream_t or NULL for the
 * context's own stream.  shard_index/shard_count select an interleaved subset
 * of 16x16 pixel tiles (tile (tx, ty) belongs to shard (tx + k ty) % shard_count, k the
 * smallest odd prime that does not divide shard_count: 3, or 5 for 3, 6, 9, ... shards);
 * pixels of other shards are left untouched. */
int rt_render(int scene, int nx, int ny, int spp_begin, int spp_count, uint64_t seed,
              double* accum_host);
int rt_render_device(int scene, int nx, int ny, int spp_begin, int spp_count, uint64_t seed,
                     int shard_index, int shard_count, double* accum_device, void* stream);

/* Rows [y_begin, y_begin + y_count) only (same pass semantics as rt_render): the
 * band of the frame trace-line (main.scm:452-469) renders one row of.  accum is
 * the whole nx*ny*3 frame; only the band's entries are read or written (the
 * host version copies only the band across PCIe). */
int rt_render_rows(int scene, int nx, int ny, int y_begin, int y_count, int spp_begin, int spp_count,
                   uint64_t seed, double* accum_host);
int rt_render_rows_device(int scene, int nx, int ny, int y_begin, int y_count, int spp_begin, int spp_count,
                          uint64_t seed, double* accum_device, void* stream);
/* trace-line (main.scm:452-469), as animate calls it (main.scm:533-544): add
 * sample number `sample_count` (1-based) of every pixel of row y to raw_data
 * (the *raw-data* running sum, nx*ny*3 doubles, y-up rows) and re-resolve row
 * y of image (*image*, nx*ny*3 bytes) with sqrt(sum/sample_count).  Host
 * buffers, caller-owned.  A frame done row by row equals the trace-all pass
 * with the same sample_count bit for bit. */
int rt_trace_line(int scene, int nx, int ny, int y, int sample_count, uint64_t seed, double* raw_data,
                  uint8_t* image);
/* One shard's tiles (as rt_render_device's shard arguments) into a COMPACT
 * accumulator: accum_compact[3q..3q+2] is the running sum of pixel
 * rt_shard_pixels(...)[q], so a rank holds and ships only its own pixels
 * (multi-GPU gather, bench.py / rtamd.dist). */
int rt_render_shard_device(int scene, int nx, int ny, int spp_begin, int spp_count, uint64_t seed,
                           int shard_index, int shard_count, double* accum_compact, void* stream);

/* The pixels shard `shard_index` of `shard_count` renders (host-only, no GPU
 * needed): interleaved 16x16 tiles in row-major tile order, tile (tx, ty)
 * belongs to shard (tx + k ty) % shard_count, k = the smallest odd prime not
 * dividing shard_count (diagonal and coprime, so no shard gets whole columns
 * or only some residues of them); pixel j = y*nx + x, listed tile by tile.
 * Pass out_pix = NULL to get the count only. */
int rt_shard_pixels(int nx, int ny, int shard_index, int shard_count, uint32_t* out_pix, int64_t* out_count);

/* ---- multi-GPU frame (one process per GPU) ----------------
 * Each rank renders its tiles with rt_render_shard_device into a compact
 * accumulator; at frame end rt_gather_shards moves every rank's accumulator to
 * rank 0 over RCCL (xGMI between the GPUs of a node) and places the pixels into
 * rank 0's y-up frame.  Replaces nothing in the reference, which renders on one
 * thread (main.scm:471-491, 633-634): it is the frame's only exchange step.
 *
 * rt_comm_unique_id: rank 0 makes the communicator's id (ncclGetUniqueId); the
 *   host program ships the RT_COMM_ID_BYTES bytes to the other ranks (e.g.
 *   over its own process group or a file).
 * rt_comm_create: every rank, with the same id, its rank and the world size;
 *   collective (returns once all ranks have called it).  The communicator
 *   runs on the context's device.
 * rt_gather_shards: every rank, collective.  accum_compact = the rank's
 *   compact accumulator (device, 3 doubles per pixel of
 *   rt_shard_pixels(nx, ny, rank, world)); frame_device = rank 0's nx*ny*3
 *   frame (device; NULL on other ranks), whose pixels of every shard are
 *   overwritten.  Enqueued on `stream` (NULL: the context's stream), which the
 *   call synchronises before it returns.  The frame equals a one-process
 *   rt_render_device of the same passes bit for bit (disjoint pixels, nothing
 *   is summed).  The communicator stays valid through the call even if another
 *   thread destroys its handle; its context must outlive the call.
 * rt_gather_layout: host-only (no GPU, no RCCL): for each rank r of `world`,
 *   out_count[r] = its shard's pixel count and out_offset[r] = the offset of
 *   its pixels in the ranks' concatenated rt_shard_pixels lists (out_offset[0]
 *   = 0).  Rank 0 receives rank r's compact accumulator at doubles
 *   3 * (out_offset[r] - out_count[0]) of its receive buffer.
 * rt_gather_shards_local: the same gather within one process (every shard of
 *   `world` on the context's device, e.g. several shards rendered by one
 *   GPU): accum_compact = a host array of `world` device pointers, shard r's
 *   compact accumulator in entry r; the same receive layout and placement as
 *   rt_gather_shards, with device copies in place of the sends and receives. */
#define RT_COMM_ID_BYTES 128
int rt_comm_unique_id(uint8_t out_id[RT_COMM_ID_BYTES]);
int rt_comm_create(int ctx, const uint8_t unique_id[RT_COMM_ID_BYTES], int rank, int world, int* out_comm);
int rt_comm_destroy(int comm);
int rt_gather_shards(int comm, int nx, int ny, const double* accum_compact, double* frame_device, void* stream);
int rt_gather_layout(int nx, int ny, int world, int64_t* out_count, int64_t* out_offset);
int rt_gather_shards_local(int ctx, int nx, int ny, int world, const double* const* accum_compact,
                           double* frame_device, void* stream);

/* Errors raised on the device.  Every loop of the kernels that waits on data
 * (rejection samplers, curve subdivision walks, persistent kernels' per-path
 * loops) has an iteration cap a valid random stream cannot reach, and queue
 * appends never pass their shard's capacity: a kernel that would instead sets
 * one of these bits and leaves the loop, and the render call fails with
 * rt_last_error() naming them ("device fault (flags N): ..."). */
enum { RT_FAULT_REJECT = 1, RT_FAULT_CURVE = 2, RT_FAULT_PATH = 4, RT_FAULT_SHARD = 8, RT_FAULT_LDS = 16 };

/* The world's closest hit for n rays (hit-obj-list over the scene list,
 * geometry.scm:33-50, with t in (0.001, 999999999999) as color asks it,
 * main.scm:104): rays = n x {ox, oy, oz, dx, dy, dz, time} (host memory);
 * out_t[i] = the hit's t and out_mat[i] = its material id (rt_add_material_*),
 * or out_mat[i] = -1 (and t 0) for a miss.  A diagnostic and test probe (the
 * oracle's orc_hit_world); scenes with constant media are refused, since the
 * medium's hit test draws from the path's random stream. */
int rt_hit_rays(int scene, int n, const double* rays, double* out_t, int32_t* out_mat);

/* rt_hit_rays through a chosen closest-hit walk (a test probe: the renders pick their walks themselves).
 * RT_WALK_HBM: the trees in device memory, 32-bit traversal stacks (rt_hit_rays is this walk).
 * RT_WALK_LDS_TIME0: k_extend_lds's query, which every scattered ray takes in scenes whose time-0 tree
 *   runs from LDS: that tree staged in LDS, 16-bit stacks, sign-selected slabs, leafless when the world is
 *   one BVH (rt_scene_info.bvh_solo).  Every ray's time must be +0.0 bit for bit (the kernel never sees
 *   another); refused when rt_scene_info.extend_lds_bytes is 0.
 * RT_WALK_LDS_CAMERA: k_camera's query, which camera rays take: the all-times tree in LDS when the scene
 *   has moving spheres (rt_scene_info.tree0_any_time 0), else the time-0 tree; the ray's own time; refused
 *   when rt_scene_info.camera_lds_bytes is 0.
 * Rays, outputs and the refusal of scenes with media as rt_hit_rays. */
enum { RT_WALK_HBM = 0, RT_WALK_LDS_TIME0 = 1, RT_WALK_LDS_CAMERA = 2 };
int rt_hit_rays_walk(int scene, int walk, int n, const double* rays, double* out_t, int32_t* out_mat);

/* rt_hit_rays with the path's random stream (RT_HAS_MEDIA_BVH; a test probe): the same rays through the same
 * closest hit in device memory, ray k drawing from the stream of (seed, pixel k, sample 0) from its first
 * number on, as a render's paths do; out_draws[k] = how many random numbers the query consumed (a constant
 * medium draws one whenever the closest hit so far leaves part of its span).  Accepts every scene rt_hit_rays
 * accepts and scenes with constant media. */
int rt_hit_rays_stream(int scene, const double* rays, int n, uint64_t seed, double* out_t, int32_t* out_mat,
                       int32_t* out_draws);

/* ---- one wavefront iteration on a caller's path states (RT_HAS_STEP_PROBE; a test probe) ---------------
 * rt_step_rays builds the path state of n paths, runs ONE iteration of the render's wavefront on it through
 * the render's own launchers, and reads everything back.  Opt-in: nothing above changes, RT_ABI_VERSION
 * stays 7; test RT_HAS_STEP_PROBE.
 *
 * Record k (host memory): rays[7k..] = {ox, oy, oz, dx, dy, dz, time}, T_in[3k..] its throughput, ctr_in[k]
 * its draw counter, pix[k] its pixel key (pix null: pix[k] = k).  Record k draws from the Philox stream of
 * (seed, pix[k], smp) from draw ctr_in[k] on (the oracle's orc_step with the same numbers).
 *
 * The state.  depth 0: the raygen layout (ray, time, counter; slot k = work id k, contiguous); the
 * throughput of a depth-0 path is 1 by construction, so any other T_in is refused.  depth >= 1: the
 * survivor layout a shade kernel leaves behind, PathRec{T, wid = k, rng} in the 8 sharded queues (record k
 * in shard (k / 256) % 8, the shards' counts in the previous iteration's counter row) with shard capacity,
 * counter rows and hit-queue strides computed as a render of n paths computes them; a scattered ray has time
 * +0.0, so any other time is refused.  RenderParams: npix = n, pixlist = pix, spp0 = smp, B = n, the libm
 * mode the scene's renders take (RT_OPT_EXACT_LIBM).  The sample buffer is pre-filled with the NaN pattern
 * 0x7FF8DEAD5CA77E12 in every double (RT_STEP_SENTINEL): a slot that still holds it was not written.
 *
 * extend: RT_STEP_EXTEND_HBM = launch_extend (HitRec queues, depth0 = (depth == 0)): k_extend<F>, or, in
 * scenes whose renders take the persistent curve kernel (every curve in the world BVH, no media, no Klein
 * set; RT_HAS_CURVE_STEP), k_extend_curves<0> exactly as a render launches it: the grid launch_extend sizes
 * (RTAMD_CURVE_BLOCKS caps it, 0 selects the per-ray k_extend), render lane 0's regions of the walk's stack
 * overflow area and rings, the claim word among the control words, appends that spill between shards.
 * RT_STEP_EXTEND_LDS = launch_extend_lds (depth >= 1 and rt_scene_info.extend_lds_bytes > 0 only), which
 * queues lambertian hits as point records exactly when a render's would (rt_scene_point_hits).
 * Scenes with media are allowed: the hit test draws, and the shade continues from its counter.
 *
 * mode RT_STEP_STEP: after the extend, launch_shade for every material type of the scene.  Outputs per
 * record k: out_status[k] = (times wid k appears among the survivors) | RT_STEP_WROTE if its sample slot no
 * longer holds the sentinel; out_color[3k..] the slot's three doubles; for a survivor (the last one found)
 * out_ray[6k..] = {o, d}, out_T[3k..], out_ctr[k]; out_t[k] / out_mat[k] = the queued hit's t and material
 * id, out_mat -1 (t 0) for a record in no hit queue, t NaN for a point record (it carries no t).
 * *out_survivors = the sum of the device's survivor counters.  out_inst[8m..8m+5] for material type m =
 * {launched, TL, LS, LL, EX, PT} of the k_shade instance launch_shade took (all 0 when the scene has no such
 * material).  out_inst[7] = the extend launch_extend took (RT_STEP_EXTEND_HBM; RT_HAS_CURVE_STEP): 0 k_extend<F>,
 * 1 k_extend_curves<0>, 2 / 3 k_extend_curves<FUSE> with the device / the exact libm (RT_STEP_FUSED only).
 * mode RT_STEP_TAIL: launch_finish on the same state at `depth` instead of extend + shade; out_color /
 * out_status as above (no survivors), out_inst[0..5] = {1, F, TL, LS, SOLO, EX} of the k_finish instance;
 * the other outputs are left alone.  Curve-kernel scenes are taken like any other.
 * mode RT_STEP_FUSED (RT_HAS_CURVE_STEP): the iteration as a render enqueues it at depth >= 1 in a scene whose
 * depth >= 1 launches take the fused curve extend: k_extend_curves<FUSE> runs every record to its end and
 * shades the hits itself.  out_color / out_status as for RT_STEP_TAIL (no survivors), out_inst[7] = 2 or 3,
 * *out_survivors = the continuation segments the launch counted (every closest-hit query past each record's
 * first); the other outputs are left alone.
 * The instance tuples come from the selection functions launch_shade / launch_finish / launch_extend
 * themselves call.
 *
 * Refused before any device work: null pointers (pix excepted), n < 0, depth outside 0..100, an unknown
 * extend or mode, an uncommitted scene, RT_STEP_EXTEND_LDS at depth 0 or in a scene without that kernel,
 * RT_STEP_FUSED at depth 0, with RT_STEP_EXTEND_LDS, or where a render would not fuse (the error names why: not
 * a curve-kernel scene, Perlin or image textures, a sampled light, RTAMD_CURVE_FUSE=0, RTAMD_CURVE_BLOCKS=0).
 * n = 0 returns at once with *out_survivors = 0 and out_inst cleared. */
#define RT_HAS_STEP_PROBE 1
enum { RT_STEP_EXTEND_HBM = 0, RT_STEP_EXTEND_LDS = 1 };
#define RT_HAS_CURVE_STEP 1
enum { RT_STEP_STEP = 0, RT_STEP_TAIL = 1, RT_STEP_FUSED = 2 };
enum { RT_STEP_WROTE = 256 };
#define RT_STEP_SENTINEL 0x7FF8DEAD5CA77E12ull
int rt_step_rays(int scene, int n, const double* rays, const double* T_in, const uint32_t* ctr_in,
                 const uint32_t* pix /* nullable */, uint64_t seed, uint32_t smp, int depth, int extend, int mode,
                 int32_t* out_status, double* out_color, double* out_ray, double* out_T, uint32_t* out_ctr,
                 double* out_t, int32_t* out_mat, int32_t* out_inst /* 32 */, uint32_t* out_survivors);

/* converge's subdivision depth (bezier.scm:179-193) as the curve kernels compute it (bez_maxd): for n
 * curves given in ray space (cps = n x 12 doubles, the control points after bezier-transform) and 8 eps
 * each (eps = width / 20), out_depth[i] = ceiling((log z) / (log 4)) with z = sqrt(2) n (n-1) l0 / (8 eps),
 * 0 where the log is -inf, saturated at 25 (one past the 24 levels the walk supports; deeper curves fault
 * the render).  A test probe of the device's log against the C library's. */
int rt_curve_depth_probe(int ctx, int n, const double* cps, const double* eps8, int32_t* out_depth);

/* The kernels' lean f64 helpers over an array (a test probe): out[i] = the helper `kind` of in[i].
 * RT_F64_SQRT_MID / RT_F64_RCP_MID: sqrt(x) / 1.0 / x for every x, by the unscaled core sequence where x
 * is finite, positive and in [2^-256, 2^256), else by the plain operation.  RT_F64_SQRT_CORE /
 * RT_F64_RCP_CORE: the core sequence alone, which equals the IEEE result only inside that window. */
enum { RT_F64_SQRT_MID = 0, RT_F64_RCP_MID = 1, RT_F64_SQRT_CORE = 2, RT_F64_RCP_CORE = 3 };
int rt_f64_probe(int ctx, int kind, const double* in, int n, double* out);

/* Statistics of the last render on this scene. */
typedef struct rt_stats {
    uint64_t segments;    /* closest-hit queries issued by the integrator (ray segments) */
    uint64_t paths;       /* camera samples */
    double   ms_total;    /* wall time of the render call */
    double   ms_extend;   /* summed device time of the extend (closest-hit) kernel */
    double   ms_shade;    /* summed device time of the shade kernel */
    uint64_t extend_launches;
    uint64_t extend_rays; /* segments the extend kernels traced (the wavefront launches and the fused curve extend; the rest ran in the tail kernel) */
    uint32_t max_depth_seen;  /* deepest wavefront iteration (the tail kernel and the fused curve extend run the deeper ones) */
    uint32_t reserved;
    double   ms_finish;       /* summed device time of the tail kernel */
    uint64_t finish_paths;    /* paths handed to the tail kernel */
    uint64_t shade_hits_d0;   /* camera-ray hits shaded by the wavefront shade kernels */
    uint64_t shade_hits;      /* deeper hits shaded by the wavefront shade kernels */
    uint64_t shade_survivors; /* paths the shade kernels wrote on to the next iteration */
    uint32_t chunks;          /* sample chunks the render was cut into (path pools) */
    uint32_t lanes;           /* render lanes (path pool + stream) kept in flight */
    uint64_t curve_pooled_batches; /* curve subdivision passes over a full survivor pool (wavefront curve kernels) */
    uint64_t curve_flat_pooled;    /* curves those passes walked whose root is a leaf (flat: depth estimate < 0) */
} rt_stats;
int rt_get_stats(int scene, rt_stats* out);

/* What a committed scene became on the device (diagnostics for benchmarks
 * and tests): primitive and tree sizes, and the LDS footprint and resident
 * grid of the persistent LDS kernels (0 = the scene does not use them). */
typedef struct rt_scene_info {
    int32_t  leaves;          /* flattened primitives (leaf records) */
    int32_t  groups;          /* closest-hit groups (a BVH counts as one) */
    int32_t  bvh_nodes;       /* inner nodes of the all-times tree */
    int32_t  bvh0_nodes;      /* inner nodes of the time-0 tree */
    int32_t  tree_depth;      /* deepest tree level (the per-lane traversal stack) */
    int32_t  bvh_solo;        /* 1: the world is exactly one BVH group */
    uint32_t extend_lds_bytes, extend_lds_blocks;   /* k_extend_lds: LDS per block, resident blocks */
    uint32_t camera_lds_bytes, camera_lds_blocks;   /* k_camera: the same */
    int32_t  cus;             /* compute units of the context's device */
    int32_t  curve_stack;     /* curve trees: stack entries the BVH4 walk of k_extend_curves may hold (0: none) */
    double   commit_ms;       /* rt_scene_commit's wall time: flattening, BVH builds (SAH, BVH4 collapse), upload */
    double   commit_upload_ms; /* of it: device allocations and host-to-device copies */
    double   commit_sah_ms;   /* of it: the SAH builds of the world BVH (on commit_threads host threads) */
    int32_t  commit_threads;  /* host threads the SAH builds may use (the process's CPUs, at most 16) */
    int32_t  tree0_any_time;  /* 1: no moving spheres in the world BVH, so its time-0 tree serves rays of every time (was reserved0) */
} rt_scene_info;
int rt_get_scene_info(int scene, rt_scene_info* out);

/* Which leaves of a committed scene the world tree took (rt_add_bvh above).  rt_scene_info keeps its layout;
 * RT_ABI_VERSION stays 7; test RT_HAS_GENERIC_BVH for this entry point.  A scene whose tree holds generic
 * leaves walks it in device memory only: its rt_scene_info reports extend_lds_bytes = camera_lds_bytes = 0
 * and rt_hit_rays_walk refuses the LDS walks. */
typedef struct rt_tree_info {
    int32_t  sphere_leaves;   /* world-level spheres and moving spheres in the tree */
    int32_t  curve_leaves;    /* world-level curves in the tree */
    int32_t  generic_leaves;  /* generic leaves in the tree: rects, and spheres / moving spheres under a chain */
    int32_t  group_leaves;    /* leaves outside the tree, in brute-force groups (constant media included) */
    int32_t  nodes, depth;    /* the all-times tree: inner nodes, deepest level */
    int32_t  nodes0, depth0;  /* the time-0 tree (0, 0: none) */
    int32_t  rot_entries;     /* distinct rotations among the tree rects' chains (no rotation counts as one) */
    int32_t  generic_min;     /* RTAMD_BVH_GENERIC_MIN in force at the commit */
    int32_t  segments;        /* media forests (RT_HAS_MEDIA_BVH): segments of the list, cut after each constant medium; else 0 */
    int32_t  segment_trees;   /* ... and how many of them got a tree; the counts above are then sums / maxima over those trees */
    int32_t  tri_leaves;      /* triangles in the tree (RT_HAS_TRIANGLES; counted in none of the above; was reserved[0]) */
    int32_t  reserved[3];
} rt_tree_info;
#define RT_HAS_GENERIC_BVH 1
#define RT_HAS_MEDIA_BVH 1
int rt_get_tree_info(int scene, rt_tree_info* out);
/* Whether a committed scene's wavefront queues its lambertian hits as point records (the hit
 * point instead of t, so the lambertian shade gathers no ray): *out = 1 when the scene's world is one sphere
 * BVH (rt_scene_info.bvh_solo) whose leaves stand under no rt_add_translate / rt_add_rotate_y, at least one
 * of the persistent LDS kernels runs (extend_lds_bytes or camera_lds_bytes > 0), the scene has no light
 * sampling target and no image texture, and RTAMD_NO_POINT_HITS is not set in the environment (read per
 * render and per call here; set, every queue keeps the t records) — else 0.  Images do not depend on it, bit
 * for bit.  A diagnostic for tests and A/B runs: opt-in, RT_ABI_VERSION stays 7 and rt_scene_info and
 * rt_stats keep their layouts; test RT_HAS_POINT_HITS for this entry point. */
#define RT_HAS_POINT_HITS 1
int rt_scene_point_hits(int scene, int* out);
/* Record per-kernel HIP events during renders (adds a little host overhead). */
int rt_set_profiling(int scene, int enabled);

/* Resolve (main.scm:481-491): c = sqrt(sum/sample_count) per channel, then
 * floor(255.99*min(1,c)) into out (nx*ny*3 bytes, same y-up layout). Host. */
int rt_resolve_u8(const double* accum, int nx, int ny, int sample_count, uint8_t* out);
/* Same on the device (accum_device and out_device are device pointers). */
int rt_resolve_u8_device(int ctx, const double* accum_device, int nx, int ny, int sample_count,
                         uint8_t* out_device, void* stream);

/* ---- adaptive sampling (an extension: the reference declares *max-sample*, main.scm:433, and never
 * uses it; trace-all always does whole-frame passes) -------------------------------------------------
 * Opt-in: nothing above changes.  RT_ABI_VERSION stays 7; test RT_HAS_ADAPTIVE for these entry points.
 *
 * Each pixel j has three records: accum[3j+c], the running sum S_c as above; accum2[3j+c], the running
 * sum Q_c of x*x (the product rounded, then the add rounded, in sample order); count[j], the uint32
 * number of samples taken.  A pixel is *converged* when, in f64, in this operation order, with
 * n = (double)count[j]:
 *
 *     d_c = Q_c - (S_c*S_c)/n            c = 0,1,2
 *     v_c = (d_c < 0 ? 0 : d_c) / (n*(n-1))      a rounding-negative variance clamps to 0, a NaN stays
 *     e2  = (v_0 + v_1) + v_2            the squared standard error of the pixel mean, channels summed
 *     m   = ((S_0 + S_1) + S_2) / n
 *     b   = m > floor ? m : floor
 *     r   = tol*b
 *     converged  <=>  e2 <= r*r
 *
 * A NaN in e2 or r compares false (so does n < 2: 0/0), and such a pixel keeps sampling until max_spp.
 * The library is built without FMA contraction, so the rule is reproducible bit for bit on the host
 * (rtamd.adaptive.converged is the NumPy restatement).
 *
 * rt_render_pixels_device: passes spp_begin .. spp_begin+spp_count-1 of the n pixels listed in
 *   pix_device (device memory) only.  List entries are unique and < nx*ny: the range is checked (a
 *   read-only pass over the list, before any kernel that writes through it is launched; an entry
 *   >= nx*ny fails the call with the buffers untouched), the uniqueness is the caller's responsibility.
 *   Pixels not in the list are neither read nor written, in any of the three buffers.  A listed pixel's
 *   new samples are exactly those rt_render_device would add for the same passes; accum2 (nullable) gets
 *   their squares, count (nullable) rises by spp_count.  Lanes, chunking, the tail threshold and every
 *   kernel choice apply to a list of any length >= 1 as they do to a frame; with n == 0 or
 *   spp_count == 0 the call does nothing.  The list must stay unchanged during the call.
 * rt_adaptive_select_device: pix_out = the entries of pix_in[0..n) that are NOT converged under (tol,
 *   floor), in pix_in's order (a stable compaction: a list in 16x16-tile order stays in it); pix_in NULL
 *   means pixels 0..n-1.  *out_n = their number; *out_capped = how many of them have count >= max_spp
 *   (pixels a driver stops sampling unconverged).  pix_out holds n entries, must not overlap pix_in, and
 *   is written in [0, *out_n) only.  The entries index accum / accum2 / count, whose extent the call does
 *   not know: their range is the caller's responsibility.  Synchronises the stream.
 * rt_render_adaptive_device / rt_render_adaptive (host buffers, PCIe-inclusive): overwrite all three
 *   buffers (nx*ny*3, nx*ny*3, nx*ny).  Round 0 renders passes [0, min_spp) of every pixel, in the
 *   full-frame tile order; each later round the next batch_spp passes (the last cut at max_spp) of the
 *   still-active pixels only; after every round, the final one included, the selection compacts the
 *   active list on the device and two counters are read back (one small copy, one synchronise per
 *   round).  It stops when the list is empty or max_spp is reached.  Afterwards a pixel's accum equals
 *   rt_render_device of passes 0..count[j]-1 at that pixel, bit for bit, and count[j] is min_spp plus a
 *   multiple of batch_spp, or max_spp.  rt_get_stats then reports the rounds together (no kernel times).
 *   `out` receives the result record and may be NULL.
 *   Not available over tile shards or several GPUs (the active set would unbalance the deal).
 * After a failed call the buffers are unspecified.  Refused before any device work: null pointers,
 * min_spp < 2, max_spp < min_spp, batch_spp < 1, tol or floor negative or not finite, n < 0 or
 * n > nx*ny, bad handles.
 * rt_resolve_u8_counts(_device): the resolve above with each pixel's own count,
 *   floor(255.99*min(1, sqrt(accum[i]/count[i/3]))); a pixel with count 0 resolves to 0. */
#define RT_HAS_ADAPTIVE 1
typedef struct rt_adaptive {
    uint32_t min_spp, max_spp, batch_spp, reserved;
    double tol, floor;
} rt_adaptive;
typedef struct rt_adaptive_result {
    uint32_t rounds, reserved;
    uint64_t samples;            /* sum of count[] */
    uint64_t pixels_converged;   /* pixels that left the active list */
    uint64_t pixels_capped;      /* pixels still not converged at max_spp */
    double   ms_total;           /* wall time of the call's device part */
    double   ms_select;          /* of it: the selections with their readbacks */
} rt_adaptive_result;
int rt_render_pixels_device(int scene, int nx, int ny, const uint32_t* pix_device, int64_t n,
                            int spp_begin, int spp_count, uint64_t seed,
                            double* accum, double* accum2 /*nullable*/, uint32_t* count /*nullable*/, void* stream);
int rt_adaptive_select_device(int ctx, const uint32_t* pix_in /*nullable*/, int64_t n,
                              const double* accum, const double* accum2, const uint32_t* count,
                              double tol, double floor, uint32_t max_spp,
                              uint32_t* pix_out, int64_t* out_n, int64_t* out_capped, void* stream);
int rt_render_adaptive_device(int scene, int nx, int ny, const rt_adaptive* p, uint64_t seed,
                              double* accum, double* accum2, uint32_t* count, void* stream, rt_adaptive_result* out);
int rt_render_adaptive(int scene, int nx, int ny, const rt_adaptive* p, uint64_t seed,
                       double* accum_host, double* accum2_host, uint32_t* count_host, rt_adaptive_result* out);
int rt_resolve_u8_counts(const double* accum, const uint32_t* count, int nx, int ny, uint8_t* out);
int rt_resolve_u8_counts_device(int ctx, const double* accum_device, const uint32_t* count_device,
                                int nx, int ny, uint8_t* out_device, void* stream);

/* ---- first-hit feature buffers (an extension: what a denoiser or compositor reads beside the radiance) ---
 * Opt-in: nothing above changes.  RT_ABI_VERSION stays 7; test RT_HAS_FEATURES for these entry points.
 *
 * Each pixel j = y*nx+x (y-up) has one record of RT_FEATURE_DOUBLES running sums, feat[8j+0..2] albedo rgb,
 * [3..5] normal xyz, [6] t, [7] hits.  For every listed pixel and every pass s in [spp_begin,
 * spp_begin+spp_count) the call takes the camera ray rt_render* traces for (seed, pixel, s) — the same
 * draws in the same order: jitter u, jitter v, the unit-disk rejection loop, the time — and its closest hit
 * in (0.001, 999999999999); a constant medium's hit test goes on drawing from the same stream, so the hit
 * is the path's own first hit.  Each channel is added to the pixel's record in sample order, as accum is:
 *   hit:   albedo += the first-hit material's texture value at the hit point, as the shading evaluates it
 *          (lambertian / metal: the albedo texture; diffuse light: the emit texture, on either face; medium:
 *          the phase texture; dielectric: (1, 1, 1));
 *          normal += the hit record's normal as the scatter function receives it (after flip-normals and
 *          the translate / rotate-y chain, not renormalised; curves: -dir; a medium: (1, 0, 0));
 *          t += the hit record's t (curves: the distance along unit(dir), see rt_add_bezier); hits += 1.
 *   miss:  albedo += the ray's sky colour (gradient or black); the other five channels += 0.
 * pix_device (device memory, nullable = the whole frame) lists n unique pixels < nx*ny: the range is checked
 * by a read-only pass over the list before anything is written (an entry >= nx*ny fails the call with feat
 * untouched), pixels not listed are neither read nor written, and with n == 0 or spp_count == 0 the call
 * does nothing.  Null feat, bad handles and negative arguments are refused before any device work.  Device
 * faults (RT_FAULT_*) are reported as for renders.  rt_render_features: feat is a HOST buffer of nx*ny*8
 * doubles, copied to the device and back (the whole frame).  Not available over tile shards. */
#define RT_HAS_FEATURES 1
#define RT_FEATURE_DOUBLES 8
int rt_render_features_device(int scene, int nx, int ny, const uint32_t* pix_device /*nullable = whole frame*/, int64_t n,
                              int spp_begin, int spp_count, uint64_t seed, double* feat_device, void* stream);
int rt_render_features(int scene, int nx, int ny, int spp_begin, int spp_count, uint64_t seed, double* feat_host);

/* ---- denoiser (an extension): an edge-avoiding a-trous filter guided by the feature buffers and by the
 * variance of the mean that accum2 / count give — the spatial half of SVGF, with albedo demodulation.
 * Test RT_HAS_DENOISE.  out_mean receives the filtered per-pixel MEAN radiance (nx*ny*3; resolve it with
 * rt_resolve_u8(_device) and sample_count 1); it must not alias an input.  accum2 and count are nullable.
 * All arithmetic is f64 in this operation order (the library is built without FMA contraction;
 * rtamd.denoise.atrous is the NumPy restatement).
 *
 * Per pixel j, with n = (double)count[j] (count NULL: sample_count) and m = (double)feat_count:
 *     c_k   = n == 0 ? 0 : S_k / n                      S = accum[3j+k], k = 0,1,2
 *     a_k   = feat[8j+k] / m,  N = feat[8j+3..5] / m,  z = feat[8j+6] / m,  h = feat[8j+7] / m
 *     den_k = a_k > albedo_floor ? a_k : albedo_floor
 *     u_k   = c_k / den_k                               the demodulated signal
 *     d_k   = Q_k - (S_k*S_k)/n                         Q = accum2[3j+k]
 *     e_k   = ((d_k < 0 ? 0 : d_k) / (n*(n-1))) / (den_k*den_k)
 *     v     = (e_0 + e_1) + e_2                         0 where n < 2 or accum2 is NULL
 *     l     = (u_0 + u_1) + u_2
 * A pixel is *valid* when u_0, u_1, u_2 and v are all finite.
 * Iteration i = 0 .. iterations-1 has step s = 2^i.  For a valid pixel p = (x, y) the taps are q = (x + dx*s,
 * y + dy*s), dy = -2..2 the outer loop, dx = -2..2 the inner one; taps outside the frame and taps that are
 * not valid are skipped.  With k = [1/16, 1/4, 3/8, 1/4, 1/16] and hk = k[dy+2]*k[dx+2]:
 *     centre tap: w = hk;  any other tap:
 *     wn = 1 if h_p == 0 and h_q == 0, else g = (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z,
 *          wn = g > 0 ? g : 0, then wn = wn*wn repeated normal_squarings times
 *     zm = z_p > z_q ? z_p : z_q;   wz = exp(-(|z_p - z_q| / (sigma_z*zm + 1e-300)))
 *     wl = exp(-(|l_p - l_q| / (sigma_l*sqrt(v_p) + 1e-10))),  1 when accum2 is NULL
 *     w  = ((hk*wn)*wz)*wl
 *     W += w;  U_k += w*u_q,k;  V += (w*w)*v_q           each sum from 0, in tap order
 * then u'_k = U_k / W, v' = V / (W*W), and l is recomputed from u' for the next iteration.  A pixel that
 * is not valid keeps its u and v through every iteration.  After the last one out_mean[3j+k] = u_k*den_k.
 * Refused before any device work: iterations outside 1..12, normal_squarings > 16, sigma_z, sigma_l or
 * albedo_floor not finite or <= 0, feat_count == 0, null pointers (accum, feat, out_mean, p), out_mean
 * equal to an input, bad handles.  The filter's scratch (two signal buffers of 32 B and a guide buffer of
 * 40 B per pixel) belongs to the context: sized at first use, freed by rt_context_destroy and
 * rt_context_release_pools.  rt_denoise: the same with HOST buffers (PCIe-inclusive). */
#define RT_HAS_DENOISE 1
/* (a struct tag, not a typedef: the host entry point carries the same name) */
struct rt_denoise { uint32_t iterations, normal_squarings; double sigma_z, sigma_l, albedo_floor; };
int rt_denoise_device(int ctx, int nx, int ny, const struct rt_denoise* p,
                      const double* accum, const double* accum2 /*nullable*/, const uint32_t* count /*nullable*/, uint32_t sample_count,
                      const double* feat, uint32_t feat_count, double* out_mean /* nx*ny*3, may not alias the inputs */, void* stream);
int rt_denoise(int ctx, int nx, int ny, const struct rt_denoise* p,
               const double* accum, const double* accum2 /*nullable*/, const uint32_t* count /*nullable*/, uint32_t sample_count,
               const double* feat, uint32_t feat_count, double* out_mean);

/* ---- image textures — t:image-texture, texture.scm:36-50 ------------------------------------------------
 * Opt-in: nothing above changes.  RT_ABI_VERSION stays 7; test RT_HAS_IMAGE_TEXTURE for this entry point.
 *
 * rgb holds nx*ny texels of 3 BYTES (r, g, b), row 0 first, and row 0 is the TOP of the image (v = 1).  The
 * reference's `data` vector may hold any numbers (it takes floor->exact of each); this ABI takes bytes.  The
 * bytes are copied at the call.  The texture id is used like any other: as a material's albedo / emission, as
 * a checker's child (a checker hands u, v, p on to its children), as a constant medium's phase texture.
 *
 * The lookup for a hit with (u, v), all f64, in this operation order (repair R4, DESIGN.md §2: as written the
 * reference indexes `data` with an inexact number, which vector-ref refuses; the indices are floored):
 *   i = u * nx;  j = (1 - v) * ny - 0.001
 *   if (!(i >= 0)) i = 0;  if (!(j >= 0)) j = 0            (so a NaN lands on 0; no NaN is ever cast)
 *   if (i > nx - 1) i = nx - 1;  if (j > ny - 1) j = ny - 1
 *   ii = (int)floor(i);  jj = (int)floor(j);  texel = ii + nx * jj
 *   colour channel = (double)byte / 255.0, a correctly rounded f64 division (Gauche's exact (/ k 255) stored
 *   in an f64vector)
 * rtamd.image.lookup is the NumPy restatement.
 *
 * The hit record's u, v:
 *   rects (box faces are rects): geometry.scm:388-389, 407-408, 426-427 — with (a, b) the hit point's
 *     in-plane coordinates on the instance-local ray (XY: x, y; XZ: x, z; YZ: y, z),
 *     u = (a - a0) / (a1 - a0), v = (b - b0) / (b1 - b0);
 *   flip-normals, translate and rotate-y pass u, v through; constant media, Klein sets and curves give 0, 0;
 *   spheres and moving spheres (repair R5: get-sphere-uv, geometry.scm:138-144, takes (atan z z) and the asin of
 *     an unnormalised y, which is complex for |y| > 1 and makes the comparison raise) — the book's formula on
 *     the unit normal n = (p - centre(time)) * (1 / radius), before any flip:
 *     phi = atan2(n.z, n.x);  theta = asin(n.y < -1 ? -1 : n.y > 1 ? 1 : n.y)
 *     u = 1 - (phi + pi) / (2 * pi);  v = (theta + pi / 2) / pi       (divisions, not reciprocal products)
 *     atan2 / asin are the device library's (within an ulp or two of the C library's).
 * Image textures do not switch the exact libm on (RT_OPT_EXACT_LIBM): nothing in a lookup is a sin or cos.
 *
 * Refused with an rt_last_error message and before any device work: a null rgb or out_tex, nx or ny < 1,
 * nx*ny > 2^26, a scene whose images together would exceed 2^31 - 1 texels, a bad scene handle, a committed
 * scene.  Storage: 4 bytes per texel in device memory (RGBX, one load per lookup), freed with the scene. */
#define RT_HAS_IMAGE_TEXTURE 1
int rt_add_texture_image(int scene, const uint8_t* rgb /* nx*ny*3, row 0 = top */, int nx, int ny, int* out_tex);

#ifdef __cplusplus
}
#endif
#endif /* RTAMD_RT_H */
