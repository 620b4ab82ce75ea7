"""Device side of the drop-in: contexts, scene upload and rendering through
librtamd's C ABI.  There is no CPU fallback anywhere in this module."""
import contextlib
import ctypes

import numpy as np

from . import _lib
from ._lib import call, dvec, out_int
from .scene import emit

_default_ctx = {}


class Context:
    """A librtamd context on one HIP device (rt_context_create)."""

    def __init__(self, device=0):
        h = out_int()
        call("rt_context_create", int(device), ctypes.byref(h))
        self.handle = h.value
        self.device = device

    def set_option(self, name, value):
        """rt_context_set_option: a render-schedule option (_lib.RT_OPTIONS:
        lanes, max_paths, tail_paths, tail_div, tail_off); 0 = automatic.
        No schedule option changes an image, only how the work is scheduled.
        exact_libm (value or a _lib.RT_LIBM name: auto / exact / device)
        selects the bounce directions' sin / cos."""
        if name == "exact_libm" and isinstance(value, str):
            value = _lib.RT_LIBM[value]
        call("rt_context_set_option", self.handle, _lib.RT_OPTIONS[name], int(value))

    def get_option(self, name):
        v = ctypes.c_int64(0)
        call("rt_context_get_option", self.handle, _lib.RT_OPTIONS[name], ctypes.byref(v))
        return v.value

    @contextlib.contextmanager
    def options(self, **kv):
        """Set options for the duration of a with-block, then restore them."""
        old = {k: self.get_option(k) for k in kv}
        try:
            for k, val in kv.items():
                self.set_option(k, val)
            yield self
        finally:
            for k, val in old.items():
                self.set_option(k, val)

    def reset_options(self):
        for k in _lib.RT_OPTIONS:
            self.set_option(k, 0)

    def release_pools(self):
        """rt_context_release_pools: free the render lanes' path pools (the
        next render on this context allocates and sizes them again)."""
        call("rt_context_release_pools", self.handle)

    def close(self):
        if self.handle:
            call("rt_context_destroy", self.handle)
            self.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def device_count():
    n = out_int()
    call("rt_device_count", ctypes.byref(n))
    return n.value


class GpuBuilder:
    """Replays a scene descriptor graph into rt_add_* calls (scene.emit)."""

    def __init__(self, ctx):
        h = out_int()
        call("rt_scene_begin", ctx.handle, ctypes.byref(h))
        self.scene = h.value

    def _out(self, name, *args):
        o = out_int()
        call(name, self.scene, *args, ctypes.byref(o))
        return o.value

    def texture_constant(self, rgb):
        return self._out("rt_add_texture_constant", dvec(rgb))

    def texture_checker(self, even, odd):
        return self._out("rt_add_texture_checker", even, odd)

    def texture_noise(self, sc):
        return self._out("rt_add_texture_noise", sc)

    def texture_marble(self, sc):
        return self._out("rt_add_texture_marble", sc)

    def texture_image(self, data, nx, ny):
        """data: contiguous uint8 array of nx*ny*3 (row 0 = top); the library copies it."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.size != nx * ny * 3:
            raise ValueError("image texture data must have nx*ny*3 bytes")
        return self._out("rt_add_texture_image", data.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), int(nx), int(ny))

    def material_lambertian(self, tex):
        return self._out("rt_add_material_lambertian", tex)

    def material_metal(self, tex, fuzz):
        return self._out("rt_add_material_metal", tex, fuzz)

    def material_dielectric(self, ref_idx):
        return self._out("rt_add_material_dielectric", ref_idx)

    def material_diffuse_light(self, tex):
        return self._out("rt_add_material_diffuse_light", tex)

    def sphere(self, c, r, mat):
        return self._out("rt_add_sphere", dvec(c), r, mat)

    def moving_sphere(self, c0, c1, t0, t1, r, mat):
        return self._out("rt_add_moving_sphere", dvec(c0), dvec(c1), t0, t1, r, mat)

    def rect(self, axis, a0, a1, b0, b1, k, mat):
        return self._out("rt_add_rect", axis, a0, a1, b0, b1, k, mat)

    def bezier(self, a, b, c, d, width, mat):
        return self._out("rt_add_bezier", dvec(a), dvec(b), dvec(c), dvec(d), width, mat)

    def bezier_array(self, cps, width, mat):
        """cps: contiguous float64 array of shape (n, 12); returns the first id."""
        cps = np.ascontiguousarray(cps, dtype=np.float64)
        ptr = cps.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        return self._out("rt_add_bezier_array", ptr, int(cps.shape[0]), width, mat)

    def klein(self, center, mat):
        return self._out("rt_add_klein", dvec(center), mat)

    def triangle(self, a, b, c, mat):
        return self._out("rt_add_triangle", dvec(a), dvec(b), dvec(c), mat)

    def mesh(self, verts, faces, uvs, mat, normals=None):
        """verts (nv, 3) float64, faces (nf, 3) int32, uvs (nv, 2) float64 or None, normals (nv, 3) float64 or
        None (rt_add_mesh_normals); returns the mesh's list object."""
        verts = np.ascontiguousarray(verts, dtype=np.float64)
        faces = np.ascontiguousarray(faces, dtype=np.int32)
        dp = ctypes.POINTER(ctypes.c_double)
        uv = None
        if uvs is not None:
            uvs = np.ascontiguousarray(uvs, dtype=np.float64)
            uv = uvs.ctypes.data_as(dp)
        if normals is not None:
            normals = np.ascontiguousarray(normals, dtype=np.float64)
            if normals.shape != (verts.shape[0], 3):
                raise ValueError("mesh: normals must have shape (nv, 3)")
            return self._out("rt_add_mesh_normals", verts.ctypes.data_as(dp), int(verts.shape[0]),
                             faces.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(faces.shape[0]), uv,
                             normals.ctypes.data_as(dp), mat)
        return self._out("rt_add_mesh", verts.ctypes.data_as(dp), int(verts.shape[0]),
                         faces.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(faces.shape[0]), uv, mat)

    def constant_medium(self, boundary, density, tex):
        return self._out("rt_add_constant_medium", boundary, density, tex)

    def flip_normals(self, obj):
        return self._out("rt_add_flip_normals", obj)

    def box(self, p0, p1, mat):
        return self._out("rt_add_box", dvec(p0), dvec(p1), mat)

    def translate(self, obj, off):
        return self._out("rt_add_translate", obj, dvec(off))

    def rotate_y(self, obj, angle):
        return self._out("rt_add_rotate_y", obj, angle)

    def list(self, objs):
        arr = (ctypes.c_int * max(1, len(objs)))(*objs)
        return self._out("rt_add_list", arr, len(objs))

    def bvh(self, objs, t0, t1, sah):
        arr = (ctypes.c_int * max(1, len(objs)))(*objs)
        return self._out("rt_add_bvh", arr, len(objs), t0, t1, sah)

    def set_camera(self, slots):
        call("rt_set_camera", self.scene, dvec(slots))

    def set_light(self, obj):
        call("rt_set_light_sampling", self.scene, obj)

    def set_lights(self, objs):
        """rt_set_light_list: the objects (rects, spheres, triangles, flips, lists, meshes) the mixture samples."""
        arr = (ctypes.c_int * max(1, len(objs)))(*objs)
        call("rt_set_light_list", self.scene, arr, len(objs))

    def set_sky(self, code):
        call("rt_set_sky", self.scene, code)

    def set_perlin(self, ranvec, px, py, pz):
        i32 = ctypes.c_int32 * 256
        call("rt_set_perlin_tables", self.scene, dvec(ranvec), i32(*px), i32(*py), i32(*pz))

    def commit(self, world):
        call("rt_scene_commit", self.scene, world)
        return self.scene


def upload(scene, ctx=None):
    """Commit a scene (rtamd.scene.Scene) on ctx; cached per context."""
    ctx = ctx or default_context()
    h = scene._handles.get(ctx.handle)
    if h is None:
        h = emit(scene, GpuBuilder(ctx))
        scene._handles[ctx.handle] = h
    return h


def stats(scene_handle):
    s = _lib.RtStats()
    call("rt_get_stats", scene_handle, ctypes.byref(s))
    return s


def scene_info(scene_handle):
    """rt_get_scene_info as a dict (tree sizes, LDS kernel footprints and grids)."""
    s = _lib.RtSceneInfo()
    call("rt_get_scene_info", scene_handle, ctypes.byref(s))
    return {name: getattr(s, name) for name, _ in s._fields_ if name != "reserved"}


def tree_info(scene_handle):
    """rt_get_tree_info as a dict: the leaves the world tree took (world-level spheres, curves, generic
    leaves), those left in brute-force groups, the trees' sizes, the rotation table's entries, the
    RTAMD_BVH_GENERIC_MIN in force at the commit, and for a media forest its segments and how many got a tree
    (both 0 otherwise)."""
    s = _lib.RtTreeInfo()
    call("rt_get_tree_info", scene_handle, ctypes.byref(s))
    return {name: getattr(s, name) for name, _ in s._fields_ if name != "reserved"}


def point_hits(scene_handle):
    """rt_scene_point_hits: whether the scene's wavefront queues lambertian hits as point records under the
    current RTAMD_NO_POINT_HITS (images are the same either way)."""
    o = out_int()
    call("rt_scene_point_hits", scene_handle, ctypes.byref(o))
    return bool(o.value)


def render_host(scene, nx, ny, spp_begin, spp_count, seed, accum, ctx=None):
    """rt_render: accum is a host float64 array of nx*ny*3 (updated in place)."""
    h = upload(scene, ctx)
    a = np.ascontiguousarray(accum, dtype=np.float64)
    if a.size != nx * ny * 3:
        raise ValueError("accum must have nx*ny*3 elements")
    call("rt_render", h, nx, ny, spp_begin, spp_count, ctypes.c_uint64(seed & (2**64 - 1)),
         a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if a is not accum:
        accum[...] = a.reshape(accum.shape)
    return h


def render_device(scene, nx, ny, spp_begin, spp_count, seed, accum_ptr, shard=0, nshard=1, stream=None,
                  ctx=None):
    """rt_render_device: accum_ptr is a device pointer (int) to nx*ny*3 doubles."""
    h = upload(scene, ctx)
    call("rt_render_device", h, nx, ny, spp_begin, spp_count, ctypes.c_uint64(seed & (2**64 - 1)), shard,
         nshard, ctypes.c_void_p(accum_ptr), ctypes.c_void_p(stream or 0))
    return h


def render_rows_device(scene, nx, ny, y_begin, y_count, spp_begin, spp_count, seed, accum_ptr, stream=None,
                       ctx=None):
    """rt_render_rows_device: passes of rows [y_begin, y_begin+y_count) into a full-frame device accumulator."""
    h = upload(scene, ctx)
    call("rt_render_rows_device", h, nx, ny, y_begin, y_count, spp_begin, spp_count,
         ctypes.c_uint64(seed & (2**64 - 1)), ctypes.c_void_p(accum_ptr), ctypes.c_void_p(stream or 0))
    return h


def render_rows_host(scene, nx, ny, y_begin, y_count, spp_begin, spp_count, seed, accum, ctx=None):
    """rt_render_rows: as render_rows_device on a host float64 frame (only the band crosses PCIe)."""
    h = upload(scene, ctx)
    if accum.dtype != np.float64 or not accum.flags.c_contiguous or accum.size != nx * ny * 3:
        raise ValueError("accum must be a contiguous float64 array of nx*ny*3 elements")
    call("rt_render_rows", h, nx, ny, y_begin, y_count, spp_begin, spp_count, ctypes.c_uint64(seed & (2**64 - 1)),
         accum.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return h


def trace_line(scene, nx, ny, y, sample_count, seed, raw_data, image, ctx=None):
    """rt_trace_line (main.scm:452-469): pass `sample_count` of row y into raw_data, row y of image resolved."""
    h = upload(scene, ctx)
    if raw_data.dtype != np.float64 or not raw_data.flags.c_contiguous or raw_data.size != nx * ny * 3:
        raise ValueError("raw_data must be a contiguous float64 array of nx*ny*3 elements")
    if image.dtype != np.uint8 or not image.flags.c_contiguous or image.size != nx * ny * 3:
        raise ValueError("image must be a contiguous uint8 array of nx*ny*3 elements")
    call("rt_trace_line", h, nx, ny, y, sample_count, ctypes.c_uint64(seed & (2**64 - 1)),
         raw_data.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
         image.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    return h


def render_shard_device(scene, nx, ny, spp_begin, spp_count, seed, shard, nshard, accum_ptr, stream=None, ctx=None):
    """rt_render_shard_device: one shard's tiles into a compact device accumulator (shard_pixels order)."""
    h = upload(scene, ctx)
    call("rt_render_shard_device", h, nx, ny, spp_begin, spp_count, ctypes.c_uint64(seed & (2**64 - 1)), shard,
         nshard, ctypes.c_void_p(accum_ptr), ctypes.c_void_p(stream or 0))
    return h


#: rt_hit_rays_walk's walks (include/rt.h)
WALK_HBM, WALK_LDS_TIME0, WALK_LDS_CAMERA = 0, 1, 2


def hit_rays(scene, rays, ctx=None, walk=WALK_HBM):
    """rt_hit_rays_walk: rays = (n, 7) float64 (origin, direction, time); returns
    (t, material id) arrays, material -1 for a miss.  ``walk``: the closest-hit
    walk the rays take (WALK_HBM is rt_hit_rays)."""
    h = upload(scene, ctx)
    r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 7)
    n = r.shape[0]
    t = np.zeros(n)
    m = np.zeros(n, dtype=np.int32)
    call("rt_hit_rays_walk", h, int(walk), n, r.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
         t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return t, m


def hit_rays_stream(scene, rays, seed, ctx=None):
    """rt_hit_rays_stream: hit_rays in device memory with ray k on the path stream (seed, pixel k, sample 0);
    returns (t, material id, draws) arrays, draws = the random numbers each query consumed.  Takes scenes
    with constant media too."""
    h = upload(scene, ctx)
    r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 7)
    n = r.shape[0]
    t = np.zeros(n)
    m = np.zeros(n, dtype=np.int32)
    draws = np.zeros(n, dtype=np.int32)
    call("rt_hit_rays_stream", h, r.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n,
         ctypes.c_uint64(seed & (2**64 - 1)), t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
         m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), draws.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return t, m, draws


def light_probe(scene, points, seed, dirs=None, ctx=None):
    """rt_light_probe: the mixture's light sampler and density for points (n, 3), point k on the path stream
    (seed, pixel k, sample 0).  Returns (out_dir (n, 3), out_pdf (n,), out_pdf_dirs (n,) or None, draws (n,)):
    random(point), pdf_value(point, out_dir), pdf_value(point, dirs[k]) and the random numbers consumed."""
    h = upload(scene, ctx)
    dp = ctypes.POINTER(ctypes.c_double)
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    d = None
    if dirs is not None:
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        if d.shape[0] != n:
            raise ValueError("one direction per point")
    out_dir, out_pdf = np.zeros((n, 3)), np.zeros(n)
    out_pdf_dirs = np.zeros(n) if d is not None else None
    draws = np.zeros(n, dtype=np.int32)
    call("rt_light_probe", h, n, p.ctypes.data_as(dp), d.ctypes.data_as(dp) if d is not None else None, _u64(seed),
         out_dir.ctypes.data_as(dp), out_pdf.ctypes.data_as(dp),
         out_pdf_dirs.ctypes.data_as(dp) if d is not None else None, draws.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return out_dir, out_pdf, out_pdf_dirs, draws


#: rt_step_rays' extends, modes and status bit (include/rt.h)
STEP_EXTEND_HBM, STEP_EXTEND_LDS = 0, 1
STEP_STEP, STEP_TAIL, STEP_FUSED = 0, 1, 2
#: StepResult.extend: the extend launch_extend took
EXTEND_PER_RAY, EXTEND_CURVES, EXTEND_CURVES_FUSED, EXTEND_CURVES_FUSED_EXACT = 0, 1, 2, 3
STEP_WROTE = 256
STEP_SENTINEL = 0x7FF8DEAD5CA77E12


class StepResult:
    """rt_step_rays' outputs.  status (n,) int32: survivor entries of the record | STEP_WROTE; color (n, 3) the
    record's sample slot; ray (n, 6), T (n, 3), ctr (n,) the survivor; t (n,), mat (n,) the queued hit (-1: none);
    survivors: the device's survivor count; shade: {material type: (TL, LS, LL, EX, PT)} of the k_shade
    instances launched (STEP); finish: (F, TL, LS, SOLO, EX) of the k_finish instance (TAIL), else None; extend:
    the extend launched (EXTEND_*; STEP with the HBM extend, FUSED).  FUSED: status and color as for TAIL, and
    survivors holds the continuation segments the fused launch counted."""
    __slots__ = ("status", "color", "ray", "T", "ctr", "t", "mat", "survivors", "shade", "finish", "extend")

    def wrote(self):
        return (self.status & STEP_WROTE) != 0

    def entries(self):
        return self.status & 255


def step_rays(scene, rays, T_in=None, ctr_in=None, pix=None, seed=0, smp=0, depth=0, extend=STEP_EXTEND_HBM,
              mode=STEP_STEP, ctx=None):
    """rt_step_rays: one wavefront iteration (extend + every material's shade, or the tail kernel) on the
    caller's path states.  rays (n, 7) float64 (origin, direction, time); T_in (n, 3), default 1; ctr_in (n,),
    default 0; pix (n,) or None (pixel key k).  Returns a StepResult."""
    h = upload(scene, ctx)
    dp, ip, up = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
    r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 7)
    n = r.shape[0]
    T = np.ones((n, 3)) if T_in is None else np.ascontiguousarray(T_in, dtype=np.float64).reshape(-1, 3)
    c = np.zeros(n, dtype=np.uint32) if ctr_in is None else np.ascontiguousarray(ctr_in, dtype=np.uint32).reshape(-1)
    p = None if pix is None else np.ascontiguousarray(pix, dtype=np.uint32).reshape(-1)
    if T.shape[0] != n or c.shape[0] != n or (p is not None and p.shape[0] != n):
        raise ValueError("one throughput, counter and pixel key per ray")
    res = StepResult()
    res.status = np.zeros(n, dtype=np.int32)
    res.color, res.ray, res.T = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros((n, 3))
    res.ctr, res.t, res.mat = np.zeros(n, dtype=np.uint32), np.zeros(n), np.full(n, -1, dtype=np.int32)
    inst = np.zeros(32, dtype=np.int32)
    surv = ctypes.c_uint32(0)
    call("rt_step_rays", h, n, r.ctypes.data_as(dp), T.ctypes.data_as(dp), c.ctypes.data_as(up),
         p.ctypes.data_as(up) if p is not None else None, _u64(seed), ctypes.c_uint32(int(smp)), int(depth), int(extend),
         int(mode), res.status.ctypes.data_as(ip), res.color.ctypes.data_as(dp), res.ray.ctypes.data_as(dp),
         res.T.ctypes.data_as(dp), res.ctr.ctypes.data_as(up), res.t.ctypes.data_as(dp), res.mat.ctypes.data_as(ip),
         inst.ctypes.data_as(ip), ctypes.byref(surv))
    res.survivors = int(surv.value)
    res.shade, res.finish, res.extend = {}, None, int(inst[7])
    if n and mode == STEP_FUSED:
        pass
    elif n and mode == STEP_TAIL:
        res.finish = (int(inst[1]), int(inst[2]), int(inst[3]), bool(inst[4]), bool(inst[5]))
    elif n:
        res.shade = {m: (int(inst[8 * m + 1]), int(inst[8 * m + 2]), bool(inst[8 * m + 3]), bool(inst[8 * m + 4]),
                         bool(inst[8 * m + 5])) for m in range(4) if inst[8 * m]}
    return res


def resolve_u8(accum, nx, ny, sample_count):
    """rt_resolve_u8 (main.scm:481-491) on the host."""
    a = np.ascontiguousarray(accum, dtype=np.float64).ravel()
    out = np.zeros(nx * ny * 3, dtype=np.uint8)
    call("rt_resolve_u8", a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nx, ny, int(sample_count),
         out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    return out


def resolve_u8_device(accum_ptr, nx, ny, sample_count, out_ptr, stream=None, ctx=None):
    """rt_resolve_u8_device (main.scm:481-491) on device buffers: nx*ny*3 doubles -> bytes."""
    ctx = ctx or default_context()
    call("rt_resolve_u8_device", ctx.handle, ctypes.c_void_p(accum_ptr), nx, ny, int(sample_count),
         ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0))


def _u64(seed):
    return ctypes.c_uint64(seed & (2**64 - 1))


def _result_dict(r):
    return {name: getattr(r, name) for name, _ in r._fields_ if name != "reserved"}


def adaptive_params(tol, min_spp=16, max_spp=1024, batch_spp=16, floor=0.05):
    """An rt_adaptive record (include/rt.h, "adaptive sampling")."""
    return _lib.RtAdaptive(int(min_spp), int(max_spp), int(batch_spp), 0, float(tol), float(floor))


def render_pixels_device(scene, nx, ny, pix_ptr, n, spp_begin, spp_count, seed, accum_ptr, accum2_ptr=None,
                         count_ptr=None, stream=None, ctx=None):
    """rt_render_pixels_device: passes of the n pixels listed at device pointer pix_ptr (uint32, unique,
    < nx*ny) into full-frame device buffers: accum, and optionally the squares' sums and sample counts."""
    h = upload(scene, ctx)
    call("rt_render_pixels_device", h, nx, ny, ctypes.c_void_p(pix_ptr), int(n), spp_begin, spp_count, _u64(seed),
         ctypes.c_void_p(accum_ptr), ctypes.c_void_p(accum2_ptr or 0), ctypes.c_void_p(count_ptr or 0),
         ctypes.c_void_p(stream or 0))
    return h


def adaptive_select_device(pix_in_ptr, n, accum_ptr, accum2_ptr, count_ptr, tol, floor, max_spp, pix_out_ptr,
                           stream=None, ctx=None):
    """rt_adaptive_select_device: the not-converged entries of the list at pix_in_ptr (None: pixels 0..n-1)
    to pix_out_ptr, in order; returns (their number, how many of them have count >= max_spp)."""
    ctx = ctx or default_context()
    m, capped = ctypes.c_int64(0), ctypes.c_int64(0)
    call("rt_adaptive_select_device", ctx.handle, ctypes.c_void_p(pix_in_ptr or 0), int(n), ctypes.c_void_p(accum_ptr),
         ctypes.c_void_p(accum2_ptr), ctypes.c_void_p(count_ptr), float(tol), float(floor), int(max_spp),
         ctypes.c_void_p(pix_out_ptr), ctypes.byref(m), ctypes.byref(capped), ctypes.c_void_p(stream or 0))
    return m.value, capped.value


def render_adaptive_device(scene, nx, ny, params, seed, accum_ptr, accum2_ptr, count_ptr, stream=None, ctx=None):
    """rt_render_adaptive_device: the adaptive render into device buffers (all three overwritten);
    params = adaptive_params(...).  Returns the result record as a dict."""
    h = upload(scene, ctx)
    res = _lib.RtAdaptiveResult()
    call("rt_render_adaptive_device", h, nx, ny, ctypes.byref(params), _u64(seed), ctypes.c_void_p(accum_ptr),
         ctypes.c_void_p(accum2_ptr), ctypes.c_void_p(count_ptr), ctypes.c_void_p(stream or 0), ctypes.byref(res))
    return _result_dict(res)


def render_adaptive_host(scene, nx, ny, params, seed, ctx=None):
    """rt_render_adaptive: returns (accum, accum2, count, result dict) as new host arrays."""
    h = upload(scene, ctx)
    accum = np.zeros(nx * ny * 3)
    accum2 = np.zeros(nx * ny * 3)
    count = np.zeros(nx * ny, dtype=np.uint32)
    res = _lib.RtAdaptiveResult()
    call("rt_render_adaptive", h, nx, ny, ctypes.byref(params), _u64(seed),
         accum.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), accum2.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
         count.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(res))
    return accum, accum2, count, _result_dict(res)


def resolve_u8_counts(accum, count, nx, ny):
    """rt_resolve_u8_counts on the host: sqrt(sum / the pixel's own count), 0 where the count is 0."""
    a = np.ascontiguousarray(accum, dtype=np.float64).ravel()
    c = np.ascontiguousarray(count, dtype=np.uint32).ravel()
    if a.size != nx * ny * 3 or c.size != nx * ny:
        raise ValueError("accum must have nx*ny*3 elements and count nx*ny")
    out = np.zeros(nx * ny * 3, dtype=np.uint8)
    call("rt_resolve_u8_counts", a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
         c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), nx, ny, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
    return out


def resolve_u8_counts_device(accum_ptr, count_ptr, nx, ny, out_ptr, stream=None, ctx=None):
    """rt_resolve_u8_counts_device on device buffers: nx*ny*3 doubles and nx*ny counts -> bytes."""
    ctx = ctx or default_context()
    call("rt_resolve_u8_counts_device", ctx.handle, ctypes.c_void_p(accum_ptr), ctypes.c_void_p(count_ptr), nx, ny,
         ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0))


def render_features_device(scene, nx, ny, spp_begin, spp_count, seed, feat_ptr, pix_ptr=None, n=0, stream=None,
                           ctx=None):
    """rt_render_features_device: the first-hit features (albedo, normal, t, hits: 8 running sums per pixel)
    of passes [spp_begin, spp_begin+spp_count) added to the nx*ny*8 doubles at device pointer feat_ptr, for
    the whole frame or the n pixels listed at device pointer pix_ptr (uint32, unique, < nx*ny)."""
    h = upload(scene, ctx)
    call("rt_render_features_device", h, nx, ny, ctypes.c_void_p(pix_ptr or 0), int(n), spp_begin, spp_count, _u64(seed),
         ctypes.c_void_p(feat_ptr), ctypes.c_void_p(stream or 0))
    return h


def render_features_host(scene, nx, ny, spp_begin, spp_count, seed, feat, ctx=None):
    """rt_render_features: as render_features_device on a host float64 array of nx*ny*8 (updated in place)."""
    h = upload(scene, ctx)
    if feat.dtype != np.float64 or not feat.flags.c_contiguous or feat.size != nx * ny * _lib.RT_FEATURE_DOUBLES:
        raise ValueError("feat must be a contiguous float64 array of nx*ny*8 elements")
    call("rt_render_features", h, nx, ny, spp_begin, spp_count, _u64(seed),
         feat.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    return h


def denoise_params(iterations=5, normal_squarings=7, sigma_z=0.1, sigma_l=4.0, albedo_floor=1e-2):
    """A struct rt_denoise (include/rt.h, "denoiser") at the defaults of rtamd.denoise.DEFAULTS."""
    return _lib.RtDenoise(int(iterations), int(normal_squarings), float(sigma_z), float(sigma_l), float(albedo_floor))


def denoise_device(nx, ny, params, accum_ptr, accum2_ptr, count_ptr, sample_count, feat_ptr, feat_count, out_ptr,
                   stream=None, ctx=None):
    """rt_denoise_device: the filtered per-pixel mean radiance (nx*ny*3 doubles at out_ptr) of the sums at
    accum_ptr, guided by the feature sums at feat_ptr (feat_count passes) and, where accum2_ptr is given, by
    the variance of the mean; count_ptr None: every pixel has sample_count samples."""
    ctx = ctx or default_context()
    call("rt_denoise_device", ctx.handle, nx, ny, ctypes.byref(params), ctypes.c_void_p(accum_ptr),
         ctypes.c_void_p(accum2_ptr or 0), ctypes.c_void_p(count_ptr or 0), int(sample_count), ctypes.c_void_p(feat_ptr),
         int(feat_count), ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or 0))


def denoise_host(nx, ny, params, accum, accum2, count, sample_count, feat, feat_count, ctx=None):
    """rt_denoise on host arrays (accum2 and count may be None); returns the filtered mean, nx*ny*3 float64."""
    ctx = ctx or default_context()
    dp, up = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    a = np.ascontiguousarray(accum, dtype=np.float64).ravel()
    f = np.ascontiguousarray(feat, dtype=np.float64).ravel()
    if a.size != nx * ny * 3 or f.size != nx * ny * _lib.RT_FEATURE_DOUBLES:
        raise ValueError("accum must have nx*ny*3 elements and feat nx*ny*8")
    a2 = None if accum2 is None else np.ascontiguousarray(accum2, dtype=np.float64).ravel()
    c = None if count is None else np.ascontiguousarray(count, dtype=np.uint32).ravel()
    if (a2 is not None and a2.size != a.size) or (c is not None and c.size != nx * ny):
        raise ValueError("accum2 must have nx*ny*3 elements and count nx*ny")
    out = np.zeros(nx * ny * 3)
    call("rt_denoise", ctx.handle, nx, ny, ctypes.byref(params), a.ctypes.data_as(dp),
         a2.ctypes.data_as(dp) if a2 is not None else None, c.ctypes.data_as(up) if c is not None else None,
         int(sample_count), f.ctypes.data_as(dp), int(feat_count), out.ctypes.data_as(dp))
    return out


def curve_depth_probe(cps, eps8, ctx=None):
    """rt_curve_depth_probe: the curve kernels' depth estimate (bez_maxd) for ray-space control points
    cps (n, 12) and 8 eps (n,); returns int32 depths."""
    ctx = ctx or default_context()
    c = np.ascontiguousarray(cps, dtype=np.float64).reshape(-1, 12)
    e = np.ascontiguousarray(eps8, dtype=np.float64).ravel()
    if e.size != c.shape[0]:
        raise ValueError("one eps8 per curve")
    out = np.zeros(c.shape[0], dtype=np.int32)
    call("rt_curve_depth_probe", ctx.handle, c.shape[0], c.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
         e.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    return out


F64_KINDS = {"sqrt_mid": 0, "rcp_mid": 1, "sqrt_core": 2, "rcp_core": 3}    # include/rt.h RT_F64_*


def f64_probe(kind, values, ctx=None):
    """rt_f64_probe: the kernels' sqrt / reciprocal helper `kind` (F64_KINDS) of every value; float64."""
    ctx = ctx or default_context()
    x = np.ascontiguousarray(values, dtype=np.float64).ravel()
    out = np.zeros(x.size, dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    call("rt_f64_probe", ctx.handle, F64_KINDS[kind], x.ctypes.data_as(dp), x.size, out.ctypes.data_as(dp))
    return out


def comm_unique_id():
    """rt_comm_unique_id: a new communicator id (RT_COMM_ID_BYTES bytes), made by rank 0."""
    buf = (ctypes.c_uint8 * _lib.RT_COMM_ID_BYTES)()
    call("rt_comm_unique_id", buf)
    return bytes(buf)


class Comm:
    """rt_comm_create / rt_gather_shards / rt_comm_destroy: the frame-end gather of a multi-GPU frame
    (one process per GPU) over RCCL, behind the C ABI."""

    def __init__(self, unique_id, rank, world, ctx=None):
        if len(unique_id) != _lib.RT_COMM_ID_BYTES:
            raise ValueError("a communicator id has %d bytes" % _lib.RT_COMM_ID_BYTES)
        self.ctx = ctx or default_context()
        self.rank, self.world = rank, world
        buf = (ctypes.c_uint8 * _lib.RT_COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        h = ctypes.c_int(0)
        call("rt_comm_create", self.ctx.handle, buf, rank, world, ctypes.byref(h))
        self.handle = h.value

    def gather_shards(self, nx, ny, accum_compact_ptr, frame_ptr, stream=None):
        """rt_gather_shards (collective): every rank's compact accumulator into rank 0's frame."""
        call("rt_gather_shards", self.handle, nx, ny, ctypes.c_void_p(accum_compact_ptr),
             ctypes.c_void_p(frame_ptr or 0), ctypes.c_void_p(stream or 0))

    def close(self):
        if getattr(self, "handle", None):
            call("rt_comm_destroy", self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def shard_pixels(nx, ny, shard, nshard):
    """rt_shard_pixels: the image pixels (j = y*nx + x) shard `shard` renders."""
    n = ctypes.c_int64(0)
    call("rt_shard_pixels", nx, ny, shard, nshard, None, ctypes.byref(n))
    out = np.zeros(n.value, dtype=np.uint32)
    call("rt_shard_pixels", nx, ny, shard, nshard, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
         ctypes.byref(n))
    return out


def gather_layout(nx, ny, world):
    """rt_gather_layout (host only): per rank its shard's pixel count and the offset of its pixels in the
    ranks' concatenated pixel lists; rank 0 receives rank r's compact accumulator at doubles
    3 * (offset[r] - count[0]) of its receive buffer."""
    cnt = np.zeros(world, dtype=np.int64)
    off = np.zeros(world, dtype=np.int64)
    call("rt_gather_layout", nx, ny, world, cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
         off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return cnt, off


def gather_shards_local(nx, ny, shard_ptrs, frame_ptr, ctx=None, stream=None):
    """rt_gather_shards_local: every shard's compact accumulator (device pointers, shard r in entry r) on
    this context's device into the frame — rt_gather_shards' receive layout and placement without RCCL."""
    ctx = ctx or default_context()
    arr = (ctypes.c_void_p * len(shard_ptrs))(*[ctypes.c_void_p(p) for p in shard_ptrs])
    call("rt_gather_shards_local", ctx.handle, nx, ny, len(shard_ptrs), arr, ctypes.c_void_p(frame_ptr),
         ctypes.c_void_p(stream or 0))
