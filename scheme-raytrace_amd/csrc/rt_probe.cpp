// rt_probe.cpp — the C ABI's probe entry points: single kernels and single steps of a render on the
// caller's arrays (closest-hit walks, the light sampler, one wavefront step or tail, the curve depth bound,
// the lean f64 helpers).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rt_host.h"
#include "rt_launch.h"

using namespace rtamd;

namespace {
// A probe's shell: device arrays for the caller's host arrays, copied in as they are made and out by
// finish(), all on the context's stream; the fault word cleared before and reported after.
struct Probe {
    hipStream_t st = nullptr;
    DevBuf bufs[8];
    struct Out { void* host; const void* dev; size_t bytes; } outs[8];
    int nbufs = 0, nouts = 0;
    bool faults = true;                          // (rt_curve_depth_probe's kernel raises none: no scene)

    int begin(Context* c, bool fault_word = true) {
        HIPCHK(hipSetDevice(c->device));
        st = c->stream;
        faults = fault_word;
        uint32_t stale = 0;
        if (faults) HIPCHK(take_fault(&stale));
        return 0;
    }
    template <class T> int alloc(size_t count, T** dev) {
        HIPCHK(bufs[nbufs].ensure(count * sizeof(T)));
        *dev = bufs[nbufs++].as<T>();
        return 0;
    }
    template <class T> int in(const T* host, size_t count, const T** dev) {
        T* d = nullptr;
        if (int rc = alloc(count, &d)) return rc;
        HIPCHK(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st));
        *dev = d;
        return 0;
    }
    template <class T> void later(T* host, const T* dev, size_t count) { outs[nouts++] = Out{host, dev, count * sizeof(T)}; }
    template <class T> int out(T* host, size_t count, T** dev) {
        if (int rc = alloc(count, dev)) return rc;
        later(host, *dev, count);
        return 0;
    }
    int finish() {
        for (int i = 0; i < nouts; ++i)
            HIPCHK(hipMemcpyAsync(outs[i].host, outs[i].dev, outs[i].bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        uint32_t f = 0;
        if (faults) HIPCHK(take_fault(&f));
        return f ? fail(fault_text(f)) : 0;
    }
};
#define TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)
}  // namespace

extern "C" {

int rt_hit_rays(int scene, int n, const double* rays, double* out_t, int32_t* out_mat) {
    return rt_hit_rays_walk(scene, RT_WALK_HBM, n, rays, out_t, out_mat);
}

int rt_hit_rays_walk(int scene, int walk, int n, const double* rays, double* out_t, int32_t* out_mat) {
    LOCK_SCENE(s, scene);
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    if (walk != RT_WALK_HBM && walk != RT_WALK_LDS_TIME0 && walk != RT_WALK_LDS_CAMERA)
        return fail("rt_hit_rays_walk: unknown walk " + std::to_string(walk));
    if (n < 0) return fail("ray count must be >= 0");
    if (n > 0 && (!rays || !out_t || !out_mat)) return fail("null pointer");
    if (s->dev.n_med > 0) return fail("rt_hit_rays: the scene has constant media, whose hit test draws random numbers");
    if (walk == RT_WALK_LDS_TIME0 && s->ext_lds == 0)
        return fail("rt_hit_rays_walk: this scene's time-0 tree does not run from LDS (rt_scene_info.extend_lds_bytes "
                    "is 0: no sphere BVH, curves or a Klein set in the world, or a tree over the LDS budget)");
    if (walk == RT_WALK_LDS_CAMERA && s->cam_lds == 0)
        return fail("rt_hit_rays_walk: this scene's camera rays do not walk a tree in LDS (rt_scene_info."
                    "camera_lds_bytes is 0: no sphere BVH, curves or a Klein set in the world, or a tree over the "
                    "LDS budget)");
    if (walk == RT_WALK_LDS_TIME0)
        for (int i = 0; i < n; ++i) {
            uint64_t bits;
            std::memcpy(&bits, &rays[7 * (size_t)i + 6], sizeof bits);
            if (bits != 0)
                return fail("rt_hit_rays_walk: RT_WALK_LDS_TIME0 takes rays of time +0.0 only (ray " +
                            std::to_string(i) + " has another time)");
        }
    CTX_OF(c, s);
    if (n == 0) return 0;
    Probe p;
    const double* d_rays; double* d_t; int32_t* d_mat;
    TRY(p.begin(c));
    TRY(p.in(rays, (size_t)n * 7, &d_rays));
    TRY(p.out(out_t, n, &d_t));
    TRY(p.out(out_mat, n, &d_mat));
    if (walk == RT_WALK_HBM)
        HIPCHK(launch_hit_rays(s->dev, d_rays, (uint32_t)n, d_t, d_mat, p.st));
    else
        HIPCHK(launch_hit_rays_lds(s->dev, walk == RT_WALK_LDS_TIME0, walk == RT_WALK_LDS_TIME0 ? s->ext_lds : s->cam_lds,
                                   d_rays, (uint32_t)n, d_t, d_mat, p.st));
    return p.finish();
}

int rt_hit_rays_stream(int scene, const double* rays, int n, uint64_t seed, double* out_t, int32_t* out_mat,
                       int32_t* out_draws) {
    LOCK_SCENE(s, scene);
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    if (n < 0) return fail("ray count must be >= 0");
    if (n > 0 && (!rays || !out_t || !out_mat || !out_draws)) return fail("null pointer");
    CTX_OF(c, s);
    if (n == 0) return 0;
    Probe p;
    const double* d_rays; double* d_t; int32_t *d_mat, *d_draws;
    TRY(p.begin(c));
    TRY(p.in(rays, (size_t)n * 7, &d_rays));
    TRY(p.out(out_t, n, &d_t));
    TRY(p.out(out_mat, n, &d_mat));
    TRY(p.out(out_draws, n, &d_draws));
    HIPCHK(launch_hit_rays_stream(s->dev, d_rays, (uint32_t)n, (uint32_t)seed, (uint32_t)(seed >> 32), d_t, d_mat,
                                  d_draws, p.st));
    return p.finish();
}

int rt_light_probe(int scene, int n, const double* points, const double* dirs, uint64_t seed, double* out_dir,
                   double* out_pdf, double* out_pdf_dirs, int32_t* out_draws) {
    LOCK_SCENE(s, scene);
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    if (s->dev.light.type == LIGHT_OFF)
        return fail("rt_light_probe: the scene has no light sampling (rt_set_light_sampling / rt_set_light_list)");
    if (n < 0) return fail("rt_light_probe: point count must be >= 0");
    if (!points || !out_dir || !out_pdf || !out_draws) return fail("rt_light_probe: null pointer");
    if ((dirs == nullptr) != (out_pdf_dirs == nullptr)) return fail("rt_light_probe: dirs and out_pdf_dirs are null together");
    CTX_OF(c, s);
    if (n == 0) return 0;
    Probe p;
    const double *d_pts, *d_dirs = nullptr;
    double *d_out, *d_pdf, *d_pdfd = nullptr;
    int32_t* d_draws;
    TRY(p.begin(c));
    TRY(p.in(points, (size_t)n * 3, &d_pts));
    if (dirs) TRY(p.in(dirs, (size_t)n * 3, &d_dirs));
    TRY(p.out(out_dir, (size_t)n * 3, &d_out));
    TRY(p.out(out_pdf, n, &d_pdf));
    if (dirs) TRY(p.out(out_pdf_dirs, n, &d_pdfd));
    TRY(p.out(out_draws, n, &d_draws));
    HIPCHK(launch_light_probe(s->dev, s->d_dev.as<const DevScene>(), scene_exact_libm(*c, *s), d_pts, d_dirs, (uint32_t)n,
                              (uint32_t)seed, (uint32_t)(seed >> 32), d_out, d_pdf, d_pdfd, d_draws, p.st));
    return p.finish();
}

}  // extern "C"

namespace {
// rt_step_rays' host images of a step's state pools: the caller's records at the slots a render's previous
// depth would have left them in (rt_plan.h step_slot), and, after the step, the pools it wrote.
struct StepImage {
    std::vector<RayRec> ray;
    std::vector<PathRec> path;
    std::vector<double> tm;
    std::vector<uint32_t> rng0, pix, key_of, prev, cnt;    // key_of: input slot -> record; prev / cnt: the
    std::vector<uint64_t> sb;                              // previous and this depth's counter rows
    std::vector<HitRec> hit;
    std::vector<LeafInfo> leaves;
};
void pack_step(int n, const double* rays, const double* T_in, const uint32_t* ctr_in, const uint32_t* pix, int depth,
               const PoolLayout& lay, StepImage& h) {
    const size_t cap = lay.cap, scap = lay.scap;
    h.pix.resize(cap);
    for (size_t k = 0; k < cap; ++k) h.pix[k] = pix ? pix[k] : (uint32_t)k;
    h.ray.resize(scap);
    h.path.resize(scap);
    h.tm.assign(scap, 0.0);
    h.rng0.assign(scap, 0u);
    h.prev.assign(kCountsPerIter, 0u);
    h.key_of.assign(scap, 0xFFFFFFFFu);
    std::memset(h.ray.data(), 0, scap * sizeof(RayRec));
    std::memset(h.path.data(), 0, scap * sizeof(PathRec));
    for (size_t k = 0; k < cap; ++k) {
        const size_t slot = step_slot(k, depth, lay, survivor_counts(h.prev.data()));
        h.key_of[slot] = (uint32_t)k;
        const double* r = rays + 7 * k;
        RayRec R{};
        R.ox = r[0]; R.oy = r[1]; R.oz = r[2]; R.dx = r[3]; R.dy = r[4]; R.dz = r[5];
        h.ray[slot] = R;
        if (depth == 0) {
            h.tm[slot] = r[6];
            h.rng0[slot] = ctr_in[k];
        } else {
            PathRec P{};
            P.tr = T_in[3 * k]; P.tg = T_in[3 * k + 1]; P.tb = T_in[3 * k + 2];
            P.wid = (uint32_t)k; P.rng = ctr_in[k];
            h.path[slot] = P;
        }
    }
    h.sb.assign(cap * 3, (uint64_t)RT_STEP_SENTINEL);
}
// the survivors (h.ray / h.path: the next depth's pool) and the hit queues of a wavefront step, per input record
int unpack_step(const Scene* s, const PoolLayout& lay, const bool pt, StepImage& h, int32_t* out_status, double* out_ray,
                double* out_T, uint32_t* out_ctr, double* out_t, int32_t* out_mat, uint32_t* out_survivors) {
    const size_t n = lay.cap, shard_cap = lay.shard_cap;
    for (size_t k = 0; k < n; ++k) { out_t[k] = 0.0; out_mat[k] = -1; }
    uint32_t total = 0;
    for (int x = 0; x < kShards; ++x) {
        const uint32_t cx = shard_count(survivor_counts(h.cnt.data()), x);
        if (cx > shard_cap) return fail("internal: shard overflow");
        total += cx;
        for (uint32_t j = 0; j < cx; ++j) {
            const size_t slot = (size_t)x * shard_cap + j;
            const PathRec& P = h.path[slot];
            if (P.wid >= (uint32_t)n) return fail("rt_step_rays: a survivor carries work id " + std::to_string(P.wid));
            const size_t k = P.wid;
            if ((out_status[k] & 255) < 255) ++out_status[k];
            const RayRec& R = h.ray[slot];
            const double ray6[6] = {R.ox, R.oy, R.oz, R.dx, R.dy, R.dz};
            std::memcpy(out_ray + 6 * k, ray6, sizeof ray6);
            out_T[3 * k] = P.tr; out_T[3 * k + 1] = P.tg; out_T[3 * k + 2] = P.tb;
            out_ctr[k] = P.rng;
        }
    }
    *out_survivors = total;
    const HitBuf hb = hit_buf(h.hit.data(), lay);       // the host copy of the queues, in HitBuf's layout
    for (int mt = 0; mt < 4; ++mt)
        for (int x = 0; x < kShards; ++x) {
            const uint32_t cx = std::min<uint32_t>(shard_count(hit_counts(h.cnt.data(), mt), x), (uint32_t)shard_cap);
            for (uint32_t j = 0; j < cx; ++j) {
                const size_t q = (size_t)x * shard_cap + j;
                int32_t leaf; uint32_t slot; double t;
                if (pt && mt == MAT_LAMBERTIAN) { leaf = hb.hp[q].leaf; slot = hb.hp[q].slot; t = std::nan(""); }
                else { const HitRec& H = hb.h[(size_t)mt * hb.stride + q]; leaf = H.leaf; slot = H.slot; t = H.t; }
                if (slot >= lay.scap || h.key_of[slot] == 0xFFFFFFFFu || leaf < 0 || leaf >= s->dev.n_leaves)
                    return fail("rt_step_rays: a hit queue holds a record of no input path");
                out_t[h.key_of[slot]] = t;
                out_mat[h.key_of[slot]] = h.leaves[leaf].mat;
            }
        }
    return 0;
}
}  // namespace

extern "C" {

/* RT_HAS_STEP_PROBE */
int rt_step_rays(int scene, int n, const double* rays, const double* T_in, const uint32_t* ctr_in, const uint32_t* pix,
                 uint64_t seed, uint32_t smp, int depth, int extend, int mode, int32_t* out_status, double* out_color,
                 double* out_ray, double* out_T, uint32_t* out_ctr, double* out_t, int32_t* out_mat, int32_t* out_inst,
                 uint32_t* out_survivors) {
    LOCK_SCENE(s, scene);
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    if (n < 0) return fail("rt_step_rays: record count must be >= 0");
    if (!rays || !T_in || !ctr_in || !out_status || !out_color || !out_ray || !out_T || !out_ctr || !out_t || !out_mat ||
        !out_inst || !out_survivors)
        return fail("rt_step_rays: null pointer");
    if (depth < 0 || depth > kMaxDepth) return fail("rt_step_rays: depth outside 0.." + std::to_string(kMaxDepth));
    if (extend != RT_STEP_EXTEND_HBM && extend != RT_STEP_EXTEND_LDS)
        return fail("rt_step_rays: unknown extend " + std::to_string(extend));
    if (mode != RT_STEP_STEP && mode != RT_STEP_TAIL && mode != RT_STEP_FUSED)
        return fail("rt_step_rays: unknown mode " + std::to_string(mode));
    if (extend == RT_STEP_EXTEND_LDS && depth == 0)
        return fail("rt_step_rays: the LDS extend serves depth >= 1 only (depth 0 is k_extend or k_camera)");
    if (extend == RT_STEP_EXTEND_LDS && s->ext_lds == 0)
        return fail("rt_step_rays: this scene's time-0 tree does not run from LDS (rt_scene_info.extend_lds_bytes is 0)");
    if (mode == RT_STEP_FUSED) {
        if (depth == 0) return fail("rt_step_rays: the fused curve extend serves depth >= 1 only (depth 0 is one launch of its own)");
        if (extend != RT_STEP_EXTEND_HBM) return fail("rt_step_rays: the fused curve extend is an RT_STEP_EXTEND_HBM launch");
        if (const char* why = curve_fuse_refusal(s->dev, (uint32_t)n))
            return fail(std::string("rt_step_rays: a render of this scene would not take the fused curve extend: ") + why);
    }
    for (int k = 0; k < n; ++k) {
        uint64_t bits;
        if (depth == 0) {
            for (int c = 0; c < 3; ++c)
                if (!(T_in[3 * (size_t)k + c] == 1.0))
                    return fail("rt_step_rays: a depth-0 path has throughput 1 (record " + std::to_string(k) + " has another)");
        } else {
            std::memcpy(&bits, &rays[7 * (size_t)k + 6], sizeof bits);
            if (bits != 0)
                return fail("rt_step_rays: a scattered ray has time +0.0 (record " + std::to_string(k) + " has another time)");
        }
    }
    CTX_OF(c, s);
    std::memset(out_inst, 0, 32 * sizeof(int32_t));
    *out_survivors = 0;
    if (n == 0) return 0;
    Probe p;
    TRY(p.begin(c));
    {
        const char* e = std::getenv("RTAMD_REJECT_CAP");
        HIPCHK(set_test_caps(e ? std::max(0, std::atoi(e)) : 4096, 0u));
    }
    // a render of n paths in one chunk: its pools (either state pool may be the depth's input, so both are
    // carved as pool A), two counter rows (the previous depth's and this one's) and control words
    const PoolLayout lay = pool_layout((size_t)n, 0);
    const size_t cap = lay.cap, scap = lay.scap;
    char *b_a, *b_b, *b_hit;
    double* b_sb;
    uint32_t *b_cnt, *b_pix;
    unsigned long long* ctl;
    TRY(p.alloc(lay.state_a_bytes, &b_a));
    TRY(p.alloc(lay.state_a_bytes, &b_b));
    TRY(p.alloc(lay.hit_bytes, &b_hit));
    TRY(p.alloc(cap * 3, &b_sb));
    TRY(p.alloc(2 * (size_t)kCountsPerIter, &b_cnt));
    TRY(p.alloc(kCtlWords, &ctl));
    TRY(p.alloc(cap, &b_pix));
    const PathState A = carve_state(b_a, scap, true), B = carve_state(b_b, scap, true);
    const PathState& cur = (depth & 1) ? B : A;         // a chunk starts in pool A and swaps every depth
    const PathState& nxt = (depth & 1) ? A : B;
    uint32_t* cnt = b_cnt + kCountsPerIter;

    StepImage h;
    pack_step(n, rays, T_in, ctr_in, pix, depth, lay, h);
    hipStream_t st = p.st;
    HIPCHK(hipMemcpyAsync(cur.ray, h.ray.data(), scap * sizeof(RayRec), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cur.path, h.path.data(), scap * sizeof(PathRec), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cur.tm, h.tm.data(), scap * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cur.rng0, h.rng0.data(), scap * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(nxt.ray, 0, scap * sizeof(RayRec), st));
    HIPCHK(hipMemsetAsync(nxt.path, 0xFF, scap * sizeof(PathRec), st));
    HIPCHK(hipMemcpyAsync(b_pix, h.pix.data(), cap * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b_sb, h.sb.data(), lay.sb_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b_cnt, 0, 2 * kCountsPerIter * sizeof(uint32_t), st));
    HIPCHK(hipMemcpyAsync(b_cnt, h.prev.data(), kCountsPerIter * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b_hit, 0, lay.hit_bytes, st));
    HIPCHK(hipMemsetAsync(ctl, 0, kCtlWords * sizeof(unsigned long long), st));

    RenderParams rp{};
    rp.nx = (uint32_t)n; rp.ny = 1u; rp.npix = (uint32_t)n;
    rp.inx = 1.0 / (double)n; rp.iny = 1.0;
    rp.spp0 = smp; rp.k0 = (uint32_t)seed; rp.k1 = (uint32_t)(seed >> 32);
    rp.pixlist = b_pix;
    rp.sb = b_sb;
    rp.B = (uint32_t)n;
    rp.compact = 0u;
    rp.exact_libm = scene_exact_libm(*c, *s) ? 1u : 0u;
    // the survivor view of the previous depth (raygen's output is contiguous)
    const QView view = depth == 0 ? QView{nullptr, (uint32_t)scap} : QView{survivor_counts(b_cnt), (uint32_t)lay.shard_cap};
    const ExtendPath path = extend == RT_STEP_EXTEND_LDS ? ExtendPath::LDS : ExtendPath::HBM;
    const bool point_hits = s->point_hits && !point_hits_off(), pt = point_records(point_hits, path);
    const StepArgs a{rp, cur, nxt, view, (uint32_t)n, depth, lay, b_hit, cnt, ctl, 0, point_hits, st};
    // the launches are the render's (enqueue_tail / enqueue_iteration); the rows name the instances they take
    int extend_inst = EXTEND_PER_RAY;
    if (mode == RT_STEP_FUSED) {
        TRY(enqueue_iteration(*s, a, path, true, nullptr, &extend_inst));
        if (extend_inst != EXTEND_CURVES_FUSED && extend_inst != EXTEND_CURVES_FUSED_EXACT)
            return fail("internal: the fused curve extend was not launched");
    } else if (mode == RT_STEP_TAIL) {
        const FinishInst fi = finish_instance(s->dev, rp, tree0_budget(*s));
        const int32_t row[6] = {1, fi.f, fi.tl, fi.ls, fi.solo ? 1 : 0, fi.ex ? 1 : 0};
        std::memcpy(out_inst, row, sizeof row);
        TRY(enqueue_tail(*s, a, nullptr));
    } else {
        for (int mt = 0; mt < 4; ++mt) {
            if (!(s->dev.mat_mask & (1 << mt))) continue;
            const ShadeInst si = shade_instance(mt, s->dev, rp, pt && mt == MAT_LAMBERTIAN);
            const int32_t row[6] = {1, si.tl, si.ls, si.ll ? 1 : 0, si.ex ? 1 : 0, si.pt ? 1 : 0};
            std::memcpy(out_inst + 8 * mt, row, sizeof row);
        }
        TRY(enqueue_iteration(*s, a, path, false, nullptr, &extend_inst));
    }
    out_inst[7] = extend_inst;
    // read everything back
    h.cnt.resize(kCountsPerIter);
    p.later(h.cnt.data(), cnt, (size_t)kCountsPerIter);
    p.later(h.sb.data(), reinterpret_cast<const uint64_t*>(b_sb), cap * 3);
    if (mode == RT_STEP_STEP) {
        h.hit.resize(5 * scap);
        h.leaves.resize((size_t)std::max(0, s->dev.n_leaves));
        p.later(h.ray.data(), nxt.ray, scap);
        p.later(h.path.data(), nxt.path, scap);
        p.later(reinterpret_cast<char*>(h.hit.data()), b_hit, lay.hit_bytes);
        if (!h.leaves.empty()) p.later(h.leaves.data(), s->dev.leaves, h.leaves.size());
    }
    TRY(p.finish());
    unsigned long long h_ctl[kCtlWords] = {0, 0, 0, 0};
    HIPCHK(hipMemcpy(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost));
    if (h_ctl[kCtlLdsErr]) return fail("internal: a persistent kernel's LDS allocation was too small (flags " +
                                       std::to_string(h_ctl[kCtlLdsErr]) + ")");
    for (size_t k = 0; k < cap; ++k) {
        bool wrote = false;
        for (int c3 = 0; c3 < 3; ++c3) wrote = wrote || h.sb[3 * k + c3] != (uint64_t)RT_STEP_SENTINEL;
        out_status[k] = wrote ? RT_STEP_WROTE : 0;
        std::memcpy(out_color + 3 * k, &h.sb[3 * k], 3 * sizeof(double));
    }
    if (mode == RT_STEP_FUSED) *out_survivors = (uint32_t)h_ctl[kCtlFuseSegs];
    if (mode != RT_STEP_STEP) return 0;
    return unpack_step(s, lay, pt, h, out_status, out_ray, out_T, out_ctr, out_t, out_mat, out_survivors);
}

int rt_curve_depth_probe(int ctx, int n, const double* cps, const double* eps8, int32_t* out_depth) {
    LOCK_CTX(c, ctx);
    if (n < 0) return fail("curve count must be >= 0");
    if (n == 0) return 0;
    if (!cps || !eps8 || !out_depth) return fail("null pointer");
    Probe p;
    const double *d_cps, *d_eps;
    int32_t* d_out;
    TRY(p.begin(c, false));
    TRY(p.in(cps, (size_t)n * 12, &d_cps));
    TRY(p.in(eps8, n, &d_eps));
    TRY(p.out(out_depth, n, &d_out));
    HIPCHK(launch_curve_depth(d_cps, d_eps, (uint32_t)n, d_out, p.st));
    return p.finish();
}

int rt_f64_probe(int ctx, int kind, const double* in, int n, double* out) {
    LOCK_CTX(c, ctx);
    if (kind < RT_F64_SQRT_MID || kind > RT_F64_RCP_CORE) return fail("rt_f64_probe: unknown kind " + std::to_string(kind));
    if (n < 0) return fail("value count must be >= 0");
    if (n == 0) return 0;
    if (!in || !out) return fail("null pointer");
    Probe p;
    const double* d_in;
    double* d_out;
    TRY(p.begin(c, false));
    TRY(p.in(in, (size_t)n, &d_in));
    TRY(p.out(out, (size_t)n, &d_out));
    HIPCHK(launch_f64_probe(kind, d_in, (uint32_t)n, d_out, p.st));
    return p.finish();
}

}  // extern "C"
