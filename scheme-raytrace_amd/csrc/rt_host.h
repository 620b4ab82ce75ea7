// rt_host.h — what librtamd's host translation units share: the object model behind the handles of
// include/rt.h (rt_model.h) with its device side, the handle registry, error reporting, the entry
// points' common prologues and the functions the units call in each other.
//   rt_scene.cpp     contexts, options, the scene builder, statistics
//   rt_build.cpp     the host scene of a commit: flattening, BVH builds, records (build_scene; no HIP)
//   rt_commit.cpp    its upload and the device-dependent sizing (commit_scene)
//   rt_render.cpp    the render scheduler (render_impl; its arithmetic: rt_plan.h) and the render / resolve entry points
//   rt_probe.cpp     the probe entry points (rt_hit_rays*, rt_light_probe, rt_step_rays, rt_curve_depth_probe, rt_f64_probe)
//   rt_gather.cpp    the frame-end gather (RCCL and in-process)
//   rt_adaptive.cpp  adaptive sampling
//   rt_features.cpp  first-hit feature buffers
//   rt_denoise.cpp   the variance-guided a-trous filter
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rt.h"
#include "rt_device.h"
#include "rt_model.h"
#include "rt_plan.h"

namespace rtamd {

// rt_last_error's text for the calling thread (rt_scene.cpp); returns 1, the entry points' error code
int fail(const std::string& msg);

#define HIPCHK(expr)                                                                   \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};


// A lane = one path pool + stream.  render_impl deals the sample chunks of a
// render to the lanes round-robin and keeps them in flight together, so the
// long, narrow tail of one chunk (its last few paths bouncing to depth 100)
// overlaps the wide first iterations of the next one instead of leaving the
// chip mostly idle.  Accumulation stays in chunk (= sample) order.
struct Lane {
    DevBuf st_a, st_b, hit, sb, counts, seg_tail;      // (rt_plan.h PoolLayout; seg_tail: the LaneCtl words)
    uint32_t* h_counts = nullptr;              // pinned survivor counts, one row per iteration
    hipStream_t stream = nullptr;
    hipEvent_t ev_cnt = nullptr;               // the last iteration's survivor counts are on the host
    hipEvent_t ev_acc = nullptr;               // this lane's last accumulate
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};             // profiling: extend / shade brackets
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_fin;      // profiling: tail kernel brackets
    size_t n_fin = 0;
    // the chunk in flight
    enum State { IDLE, RUNNING, DONE } state = IDLE;
    int chunk = -1, depth = 0;
    int index = 0;                             // the lane's position in Context::lanes
    bool fused_camera = false;                 // depth 0 runs k_camera (no raygen pass)
    uint32_t n = 0, S = 0;
    uint64_t seq = 0;                          // enqueue order of the pending iteration
    RenderParams rp{};
    PathState A{}, B{}, *cur = nullptr, *nxt = nullptr;
    QView view{nullptr, 0};
    ~Lane() {
        if (h_counts) (void)hipHostFree(h_counts);
        for (hipEvent_t e : {ev_cnt, ev_acc, ev[0], ev[1], ev[2]}) if (e) (void)hipEventDestroy(e);
        for (auto& pr : ev_fin) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// The frame-end gather's layout for one frame size and world (rt_gather_layout): per rank its shard's
// pixel count and the offset of its pixels in the ranks' concatenated pixel lists (rt_shard_pixels order,
// ranks in order).  The root (rank 0) also keeps that concatenated list on the device and a receive
// buffer for the other ranks' compact accumulators: rank r's lands at doubles recv_at(r).  Both gathers —
// over RCCL (rt_gather_shards) and within one process (rt_gather_shards_local) — fill it the same way and
// place it with the same kernel (gather_place).
struct GatherPlan {
    int nx = -1, ny = -1, world = 0;
    bool root = false;
    std::vector<int64_t> count, off;
    DevBuf pix, recv;
    size_t recv_at(int r) const { return 3 * (size_t)(off[r] - count[0]); }
    int64_t others() const { return off[world - 1] + count[world - 1] - count[0]; }
};

// A context owns the render lanes' path pools: every scene rendered on it
// shares them (the C ABI renders one scene at a time per context), so a
// second scene does not take a second 65 % of device memory.
// The render schedule's knobs are options of the context (rt_context_set_option,
// include/rt.h RT_OPT_*), 0 = the library's automatic choice.
struct Context {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf accum_tmp, img_tmp;
    size_t pool_cap = 0;                       // paths per chunk (max_paths), fixed at the first render
    int pool_lanes = 0;                        // the lanes pool_cap was sized for
    std::unique_ptr<Lane> lanes[kLanes];       // rt_context_release_pools frees them
    int64_t opt_lanes = 0;                     // RT_OPT_LANES (0: 2, or 1 for curve-kernel scenes)
    int64_t opt_max_paths = 0;                 // RT_OPT_MAX_PATHS (0: sized from free memory)
    int64_t opt_tail_paths = 0;                // RT_OPT_TAIL_PATHS (0: 32768)
    int64_t opt_tail_div = 0;                  // RT_OPT_TAIL_DIV (0: 256)
    bool wavefront_only = false;               // RT_OPT_TAIL_OFF: no tail kernel (tests, A/B)
    GatherPlan gplan;                          // rt_gather_shards_local's plan (the frame size last gathered)
    int64_t opt_exact_libm = RT_LIBM_AUTO;     // RT_OPT_EXACT_LIBM: the bounce directions' sin / cos
    // adaptive sampling: the two active-pixel lists a render alternates between, the selection's block
    // counts / offsets and its two result words (with the range check's word after them), and the host
    // entry point's device copies of accum2 / count
    DevBuf sel_list[2], sel_scratch, sel_words, accum2_tmp, count_tmp;
    // denoiser scratch: the ping-pong signal buffers (32 B per pixel each) and the guide buffer (40 B per pixel),
    // sized at first use; rt_context_release_pools frees them
    DevBuf dn_signal[2], dn_guide;
};

struct Scene : SceneDesc {       // the builder's record (rt_model.h) and what a commit made of it
    int ctx = -1;
    bool committed = false;

    // flattened + uploaded
    DevScene dev{};
    DevBuf d_sph, d_msph, d_rect, d_bez, d_klein, d_med, d_bgroups, d_groups, d_chains, d_leaves, d_mats, d_texs, d_ranvec, d_perm, d_bvh2, d_bleaf;
    DevBuf d_fbvh2, d_fbleaf, d_fsph, d_fid;      // time-0 BVH (commit_scene)
    DevBuf d_bvh4, d_stk_ovf, d_bez_ring, d_fuse_ring;         // curve trees: BVH4, the walk's stack overflow, rings
    DevBuf d_dev;                                  // a device copy of `dev` (kernels that take the scene by pointer)
    DevBuf d_leaf_cls;
    DevBuf d_order;
    DevBuf d_teximg;                               // the image textures' texels
    DevBuf d_gleaf, d_leaf_pos, d_g0bvh2, d_g0bleaf, d_rot;   // generic tree leaves (DevScene::gleaf)
    DevBuf d_tri, d_triuv, d_trinrm;               // triangles, their texture coordinates and shading normals (DevScene::tri)
    DevBuf d_lights;                               // the light list's records (DevScene::lights)
    rt_tree_info tree{};                           // rt_get_tree_info's record, filled by commit_scene
    size_t ext_lds = 0;                            // k_extend_lds: LDS bytes (0 = not used) and grid cap
    uint32_t ext_lds_blocks = 0;
    size_t cam_lds = 0;                            // k_camera (fused raygen + depth-0 extend), same
    uint32_t cam_blocks = 0;
    // those two kernels queue lambertian hits as point records (rt_device.h HitPt): a SOLO world whose every
    // leaf is a sphere or moving sphere under no instance chain, checked at the commit (RTAMD_NO_POINT_HITS,
    // read per render, switches the records off)
    bool point_hits = false;
    // render buffers (the lanes' path pools belong to the context)
    DevBuf pixlist;
    int pix_nx = -1, pix_ny = -1, pix_y0 = -1, pix_y1 = -1, pix_shard = -1, pix_nshard = -1;
    uint32_t pix_n = 0;
    bool profiling = false;
    rt_stats stats{};
    double commit_ms = 0.0, commit_upload_ms = 0.0;   // rt_scene_commit: wall time, of it device allocation + copies
    double commit_sah_ms = 0.0;                        // ... and the SAH builds (commit_threads host threads)
    int commit_threads = 1;
};

// ------------------------------------------------------------ registry
// (rt_scene.cpp; communicators live in rt_gather.cpp, the only unit that knows RCCL)
extern std::mutex g_mu;
extern std::map<int, std::unique_ptr<Context>> g_ctx;
extern std::map<int, std::unique_ptr<Scene>> g_scene;

inline Context* get_ctx(int h) {
    auto it = g_ctx.find(h);
    return it == g_ctx.end() ? nullptr : it->second.get();
}
inline Scene* get_scene(int h) {
    auto it = g_scene.find(h);
    return it == g_scene.end() ? nullptr : it->second.get();
}

// ----------------------------------------------------------- prologues
// An entry point's first steps.  The LOCK_* ones hold the registry lock for the rest of the call.
#define LOCK_SCENE(s, h)                                                        \
    std::lock_guard<std::mutex> lk_(g_mu);                                      \
    Scene* s = get_scene(h);                                                    \
    if (!s) return fail("invalid scene handle");
#define LOCK_CTX(c, h)                                                          \
    std::lock_guard<std::mutex> lk_(g_mu);                                      \
    Context* c = get_ctx(h);                                                    \
    if (!c) return fail("invalid context handle");
// the scene builder's: a committed scene takes no more changes
#define SCENE_OR_FAIL(s, h)                                                     \
    std::lock_guard<std::mutex> lk_(g_mu);                                      \
    Scene* s = get_scene(h);                                                    \
    if (!s) return fail("invalid scene handle " + std::to_string(h));            \
    if (s->committed) return fail("scene " + std::to_string(h) + " already committed");
// scene s's context
#define CTX_OF(c, s)                                                            \
    Context* c = get_ctx(s->ctx);                                               \
    if (!c) return fail("scene's context was destroyed");
// context c's device made current, and st = the caller's stream or, for null, the context's
#define CTX_STREAM(c, st, stream)                                               \
    HIPCHK(hipSetDevice(c->device));                                            \
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;

inline int check_tex(Scene* s, int t) {
    if (t < 0 || t >= (int)s->texs.size()) return fail("invalid texture id " + std::to_string(t));
    return 0;
}
inline int check_mat(Scene* s, int m) {
    if (m < 0 || m >= (int)s->mats.size()) return fail("invalid material id " + std::to_string(m));
    return 0;
}
inline int check_obj(Scene* s, int o) {
    if (o < 0 || o >= (int)s->objs.size()) return fail("invalid object id " + std::to_string(o));
    return 0;
}
inline int check_frame(int nx, int ny) {
    if (nx <= 0 || ny <= 0) return fail("image size must be positive");
    if ((uint64_t)nx * (uint64_t)ny >= (1ull << 31)) return fail("image too large");
    return 0;
}

// ------------------------------------------------------------- between units
// rt_commit.cpp: build the host scene of the object tree under `world` (rt_build.h), upload it
int commit_scene(Scene* s, int world);

// The pixels a render covers: rows [y0, y1) of the frame (trace-all: every
// row; trace-line, main.scm:452-469: one row), restricted to shard `shard` of
// `nshard` interleaved 16x16 tiles (the diagonal deal of make_pixlist: tile
// (x, y) -> shard (x + k y) % nshard).  Listed tile by tile in row-major
// tile order, pixel j = y*nx + x.
struct PixSel { int y0, y1, shard, nshard; };
PixSel full_frame(int ny);
std::vector<uint32_t> make_pixlist(int nx, int ny, const PixSel& ps);

// A render's pixels on the device: n unique entries pix[q] = image pixel j < nx*ny, in the order the
// samples are laid out.  The accumulator is indexed by j, or by q when `compact`.  A render also adds
// its samples' squares to accum2 and their number to count where given (each nullable, never compact).
struct PixSet {
    const uint32_t* pix;
    uint32_t n;
    bool compact;
    double* accum2;
    uint32_t* count;
};
// rt_render.cpp: passes spp_begin .. spp_begin+spp_count-1 of the pixels of px into accum
int render_impl(Scene* s, int nx, int ny, const PixSet& px, int spp_begin, int spp_count, uint64_t seed,
                double* accum, hipStream_t stream);
// rt_render.cpp: the pixels `ps` selects as a PixSet, the scene's cached device list (uploaded again when
// the selection differs from the cached one); and rt_last_error's text for a device fault word
int pixset_of(Scene* s, int nx, int ny, const PixSel& ps, bool compact, PixSet* out);
std::string fault_text(uint32_t f);

// rt_render.cpp: what a scene's renders decide from the context and the environment, for the probes too.
// the libm mode a scene's renders (and rt_light_probe) take under the context's RT_OPT_EXACT_LIBM
bool scene_exact_libm(const Context& c, const Scene& s);
// The persistent curve kernels serve scenes whose world BVH holds every curve (launch_extend)
bool curve_kernel_scene(const DevScene& d);
// RTAMD_NO_POINT_HITS (A/B, tests; read per render): every hit queue keeps HitRec
bool point_hits_off();
// null when a depth >= 1 launch of n rays takes the fused curve extend (k_extend_curves<FUSE>), else why not
const char* curve_fuse_refusal(const DevScene& d, uint32_t n);

// One step of a chunk as renders and rt_step_rays enqueue it.  The closest-hit launch of a wavefront
// iteration: k_camera (raygen + the first hit, depth 0), k_extend_lds (depth >= 1, the time-0 tree in LDS) or
// k_extend / the persistent curve kernel.
enum class ExtendPath { CAMERA, LDS, HBM };
// point records are what the SOLO LDS kernels write, so a render can mix the two formats across depths:
// one of those kernels switched off, or a chunk whose depth 0 is k_raygen + k_extend
inline bool point_records(bool point_hits, ExtendPath path) {
    return point_hits && (path == ExtendPath::CAMERA || path == ExtendPath::LDS);
}
// LDS bytes the tail kernel's time-0 tree may take
inline size_t tree0_budget(const Scene& s) { return s.ext_lds ? (size_t)32 << 10 : 0; }
struct StepArgs {
    const RenderParams& rp;
    const PathState& cur;                      // the n live paths, seen through `in` (the previous depth's
    const PathState& nxt;                      // survivors; contiguous at depth 0), and where survivors go
    QView in;
    uint32_t n;
    int depth;
    const PoolLayout& lay;
    void* hit;                                 // the hit queues' buffer (lay.hit_bytes)
    uint32_t* counts;                          // this depth's counter row (kCountsPerIter words, zero)
    unsigned long long* ctl;                   // the LaneCtl words
    int lane;                                  // the render lane's index: its region of the curve walk's buffers
    bool point_hits;                           // the scene's, unless switched off (point_hits_off)
    hipStream_t stream;
};
// extend + the shade of every material the scene has; may_fuse: a curve-kernel scene's depth >= 1 may take
// the fused curve extend, which shades its hits itself; ev: null, or three events recorded around the two;
// extend_inst: null, or where launch_extend leaves the ExtendInst it took (ExtendPath::HBM only)
int enqueue_iteration(const Scene& s, const StepArgs& a, ExtendPath path, bool may_fuse, const hipEvent_t* ev,
                      int* extend_inst = nullptr);
// the tail kernel, which finishes the n paths; ev: null, or two events recorded around it
int enqueue_tail(const Scene& s, const StepArgs& a, const std::pair<hipEvent_t, hipEvent_t>* ev);

}  // namespace rtamd
