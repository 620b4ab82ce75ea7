// rt_render.cpp — the wavefront driver loop (raygen → [extend → shade/compact]* → accumulate) over the
// context's render lanes, and the C ABI's render, row, shard, probe and resolve entry points.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_host.h"
#include "rt_launch.h"

using namespace rtamd;

// -------------------------------------------------------------- render
namespace {
// The diagonal tile deal's row stride: the smallest odd prime coprime with the shard count (3 for every
// count not divisible by 3, so 1, 2, 4 and 8 shards keep the round-5 deal; 5 for 3 or 6 shards).  With a
// stride sharing a factor with the count, shard r would only ever get the columns tx = r mod that factor.
int tile_stride(const int nshard) {
    for (int k : {3, 5, 7, 11, 13, 17, 19, 23, 29, 31})
        if (nshard % k != 0) return k;
    return 37;                               // a product of the primes to 31 exceeds any int shard count
}
}  // namespace

namespace rtamd {
PixSel full_frame(int ny) { return PixSel{0, ny, 0, 1}; }
std::vector<uint32_t> make_pixlist(int nx, int ny, const PixSel& ps) {
    const int T = 16;
    const int tx = (nx + T - 1) / T, ty = (ny + T - 1) / T;
    std::vector<uint32_t> out;
    out.reserve((size_t)nx * (size_t)(ps.y1 - ps.y0) / (size_t)ps.nshard + T * T);
    // tile (x, y) belongs to shard (x + k y) % nshard, k = tile_stride(nshard).  Plain t % nshard degenerates
    // into vertical 16-px stripes whenever nshard divides the tiles per row (C2: 120, C4: 64): every rank then
    // renders the same columns of every row, and the Cornell box's walls are not alike (shard balance at C4,
    // one GPU per shard: max / mean 1.0385 for 8 shards, 1.0247 for 4; profiles/r05/balance.log).  The
    // diagonal deal with k coprime to nshard gives every shard one tile of each nshard consecutive ones along
    // a row and along a column.
    const int k = tile_stride(ps.nshard);
    for (int t = 0; t < tx * ty; ++t) {
        if (((t % tx) + k * (t / tx)) % ps.nshard != ps.shard) continue;
        const int bx = (t % tx) * T, by = (t / tx) * T;
        for (int yy = std::max(by, ps.y0); yy < std::min(std::min(by + T, ny), ps.y1); ++yy)
            for (int xx = bx; xx < std::min(bx + T, nx); ++xx) out.push_back((uint32_t)(yy * nx + xx));
    }
    return out;
}
}  // namespace rtamd

namespace rtamd {
std::string fault_text(uint32_t f) {
    std::string m = "device fault (flags " + std::to_string(f) + "):";
    if (f & RT_FAULT_REJECT) m += " a rejection sampler exceeded its attempt cap;";
    if (f & RT_FAULT_CURVE) m += " a curve walk exceeded its step bound or a curve needed more subdivision levels than the walk supports;";
    if (f & RT_FAULT_PATH) m += " a persistent kernel's path or ray exceeded its step bound;";
    if (f & RT_FAULT_SHARD) m += " a queue shard overflowed (the append was dropped);";
    if (f & RT_FAULT_LDS) m += " a persistent kernel's LDS allocation was too small;";
    return m;
}
}  // namespace rtamd

namespace rtamd {
bool scene_exact_libm(const Context& c, const Scene& s) {
    return c.opt_exact_libm == RT_LIBM_EXACT ||
           (c.opt_exact_libm == RT_LIBM_AUTO && (s.dev.n_bez > 0 || s.dev.has_noise_tex));
}
bool curve_kernel_scene(const DevScene& d) {
    return d.n_bez > 0 && d.bvh_has_bez && d.bez_groups == 0 && d.n_med == 0 && d.n_klein == 0;
}
bool point_hits_off() { return std::getenv("RTAMD_NO_POINT_HITS") != nullptr; }
}  // namespace rtamd

namespace {
// the path-pool cap (rt_plan.h pool_cap_for) for the device's free memory now
size_t max_paths(const Context& c, const int lanes) {
    size_t free_b = 0, total_b = 0;
    if (c.opt_max_paths <= 0 && !(hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)) {
        (void)hipGetLastError();
        free_b = 0;
    }
    return pool_cap_for(free_b, lanes, c.opt_max_paths);
}
int lanes_wanted(const Context& c) {   // RT_OPT_LANES: path pools kept in flight (1 = no overlap)
    return c.opt_lanes > 0 ? (int)std::min<int64_t>(c.opt_lanes, kLanes) : 2;
}
// Scenes whose world BVH holds curves run the persistent curve kernel, whose
// grid fills the chip by itself: a second lane's kernels only queue behind it
// and its narrow tails, so one lane is faster (C5 at 64 spp: 200.3 vs 164.1
// Mrays/s, profiles/r03/ab/ab_lanes_c5.log; round 5, 398.0 vs 304.9 at 32 spp and
// 409.1 vs 306.5 at 256 spp, profiles/r05/ab/lanes/).  RT_OPT_LANES overrides.
int lanes_for(const Context& c, const DevScene& d) {
    if (c.opt_lanes > 0) return lanes_wanted(c);
    return curve_kernel_scene(d) ? 1 : lanes_wanted(c);
}

// The fused curve extend (rt_kernels.hip k_extend_curves<FUSE>: every depth >= 1 of a chunk in one launch)
// serves curve-kernel scenes whose hits it can shade itself: no Perlin tables (the fused kernel keeps no
// LDS copy of them), no image textures (it carries no u, v) and no light mixture (f2).  It pays where the per-depth launches are small: each
// persistent launch drains once (~1.1 ms at C5), which a depth-1 launch of n rays amortises over n.  C5,
// fused vs one launch per depth (profiles/r05/ab/fuse/): 1 spp 275.2 vs 189.5 Mrays/s, 8 spp 380.4 vs
// 356.1, 32 spp 394.8 vs 395.8, 256 spp (128-spp chunks) 402.9 vs 407.8 — so it is taken for depth-1
// launches of at most kFuseMaxRays rays (full frames below ~16 spp per chunk, e.g. the progressive
// one-pass-at-a-time loop, main.scm:533-544).  RTAMD_CURVE_FUSE=0 / 1: never / always (A/B, tests).
// (2^23 / 2^25: the same within noise at 32 and 256 spp, profiles/r06/fuse_max/)
constexpr uint32_t kFuseMaxRays = 1u << 24;
}  // namespace

namespace rtamd {
const char* curve_fuse_refusal(const DevScene& d, const uint32_t n) {
    if (!curve_kernel_scene(d)) return "the scene's renders do not take the persistent curve kernel";
    if (!curve_persistent()) return "RTAMD_CURVE_BLOCKS=0 selects the per-ray kernel";
    if (d.has_perlin) return "the scene has Perlin textures";
    if (d.has_image_tex) return "the scene has image textures";
    if (d.light.type != LIGHT_OFF) return "the scene samples a light";
    if (!d.fuse_ring) return "the scene has no hand-off ring";
    if (d.n_leaves >= (1 << kFuseLeafBits) - 1) return "the scene has too many leaves";    // FuseHit packs leaf + 1 in 25 bits
    const char* e = std::getenv("RTAMD_CURVE_FUSE");   // read per render: tests switch it inside one process
    if (e && e[0] == '0') return "RTAMD_CURVE_FUSE=0";
    if (e && e[0] == '1') return nullptr;
    return n <= kFuseMaxRays ? nullptr : "the launch has more rays than the fused extend takes";
}
}  // namespace rtamd

namespace {
bool curve_fuse(const DevScene& d, const uint32_t n) { return curve_fuse_refusal(d, n) == nullptr; }

// What every render checks first.  render_sel runs it ahead of its own checks, so the same error wins
// however the pixels are given.
int check_render(const Scene* s, int nx, int ny, int spp_begin, int spp_count) {
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    if (nx <= 0 || ny <= 0) return fail("image size must be positive");
    if (spp_begin < 0 || spp_count < 0) return fail("spp_begin/spp_count must be >= 0");
    if ((uint64_t)spp_begin + (uint64_t)spp_count > 0xFFFFFFFFull) return fail("sample index out of range");
    return 0;
}
}  // namespace

namespace rtamd {
int enqueue_iteration(const Scene& s, const StepArgs& a, const ExtendPath path, const bool may_fuse, const hipEvent_t* ev,
                      int* extend_inst) {
    const HitBuf hit = hit_buf(a.hit, a.lay);
    const uint32_t shard_cap = (uint32_t)a.lay.shard_cap;
    const bool pt = point_records(a.point_hits, path);
    bool fused = false;
    if (ev) HIPCHK(hipEventRecord(ev[0], a.stream));
    if (path == ExtendPath::CAMERA)             // raygen + first closest hit in one kernel
        HIPCHK(launch_camera(s.dev, a.rp, a.cur, a.n, hit, pt, shard_cap, a.counts, s.cam_lds, s.cam_blocks,
                             a.ctl + kCtlLdsErr, a.stream));
    else if (path == ExtendPath::LDS)           // every ray of a depth >= 1 launch has time +0.0
        HIPCHK(launch_extend_lds(s.dev, a.rp, a.cur, a.in, a.n, hit, pt, shard_cap, a.counts, s.ext_lds_blocks,
                                 a.ctl + kCtlLdsErr, a.stream));
    else {
        // the curve walk's stack overflow area: one region per render lane (lanes run concurrently)
        DevScene dl = s.dev;
        if (dl.stk_ovf) dl.stk_ovf += (size_t)a.lane * dl.ovf_lanes * (size_t)(dl.stack4 - dl.lds4);
        if (dl.bez_ring) dl.bez_ring += (size_t)a.lane * dl.ring_waves * kBezRing * 16u;
        if (dl.fuse_ring) dl.fuse_ring += (size_t)a.lane * dl.ring_waves * kFuseWaveBytes;
        // the fused curve extend (k_extend_curves<FUSE>): every depth from 1 on in this one launch
        CurveFuse fz{a.ctl + kCtlFuseSegs, (uint32_t)a.depth};
        fused = may_fuse && a.depth > 0 && curve_fuse(s.dev, a.n);
        HIPCHK(launch_extend(dl, s.d_dev.as<const DevScene>(), a.rp, a.cur, a.in, a.n, hit, shard_cap, a.counts,
                             a.depth == 0, reinterpret_cast<unsigned int*>(a.ctl + kCtlClaim),
                             fused ? &fz : nullptr, a.stream, extend_inst));
    }
    if (ev) HIPCHK(hipEventRecord(ev[1], a.stream));
    for (int mt = 0; mt < 4 && !fused; ++mt) {         // (a fused launch shades its hits itself: no queues)
        if (!(s.dev.mat_mask & (1 << mt))) continue;
        const QView qv{hit_counts(a.counts, mt), shard_cap};
        HIPCHK(launch_shade(mt, s.dev, s.d_dev.as<const DevScene>(), a.rp, a.cur, hit, pt, qv, a.n, a.nxt,
                            survivor_counts(a.counts), shard_cap, (uint32_t)a.depth, a.stream));
    }
    if (ev) HIPCHK(hipEventRecord(ev[2], a.stream));
    return 0;
}

int enqueue_tail(const Scene& s, const StepArgs& a, const std::pair<hipEvent_t, hipEvent_t>* ev) {
    if (ev) HIPCHK(hipEventRecord(ev->first, a.stream));
    HIPCHK(hipMemsetAsync(a.ctl + kCtlClaim, 0, sizeof(unsigned long long), a.stream));
    HIPCHK(launch_finish(s.dev, s.d_dev.as<const DevScene>(), a.rp, a.cur, a.in, a.n, a.ctl + kCtlSegments,
                         tree0_budget(s), (uint32_t)a.depth, a.stream));
    if (ev) HIPCHK(hipEventRecord(ev->second, a.stream));
    return 0;
}
}  // namespace rtamd

namespace {
// The lanes of a render made ready: streams, events, pools of `lay` (kept from earlier renders when large
// enough), control words cleared.  Each lane's stream waits for ev_in, the caller's prior work.
int prepare_lanes(Context* c, const Scene* s, const int nlanes, const PoolLayout& lay, hipEvent_t ev_in) {
    for (int li = 0; li < nlanes; ++li) {
        if (!c->lanes[li]) c->lanes[li].reset(new Lane());
        c->lanes[li]->index = li;
        Lane& L = *c->lanes[li];
        if (!L.stream) HIPCHK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        if (!L.ev_cnt) HIPCHK(hipEventCreateWithFlags(&L.ev_cnt, hipEventDisableTiming));
        if (!L.ev_acc) HIPCHK(hipEventCreateWithFlags(&L.ev_acc, hipEventDisableTiming));
        if (s->profiling && !L.ev[0]) for (auto& e : L.ev) HIPCHK(hipEventCreate(&e));
        HIPCHK(L.st_a.ensure(lay.state_a_bytes));
        HIPCHK(L.st_b.ensure(lay.state_b_bytes));
        HIPCHK(L.hit.ensure(lay.hit_bytes));
        HIPCHK(L.sb.ensure(lay.sb_bytes));
        HIPCHK(L.counts.ensure(kIters * kCountsPerIter * sizeof(uint32_t)));
        HIPCHK(L.seg_tail.ensure(kCtlWords * sizeof(unsigned long long)));
        if (!L.h_counts) HIPCHK(hipHostMalloc((void**)&L.h_counts, kIters * kCountsPerIter * sizeof(uint32_t)));
        HIPCHK(hipStreamWaitEvent(L.stream, ev_in, 0));
        HIPCHK(hipMemsetAsync(L.seg_tail.p, 0, kCtlWords * sizeof(unsigned long long), L.stream));
        L.A = carve_state(L.st_a.p, lay.scap, true);
        L.B = carve_state(L.st_b.p, lay.scap, false);
        L.state = Lane::IDLE;
        L.n_fin = 0;
    }
    return 0;
}

// One render over prepared lanes: its chunks dealt to the lanes, each stepped depth by depth as its
// survivor counts arrive, and accumulated in chunk order.
struct RenderRun {
    Context* c;
    Scene* s;
    int nx, ny;
    const PixSet& px;
    int spp_begin, spp_count;
    double* accum;
    RenderPlan plan;
    PoolLayout lay;
    TailOpts tail;
    uint32_t k0, k1;                            // the seed's halves
    // RT_OPT_EXACT_LIBM: auto = exact in scenes with curves or noise / marble textures ("libm"):
    // C3 (marble) frame rows with the device library's sin / cos were 0.79 % of pixels off by more than 1e-9;
    // exact there costs 1.7 % (profiles/r06/c3_libm/).  The cover scene keeps the device's: exact would cost it
    // 1.4 % (profiles/r06/c2_libm/) for 26 of 15 360 horizon pixels at 256 passes, all within 1e-7
    bool exact_libm;
    // point records for the lambertian queue of the launches the SOLO LDS kernels make (rt_device.h HitPt)
    bool point_hits;
    uint64_t seq = 0;
    int next_chunk = 0, next_acc = 0;
    Lane* last_acc = nullptr;

    uint32_t* counts_row(const Lane& L) const { return L.counts.as<uint32_t>() + L.depth * kCountsPerIter; }

    // Enqueue the lane's next step for its current path count: one wavefront
    // iteration (extend + shades + the survivor-count readback), or, below
    // the tail threshold, the tail kernel that finishes every remaining path.
    int step(Lane& L) {
        const uint32_t thr = tail_paths(tail, L.rp.B, plan.nchunks);
        if (L.n == 0) { L.state = Lane::DONE; return 0; }
        if (L.depth > kMaxDepth + 1) return fail("internal: path exceeded the depth cap");
        const StepArgs a{L.rp, *L.cur, *L.nxt, L.view, L.n, L.depth, lay, L.hit.p, counts_row(L),
                         L.seg_tail.as<unsigned long long>(), L.index, point_hits, L.stream};
        if (L.n <= thr) {
            std::pair<hipEvent_t, hipEvent_t>* fe = nullptr;
            if (s->profiling) {
                if (L.n_fin == L.ev_fin.size()) {
                    hipEvent_t e0 = nullptr, e1 = nullptr;
                    HIPCHK(hipEventCreate(&e0));
                    HIPCHK(hipEventCreate(&e1));
                    L.ev_fin.push_back({e0, e1});
                }
                fe = &L.ev_fin[L.n_fin++];
            }
            if (int rc = enqueue_tail(*s, a, fe)) return rc;
            s->stats.finish_paths += L.n;
            L.state = Lane::DONE;
            return 0;
        }
        const ExtendPath path = L.depth == 0 && L.fused_camera ? ExtendPath::CAMERA
                                : L.depth > 0 && s->ext_lds    ? ExtendPath::LDS
                                                               : ExtendPath::HBM;
        if (int rc = enqueue_iteration(*s, a, path, true, s->profiling ? L.ev : nullptr)) return rc;
        HIPCHK(hipMemcpyAsync(L.h_counts + L.depth * kCountsPerIter, a.counts, kCountsPerIter * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, L.stream));
        HIPCHK(hipEventRecord(L.ev_cnt, L.stream));
        L.state = Lane::RUNNING;
        L.seq = seq++;
        return 0;
    }
    // The iteration's counts have arrived: take its statistics, move on.
    int advance(Lane& L) {
        if (s->profiling) {
            float a = 0, b = 0;
            HIPCHK(hipEventElapsedTime(&a, L.ev[0], L.ev[1]));
            HIPCHK(hipEventElapsedTime(&b, L.ev[1], L.ev[2]));
            s->stats.ms_extend += a; s->stats.ms_shade += b;
            s->stats.extend_launches += 1;
        }
        s->stats.extend_rays += L.n;
        s->stats.segments += L.n;
        if ((uint32_t)L.depth > s->stats.max_depth_seen) s->stats.max_depth_seen = (uint32_t)L.depth;
        uint32_t* row = L.h_counts + L.depth * kCountsPerIter;
        uint32_t n = 0;
        for (int x = 0; x < kShards; ++x) {
            const uint32_t c_x = shard_count(survivor_counts(row), x);
            if (c_x > lay.shard_cap) return fail("internal: shard overflow");
            n += c_x;
        }
        uint64_t hits = 0;
        // a hit-queue counter can pass its shard's capacity (k_extend_curves' items then spill into the next
        // shard): what the queue holds is the clamped count
        for (int mt = 0; mt < 4; ++mt)
            for (int x = 0; x < kShards; ++x) hits += std::min<uint32_t>(shard_count(hit_counts(row, mt), x), (uint32_t)lay.shard_cap);
        (L.depth == 0 ? s->stats.shade_hits_d0 : s->stats.shade_hits) += hits;
        s->stats.shade_survivors += n;
        L.view = QView{survivor_counts(counts_row(L)), (uint32_t)lay.shard_cap};
        std::swap(L.cur, L.nxt);
#ifdef RT_STATS
        static const bool dbg_depth = std::getenv("RTAMD_DEBUG_DEPTH") != nullptr;   // stats builds: live paths per depth
        if (dbg_depth) std::fprintf(stderr, "depth-count lane %d chunk %d depth %d in %u out %u\n", L.index, L.chunk,
                                    L.depth, L.n, n);
#endif
        L.n = n;
        ++L.depth;
        return step(L);
    }
    int start(Lane& L, int ch) {
        const int done = ch * (int)plan.chunk;
        L.chunk = ch;
        L.S = (uint32_t)std::min<int>((int)plan.chunk, spp_count - done);
        RenderParams& rp = L.rp;
        rp = RenderParams{};
        rp.nx = (uint32_t)nx; rp.ny = (uint32_t)ny; rp.npix = px.n;
        rp.inx = 1.0 / (double)nx; rp.iny = 1.0 / (double)ny;
        rp.spp0 = (uint32_t)(spp_begin + done); rp.k0 = k0; rp.k1 = k1;
        rp.pixlist = px.pix;
        rp.sb = L.sb.as<double>();
        rp.B = px.n * L.S;
        rp.compact = px.compact ? 1u : 0u;
        rp.exact_libm = exact_libm ? 1u : 0u;
        HIPCHK(hipMemsetAsync(L.counts.p, 0, kIters * kCountsPerIter * sizeof(uint32_t), L.stream));
        const uint32_t thr = tail_paths(tail, rp.B, plan.nchunks);
        L.fused_camera = s->cam_lds != 0 && rp.B > thr;      // the tail kernel starts from raygen's state
        if (!L.fused_camera) HIPCHK(launch_raygen(s->dev, rp, L.A, L.stream));
        L.cur = &L.A;
        L.nxt = &L.B;
        L.view = QView{nullptr, (uint32_t)lay.scap};     // raygen output: contiguous
        L.n = rp.B;
        L.depth = 0;
        s->stats.paths += rp.B;
        return step(L);
    }
    // finished chunks into the accumulator, in chunk order
    int accumulate(bool& progressed) {
        for (int li = 0; li < plan.nlanes; ++li) {
            Lane& L = *c->lanes[li];
            if (L.state != Lane::DONE || L.chunk != next_acc) continue;
            if (last_acc && last_acc != &L) HIPCHK(hipStreamWaitEvent(L.stream, last_acc->ev_acc, 0));
            if (px.accum2 || px.count)
                HIPCHK(launch_accumulate_moments(L.rp, L.S, accum, px.accum2, px.count, L.stream));
            else
                HIPCHK(launch_accumulate(L.rp, L.S, accum, L.stream));
            HIPCHK(hipEventRecord(L.ev_acc, L.stream));
            last_acc = &L;
            ++next_acc;
            L.state = Lane::IDLE;
            progressed = true;
            li = -1;                                     // the next chunk may sit on an earlier lane
        }
        return 0;
    }
    int run() {
        while (next_acc < plan.nchunks) {
            bool progressed = false;
            if (int rc = accumulate(progressed)) return rc;
            for (int li = 0; li < plan.nlanes; ++li) {      // idle lanes take the next chunk
                Lane& L = *c->lanes[li];
                if (L.state != Lane::IDLE || next_chunk >= plan.nchunks) continue;
                if (int rc = start(L, next_chunk++)) return rc;
                progressed = true;
            }
            for (int li = 0; li < plan.nlanes; ++li) {      // lanes whose counts have arrived
                Lane& L = *c->lanes[li];
                if (L.state != Lane::RUNNING) continue;
                const hipError_t q = hipEventQuery(L.ev_cnt);
                if (q == hipErrorNotReady) continue;
                HIPCHK(q);
                if (int rc = advance(L)) return rc;
                progressed = true;
            }
            if (progressed) continue;
            Lane* oldest = nullptr;                          // nothing to do: wait for the oldest pending step
            for (int li = 0; li < plan.nlanes; ++li) {
                Lane& L = *c->lanes[li];
                if (L.state == Lane::RUNNING && (!oldest || L.seq < oldest->seq)) oldest = &L;
            }
            if (!oldest) return fail("internal: render lanes stalled");
            HIPCHK(hipEventSynchronize(oldest->ev_cnt));
        }
        for (int li = 0; li < plan.nlanes; ++li) HIPCHK(hipStreamSynchronize(c->lanes[li]->stream));
        return 0;
    }
};

// A finished render's fault word, curve counters, control words and profiling brackets into its statistics
int collect(Context* c, Scene* s, const int nlanes) {
    uint32_t f = 0;
    HIPCHK(take_fault(&f));
    if (f) return fail(fault_text(f));
    unsigned long long cs[2];
    HIPCHK(take_curve_stats(cs));
    s->stats.curve_pooled_batches = cs[0];
    s->stats.curve_flat_pooled = cs[1];
    for (int li = 0; li < nlanes; ++li) {
        Lane& L = *c->lanes[li];
        unsigned long long ctl[kCtlWords] = {0, 0, 0, 0};
        HIPCHK(hipMemcpy(ctl, L.seg_tail.p, sizeof ctl, hipMemcpyDeviceToHost));
        if (ctl[kCtlLdsErr]) return fail("internal: a persistent kernel's LDS allocation was too small (flags " +
                                         std::to_string(ctl[kCtlLdsErr]) + ")");
        s->stats.segments += ctl[kCtlSegments] + ctl[kCtlFuseSegs];
        s->stats.extend_rays += ctl[kCtlFuseSegs];     // the fused curve extend's segments past its launch's rays
        for (size_t k = 0; k < L.n_fin; ++k) {
            float a = 0;
            HIPCHK(hipEventElapsedTime(&a, L.ev_fin[k].first, L.ev_fin[k].second));
            s->stats.ms_finish += a;
        }
    }
    return 0;
}
}  // namespace

namespace rtamd {
// Render passes spp_begin .. spp_begin+spp_count-1 of the pixels of `px`
// into accum (indexed by image pixel j, or by the list's own pixel index
// q when px.compact).
int render_impl(Scene* s, int nx, int ny, const PixSet& px, int spp_begin, int spp_count, uint64_t seed,
                double* accum, hipStream_t stream) {
    if (int rc = check_render(s, nx, ny, spp_begin, spp_count)) return rc;
    if ((uint64_t)nx * (uint64_t)ny >= (1ull << 31)) return fail("image too large");
    CTX_OF(c, s);
    HIPCHK(hipSetDevice(c->device));
    if (!stream) stream = c->stream;
    auto t_start = std::chrono::steady_clock::now();
    std::memset(&s->stats, 0, sizeof s->stats);
    {
        uint32_t stale = 0;
        HIPCHK(take_fault(&stale));                  // a fault word left by another context's failed launch
        unsigned long long cs[2];
        HIPCHK(take_curve_stats(cs));                // counters start at zero for this render
        // tests: drive a sampler / the curve kernel's per-ray loop into its cap
        const char* e = std::getenv("RTAMD_REJECT_CAP");
        const char* rc = std::getenv("RTAMD_CURVE_RAY_CAP");
        HIPCHK(set_test_caps(e ? std::max(0, std::atoi(e)) : 4096, rc ? (uint32_t)std::strtoul(rc, nullptr, 10) : 0u));
    }
    if (spp_count == 0 || px.n == 0) return 0;
    // the cap is sized on the context's first render (before its pools exist), then kept; an option change
    // that resets it (RT_OPT_LANES, RT_OPT_MAX_PATHS) frees the old pools first, so the sizing sees the
    // memory they held and the lanes together stay within it
    if (!c->pool_cap) {
        for (auto& L : c->lanes)
            if (L && L->stream) HIPCHK(hipStreamSynchronize(L->stream));
        for (auto& L : c->lanes) L.reset();
        c->pool_lanes = std::min(kLanes, lanes_wanted(*c));
        c->pool_cap = max_paths(*c, c->pool_lanes);
    }
    const RenderPlan plan = plan_render(px.n, spp_count, c->pool_cap, lanes_for(*c, s->dev));
    s->stats.chunks = (uint32_t)plan.nchunks;
    s->stats.lanes = (uint32_t)plan.nlanes;
    const char* slack = std::getenv("RTAMD_SHARD_SLACK");    // test switch (rt_plan.h pool_layout; any value sets it)
    const PoolLayout lay = pool_layout((size_t)px.n * plan.chunk,
                                       slack ? std::max<size_t>(256, std::strtoull(slack, nullptr, 10)) : 0);
    if (lay.scap >= (1ull << 32)) return fail("path pool too large");
    // callers' prior work on `stream` (e.g. zeroing accum) comes first
    hipEvent_t ev_in = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
    std::unique_ptr<void, void (*)(void*)> ev_in_guard(ev_in, [](void* e) { (void)hipEventDestroy((hipEvent_t)e); });
    HIPCHK(hipEventRecord(ev_in, stream));
    if (int rc = prepare_lanes(c, s, plan.nlanes, lay, ev_in)) return rc;
    // An error return below leaves kernels queued on the lanes that may still
    // write the caller's accumulator: drain every lane before returning.
    struct Drain {
        Context* c; int n; bool armed = true;
        ~Drain() {
            if (!armed) return;
            for (int i = 0; i < n; ++i)
                if (c->lanes[i] && c->lanes[i]->stream) (void)hipStreamSynchronize(c->lanes[i]->stream);
            uint32_t f = 0;
            (void)take_fault(&f);                  // do not leak this render's fault bits into the next
        }
    } drain{c, plan.nlanes};
    const TailOpts tail{c->wavefront_only, c->opt_tail_paths, c->opt_tail_div, curve_kernel_scene(s->dev)};
    RenderRun run{c, s, nx, ny, px, spp_begin, spp_count, accum, plan, lay, tail, (uint32_t)seed, (uint32_t)(seed >> 32),
                  scene_exact_libm(*c, *s), s->point_hits && !point_hits_off()};
    if (int rc = run.run()) return rc;
    drain.armed = false;
    if (int rc = collect(c, s, plan.nlanes)) return rc;
    // later work on the caller's stream sees the finished accumulator
    HIPCHK(hipStreamSynchronize(stream));
    s->stats.ms_total =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return 0;
}
}  // namespace rtamd

namespace rtamd {
// The pixels `ps` selects as a PixSet: the scene's cached device list, made and uploaded again when the
// selection differs from the cached one.  (nx, ny and ps are valid: render_sel)
int pixset_of(Scene* s, int nx, int ny, const PixSel& ps, bool compact, PixSet* out) {
    CTX_OF(c, s);
    HIPCHK(hipSetDevice(c->device));
    if (s->pix_nx != nx || s->pix_ny != ny || s->pix_y0 != ps.y0 || s->pix_y1 != ps.y1 || s->pix_shard != ps.shard ||
        s->pix_nshard != ps.nshard) {
        std::vector<uint32_t> pl = make_pixlist(nx, ny, ps);
        s->pix_nx = -1;                              // stale until the upload below succeeds
        HIPCHK(s->pixlist.ensure(std::max<size_t>(1, pl.size()) * sizeof(uint32_t)));
        if (!pl.empty()) HIPCHK(hipMemcpy(s->pixlist.p, pl.data(), pl.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        s->pix_nx = nx; s->pix_ny = ny; s->pix_y0 = ps.y0; s->pix_y1 = ps.y1;
        s->pix_shard = ps.shard; s->pix_nshard = ps.nshard;
        s->pix_n = (uint32_t)pl.size();
    }
    *out = PixSet{s->pixlist.as<const uint32_t>(), s->pix_n, compact, nullptr, nullptr};
    return 0;
}
}  // namespace rtamd

namespace {
// render_impl over the pixels `ps` selects.  The checks stand in the order their errors have always won:
// render_impl's first four, the selection's, the frame size.  A render of no passes does no list work
// and leaves the cached list as it is (render_impl returns after its clears).
int render_sel(Scene* s, int nx, int ny, const PixSel& ps, int spp_begin, int spp_count, uint64_t seed,
               double* accum, bool compact, hipStream_t stream) {
    if (int rc = check_render(s, nx, ny, spp_begin, spp_count)) return rc;
    if (ps.nshard <= 0 || ps.shard < 0 || ps.shard >= ps.nshard) return fail("invalid shard index/count");
    if (ps.y0 < 0 || ps.y1 < ps.y0 || ps.y1 > ny) return fail("row range outside the image");
    if ((uint64_t)nx * (uint64_t)ny >= (1ull << 31)) return fail("image too large");
    PixSet px{nullptr, 0, compact, nullptr, nullptr};
    if (spp_count > 0)
        if (int rc = pixset_of(s, nx, ny, ps, compact, &px)) return rc;
    return render_impl(s, nx, ny, px, spp_begin, spp_count, seed, accum, stream);
}
}  // namespace

extern "C" {

int rt_render_device(int scene, int nx, int ny, int spp_begin, int spp_count, uint64_t seed, int shard,
                     int nshard, double* accum, void* stream) {
    LOCK_SCENE(s, scene);
    if (!accum) return fail("null accum");
    if (ny <= 0) return fail("image size must be positive");
    return render_sel(s, nx, ny, PixSel{0, ny, shard, nshard}, spp_begin, spp_count, seed, accum, false,
                      (hipStream_t)stream);
}

int rt_render_shard_device(int scene, int nx, int ny, int spp_begin, int spp_count, uint64_t seed, int shard,
                           int nshard, double* accum_compact, void* stream) {
    LOCK_SCENE(s, scene);
    if (!accum_compact) return fail("null accum");
    if (ny <= 0) return fail("image size must be positive");
    return render_sel(s, nx, ny, PixSel{0, ny, shard, nshard}, spp_begin, spp_count, seed, accum_compact, true,
                      (hipStream_t)stream);
}

int rt_render_rows_device(int scene, int nx, int ny, int y_begin, int y_count, int spp_begin, int spp_count,
                          uint64_t seed, double* accum, void* stream) {
    LOCK_SCENE(s, scene);
    if (!accum) return fail("null accum");
    if (y_begin < 0 || y_count < 0 || (int64_t)y_begin + y_count > ny) return fail("row range outside the image");
    return render_sel(s, nx, ny, PixSel{y_begin, y_begin + y_count, 0, 1}, spp_begin, spp_count, seed, accum, false,
                      (hipStream_t)stream);
}

namespace {
// rows [y0, y0+yn) of a host accumulator through the context's device copy
int render_rows_host(Scene* s, int nx, int ny, int y0, int yn, int spp_begin, int spp_count, uint64_t seed,
                     double* accum_host) {
    if (nx <= 0 || ny <= 0) return fail("image size must be positive");
    if (y0 < 0 || yn < 0 || (int64_t)y0 + yn > ny) return fail("row range outside the image");
    CTX_OF(c, s);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->accum_tmp.ensure((size_t)nx * ny * 3 * sizeof(double)));
    const size_t off = (size_t)y0 * nx * 3, cnt = (size_t)yn * nx * 3;
    double* dev = c->accum_tmp.as<double>();
    HIPCHK(hipMemcpyAsync(dev + off, accum_host + off, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (int rc = render_sel(s, nx, ny, PixSel{y0, y0 + yn, 0, 1}, spp_begin, spp_count, seed, dev, false, c->stream))
        return rc;
    HIPCHK(hipMemcpyAsync(accum_host + off, dev + off, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
}  // namespace

int rt_render_rows(int scene, int nx, int ny, int y_begin, int y_count, int spp_begin, int spp_count, uint64_t seed,
                   double* accum_host) {
    LOCK_SCENE(s, scene);
    if (!accum_host) return fail("null accum");
    return render_rows_host(s, nx, ny, y_begin, y_count, spp_begin, spp_count, seed, accum_host);
}

int rt_trace_line(int scene, int nx, int ny, int y, int sample_count, uint64_t seed, double* raw_data,
                  uint8_t* image) {
    LOCK_SCENE(s, scene);
    if (!raw_data || !image) return fail("null buffer");
    if (sample_count < 1) return fail("sample_count is 1-based (main.scm:452)");
    if (int rc = render_rows_host(s, nx, ny, y, 1, sample_count - 1, 1, seed, raw_data)) return rc;
    // main.scm:462-469: correct-gamma of sum/sample-count, floor(255.99*min(1,c)), for row y only
    const size_t b = (size_t)y * nx * 3, e = b + (size_t)nx * 3;
    for (size_t i = b; i < e; ++i) {
        const double c = std::sqrt(raw_data[i] / sample_count);
        const double m = (1.0 < c) ? 1.0 : c;
        image[i] = (uint8_t)std::floor(255.99 * m);
    }
    return 0;
}

int rt_render(int scene, int nx, int ny, int spp_begin, int spp_count, uint64_t seed, double* accum_host) {
    LOCK_SCENE(s, scene);
    if (!accum_host) return fail("null accum");
    if (nx <= 0 || ny <= 0) return fail("image size must be positive");
    CTX_OF(c, s);
    HIPCHK(hipSetDevice(c->device));
    const size_t bytes = (size_t)nx * ny * 3 * sizeof(double);
    HIPCHK(c->accum_tmp.ensure(bytes));
    HIPCHK(hipMemcpyAsync(c->accum_tmp.p, accum_host, bytes, hipMemcpyHostToDevice, c->stream));
    if (int rc = render_sel(s, nx, ny, full_frame(ny), spp_begin, spp_count, seed, c->accum_tmp.as<double>(), false,
                            c->stream))
        return rc;
    HIPCHK(hipMemcpyAsync(accum_host, c->accum_tmp.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int rt_shard_pixels(int nx, int ny, int shard, int nshard, uint32_t* out_pix, int64_t* out_count) {
    if (nx <= 0 || ny <= 0) return fail("image size must be positive");
    if (nshard <= 0 || shard < 0 || shard >= nshard) return fail("invalid shard index/count");
    if (!out_count) return fail("null out pointer");
    const std::vector<uint32_t> pl = make_pixlist(nx, ny, PixSel{0, ny, shard, nshard});
    *out_count = (int64_t)pl.size();
    if (out_pix && !pl.empty()) std::memcpy(out_pix, pl.data(), pl.size() * sizeof(uint32_t));
    return 0;
}

int rt_resolve_u8(const double* accum, int nx, int ny, int count, uint8_t* out) {
    if (!accum || !out) return fail("null buffer");
    if (count <= 0) return fail("sample_count must be positive");
    const size_t n = (size_t)nx * ny * 3;
    for (size_t i = 0; i < n; ++i) {
        const double c = std::sqrt(accum[i] / count);
        const double m = (1.0 < c) ? 1.0 : c;
        out[i] = (uint8_t)std::floor(255.99 * m);
    }
    return 0;
}

int rt_resolve_u8_device(int ctx, const double* accum, int nx, int ny, int count, uint8_t* out, void* stream) {
    LOCK_CTX(c, ctx);
    if (!accum || !out) return fail("null buffer");
    if (count <= 0) return fail("sample_count must be positive");
    CTX_STREAM(c, st, stream);
    HIPCHK(launch_resolve_u8(accum, (uint32_t)((size_t)nx * ny * 3), count, out, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

/* RT_HAS_POINT_HITS */
int rt_scene_point_hits(int scene, int* out) {
    LOCK_SCENE(s, scene);
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    if (!out) return fail("null out pointer");
    *out = (s->point_hits && !point_hits_off()) ? 1 : 0;
    return 0;
}

}  // extern "C"
