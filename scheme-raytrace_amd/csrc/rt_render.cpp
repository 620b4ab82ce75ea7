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

namespace {
// Path-pool cap (paths per chunk).  Bigger pools mean fewer chunks, each
// with its own narrow tail: C2 (1920x1080x1024 spp) 13 383 Mrays/s with 96M
// paths (22 chunks), 13 675 with 200M (12), 13 742 with 330M (8 chunks;
// profiles/r02/pool/); round 5, with the first frame on new pools excluded (a re-allocated pool's first frame
// waits for the driver to clear the memory it reuses, tools/realloc_probe.py): 8 chunks (288Mi- or 320Mi-path
// cap) 13 804–13 888, 10 / 12 chunks 13 657–13 711, 6 chunks (354Mi) 13 927 / 13 957 (profiles/r05/ab/pool/).
// Default 384Mi paths, but at most what lets the render lanes' pools (kPoolBytesPerPath) take 65 % of the
// device's free memory — on a 288-GB MI355X C2's frame then cuts into 6 chunks (196 GB of pools; at 288 B
// per path it would tip into 8).  RT_OPT_MAX_PATHS overrides.
// A lane's pools per path: state pool A (ray, path record, and the depth-0 time and draw counter: a chunk
// starts in A, so pool B never holds depth-0 state), state pool B, the hit queues (5 x 16 B: three HitRec
// queues and the lambertian one as HitRec or HitPt, rt_device.h HitBuf) and the sample colours — 276 B
constexpr size_t kStateBytesB = sizeof(RayRec) + sizeof(PathRec);
constexpr size_t kStateBytesA = kStateBytesB + sizeof(double) + sizeof(uint32_t);
constexpr size_t kHitBytesPerPath = 3 * sizeof(HitRec) + sizeof(HitPt);
constexpr size_t kPoolBytesPerPath = kStateBytesA + kStateBytesB + kHitBytesPerPath + 3 * sizeof(double);
static_assert(kHitBytesPerPath == 5 * sizeof(HitRec), "HitBuf's layout: five 16-B strides");
size_t max_paths(const Context& c, const int lanes) {
    if (c.opt_max_paths > 0) return c.opt_max_paths < 1024 ? 1024 : (size_t)c.opt_max_paths;
    size_t v = (size_t)384 << 20;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
        const size_t fit = free_b / 100 * 65 / ((size_t)std::max(1, lanes) * kPoolBytesPerPath);
        if (fit < v) v = fit;
    } else {
        (void)hipGetLastError();
    }
    return v < ((size_t)1 << 20) ? ((size_t)1 << 20) : v;
}

// the libm mode a scene's renders (and rt_light_probe) take under the context's RT_OPT_EXACT_LIBM
bool scene_exact_libm(const Context& c, const Scene& s) {
    return c.opt_exact_libm == RT_LIBM_EXACT ||
           (c.opt_exact_libm == RT_LIBM_AUTO && (s.dev.n_bez > 0 || s.dev.has_noise_tex));
}
int lanes_wanted(const Context& c) {   // RT_OPT_LANES: path pools kept in flight (1 = no overlap)
    return c.opt_lanes > 0 ? (int)std::min<int64_t>(c.opt_lanes, kLanes) : 2;
}
// The persistent curve kernels serve scenes whose world BVH holds every curve (launch_extend)
bool curve_kernel_scene(const DevScene& d) {
    return d.n_bez > 0 && d.bvh_has_bez && d.bez_groups == 0 && d.n_med == 0 && d.n_klein == 0;
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
bool curve_fuse(const DevScene& d, const uint32_t n) {
    if (!(curve_kernel_scene(d) && curve_persistent() && !d.has_perlin && !d.has_image_tex && d.light.type == LIGHT_OFF)) return false;
    if (!d.fuse_ring || d.n_leaves >= (1 << kFuseLeafBits) - 1) return false;    // FuseHit packs leaf + 1 in 25 bits
    const char* e = std::getenv("RTAMD_CURVE_FUSE");   // read per render: tests switch it inside one process
    if (e && e[0] == '0') return false;
    if (e && e[0] == '1') return true;
    return n <= kFuseMaxRays;
}

// A chunk's live paths at or below max(tail_threshold, B / tail_divisor) go to
// the tail kernel; RT_OPT_TAIL_OFF keeps every depth in the wavefront.
// Without those options the threshold also follows the render's shape (round 5, C2's scene, same images;
// profiles/r05/ab/tail/): a render of one chunk has no second lane to fill its narrow depths, so the tail
// kernel takes over at B/4, at most 524 288 paths (1 spp per frame, the progressive loop: 2.60 → 2.13 ms); renders of a few
// small chunks take it at up to B/64, at most 262 144 paths (4 spp: 4.85 → 4.17 ms; 16 spp: 12.7 → 11.3 ms);
// large chunks keep B/256 (the 8-GPU per-rank share, 680×381×1024 spp: 73.6 ms at B/256, 75.1 at B/64; C2:
// B/256 over B/128, rounds 2–3).  Curve-kernel scenes keep the fixed rule (their tail kernel walks curves
// per ray; the fused curve extend serves their small launches).
uint32_t tail_paths(const Context& c, const uint32_t B, const int nchunks, const bool curves) {
    if (c.wavefront_only) return 0u;
    if (c.opt_tail_paths <= 0 && c.opt_tail_div <= 0 && !curves) {
        // (bounded: a large single chunk — one render lane, e.g. Cornell at 256 spp, 268M paths — keeps B/256;
        // B/4 there handed a quarter of the paths to the tail kernel: 100.6 of 213 ms)
        if (nchunks == 1) return std::max<uint32_t>(std::max<uint32_t>(32768u, std::min<uint32_t>(B / 4u, 524288u)), B / 256u);
        return std::max<uint32_t>(std::max<uint32_t>(32768u, std::min<uint32_t>(B / 64u, 262144u)), B / 256u);
    }
    const uint32_t thr = c.opt_tail_paths > 0 ? (uint32_t)std::min<int64_t>(c.opt_tail_paths, 0xFFFFFFFFll) : 32768u;
    // B/256 with 288M-path pools (+0.9 % over B/128, profiles/r02/tail*/; B/128 was best with 96M pools)
    const uint32_t div = c.opt_tail_div > 0 ? (uint32_t)std::min<int64_t>(c.opt_tail_div, 0xFFFFFFFFll) : 256u;
    return std::max<uint32_t>(thr, B / div);
}

// depth0: pool A, which also holds raygen's time and draw counter (pool B: null, never read)
PathState carve_state(void* base, size_t cap, const bool depth0) {
    PathState st{};
    char* p = static_cast<char*>(base);
    st.ray = reinterpret_cast<RayRec*>(p);
    p += cap * sizeof(RayRec);
    st.path = reinterpret_cast<PathRec*>(p);
    p += cap * sizeof(PathRec);
    if (!depth0) return st;
    st.tm = reinterpret_cast<double*>(p);
    p += cap * sizeof(double);
    st.rng0 = reinterpret_cast<uint32_t*>(p);
    return st;
}
// RTAMD_NO_POINT_HITS (A/B, tests; read per render): every hit queue keeps HitRec
bool point_hits_off() { return std::getenv("RTAMD_NO_POINT_HITS") != nullptr; }
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
    if (spp_count == 0) return 0;

    const uint32_t npix = px.n;
    if (npix == 0) return 0;
    // Chunks of samples: as few as the pool cap allows, but at least two (one
    // per render lane) and an even count when the samples allow, so the two
    // lanes end together (a frame of three chunks would leave one lane alone
    // for a third of it).  A floor of four cost 6.5 % on a 1/8-frame shard
    // (680x381x1024 spp, the per-rank work at 8 GPUs) and 2.4 % at 1/4
    // (profiles/r02/mc/).
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
    const size_t cap_paths = c->pool_cap;
    uint32_t chunk = (uint32_t)std::max<size_t>(1, cap_paths / npix);
    if (chunk > (uint32_t)spp_count) chunk = (uint32_t)spp_count;
    {
        const int min_chunks = lanes_for(*c, s->dev);   // one chunk per lane at least
        int n = (int)((spp_count + chunk - 1) / chunk);
        if (n < min_chunks) n = std::min(min_chunks, spp_count);
        if (n > 1 && (n & 1) && n < spp_count) ++n;
        chunk = (uint32_t)((spp_count + n - 1) / n);
    }
    const int nchunks = (int)((spp_count + chunk - 1) / chunk);
    const int nlanes = std::max(1, std::min(std::min(kLanes, lanes_for(*c, s->dev)), nchunks));
    const size_t cap = (size_t)npix * chunk;
    s->stats.chunks = (uint32_t)nchunks;
    s->stats.lanes = (uint32_t)nlanes;
    // sharded compaction (rt_device.h kShards): shard capacity bounds what the
    // blocks of one shard can append in one wavefront step (extend: one item
    // per thread; the four shade kernels: grid-stride over at most 4096 blocks)
    const size_t gmax = std::min<size_t>(4096, (cap + 255) / 256 + kShards);
    size_t slack = 4 * 32 * gmax + 256;
    // test switch (RTAMD_SHARD_SLACK): a smaller slack drives k_extend_curves' hit appends past their wave's
    // shard (wave_append<true> spills into the next one); 256 still bounds the shade kernels' survivors
    if (const char* e = std::getenv("RTAMD_SHARD_SLACK")) slack = std::max<size_t>(256, std::strtoull(e, nullptr, 10));
    const size_t shard_cap = (cap + kShards - 1) / kShards + slack;
    const size_t scap = shard_cap * kShards;
    if (scap >= (1ull << 32)) return fail("path pool too large");
    constexpr int kCountsPerIter = 5 * kShards * kCntStride;   // 4 material hit queues + survivors, 8 shards each
    constexpr int kIters = kMaxDepth + 4;
    // callers' prior work on `stream` (e.g. zeroing accum) comes first
    hipEvent_t ev_in = nullptr;
    HIPCHK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
    std::unique_ptr<void, void (*)(void*)> ev_in_guard(ev_in, [](void* e) { (void)hipEventDestroy((hipEvent_t)e); });
    HIPCHK(hipEventRecord(ev_in, stream));
    for (int li = 0; li < nlanes; ++li) {
        if (!c->lanes[li]) c->lanes[li].reset(new Lane());
        c->lanes[li]->index = li;
        Lane& L = *c->lanes[li];
        if (!L.stream) HIPCHK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        if (!L.ev_cnt) HIPCHK(hipEventCreateWithFlags(&L.ev_cnt, hipEventDisableTiming));
        if (!L.ev_acc) HIPCHK(hipEventCreateWithFlags(&L.ev_acc, hipEventDisableTiming));
        if (s->profiling && !L.ev[0]) for (auto& e : L.ev) HIPCHK(hipEventCreate(&e));
        HIPCHK(L.st_a.ensure(scap * kStateBytesA));
        HIPCHK(L.st_b.ensure(scap * kStateBytesB));
        HIPCHK(L.hit.ensure(scap * kHitBytesPerPath));     // the 4 material hit queues (sharded like the survivors)
        HIPCHK(L.sb.ensure(cap * 3 * sizeof(double)));
        HIPCHK(L.counts.ensure(kIters * kCountsPerIter * sizeof(uint32_t)));
        // tail segments, next tail path / curve claim, LDS errors, the fused curve extend's continuation segments
        HIPCHK(L.seg_tail.ensure(4 * sizeof(unsigned long long)));
        if (!L.h_counts) HIPCHK(hipHostMalloc((void**)&L.h_counts, kIters * kCountsPerIter * sizeof(uint32_t)));
        HIPCHK(hipStreamWaitEvent(L.stream, ev_in, 0));
        HIPCHK(hipMemsetAsync(L.seg_tail.p, 0, 4 * sizeof(unsigned long long), L.stream));
        L.A = carve_state(L.st_a.p, scap, true);
        L.B = carve_state(L.st_b.p, scap, false);
        L.state = Lane::IDLE;
        L.n_fin = 0;
    }
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
    } drain{c, nlanes};
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    // RT_OPT_EXACT_LIBM: auto = exact in scenes with curves or noise / marble textures ("libm"):
    // C3 (marble) frame rows with the device library's sin / cos were 0.79 % of pixels off by more than 1e-9;
    // exact there costs 1.7 % (profiles/r06/c3_libm/).  The cover scene keeps the device's: exact would cost it
    // 1.4 % (profiles/r06/c2_libm/) for 26 of 15 360 horizon pixels at 256 passes, all within 1e-7
    const bool exact_libm = scene_exact_libm(*c, *s);
    // point records for the lambertian queue of the launches the SOLO LDS kernels make (rt_device.h HitPt)
    const bool point_hits = s->point_hits && !point_hits_off();
    uint64_t seq = 0;

    // Enqueue the lane's next step for its current path count: one wavefront
    // iteration (extend + shades + the survivor-count readback), or, below
    // the tail threshold, the tail kernel that finishes every remaining path.
    auto step = [&](Lane& L) -> int {
        const uint32_t tail = tail_paths(*c, L.rp.B, nchunks, curve_kernel_scene(s->dev));
        if (L.n == 0) { L.state = Lane::DONE; return 0; }
        if (L.depth > kMaxDepth + 1) return fail("internal: path exceeded the depth cap");
        if (L.n <= tail) {
            std::pair<hipEvent_t, hipEvent_t>* fe = nullptr;
            if (s->profiling) {
                if (L.n_fin == L.ev_fin.size()) {
                    hipEvent_t e0 = nullptr, e1 = nullptr;
                    HIPCHK(hipEventCreate(&e0));
                    HIPCHK(hipEventCreate(&e1));
                    L.ev_fin.push_back({e0, e1});
                }
                fe = &L.ev_fin[L.n_fin++];
                HIPCHK(hipEventRecord(fe->first, L.stream));
            }
            HIPCHK(hipMemsetAsync(L.seg_tail.as<unsigned long long>() + 1, 0, sizeof(unsigned long long), L.stream));
            HIPCHK(launch_finish(s->dev, s->d_dev.as<const DevScene>(), L.rp, *L.cur, L.view, L.n, L.seg_tail.as<unsigned long long>(),
                                 s->ext_lds ? (size_t)32 << 10 : 0, (uint32_t)L.depth, L.stream));
            if (fe) HIPCHK(hipEventRecord(fe->second, L.stream));
            s->stats.finish_paths += L.n;
            L.state = Lane::DONE;
            return 0;
        }
        uint32_t* cnt = L.counts.as<uint32_t>() + L.depth * kCountsPerIter;   // [material][shard], survivors at 4
        bool fused = false;
        HitBuf hit{L.hit.as<HitRec>() + scap, (uint32_t)scap, L.hit.as<HitPt>()};
        const bool camera = L.depth == 0 && L.fused_camera, ext_lds = L.depth > 0 && s->ext_lds;
        // point records are what the SOLO LDS kernels write, so a render can mix the two formats across depths:
        // one of those kernels switched off, or a chunk whose depth 0 is k_raygen + k_extend
        const bool pt = point_hits && (camera || ext_lds);
        if (s->profiling) HIPCHK(hipEventRecord(L.ev[0], L.stream));
        if (camera)                             // raygen + first closest hit in one kernel
            HIPCHK(launch_camera(s->dev, L.rp, *L.cur, L.n, hit, pt, (uint32_t)shard_cap, cnt,
                                 s->cam_lds, s->cam_blocks, L.seg_tail.as<unsigned long long>() + 2, L.stream));
        else if (ext_lds)                       // every ray of a depth >= 1 launch has time +0.0
            HIPCHK(launch_extend_lds(s->dev, L.rp, *L.cur, L.view, L.n, hit, pt, (uint32_t)shard_cap,
                                     cnt, s->ext_lds_blocks, L.seg_tail.as<unsigned long long>() + 2, L.stream));
        else {
            // the curve walk's stack overflow area: one region per render lane (lanes run concurrently)
            DevScene dl = s->dev;
            if (dl.stk_ovf) dl.stk_ovf += (size_t)L.index * dl.ovf_lanes * (size_t)(dl.stack4 - dl.lds4);
            if (dl.bez_ring) dl.bez_ring += (size_t)L.index * dl.ring_waves * kBezRing * 16u;
            if (dl.fuse_ring) dl.fuse_ring += (size_t)L.index * dl.ring_waves * kFuseWaveBytes;
            // the fused curve extend (k_extend_curves<FUSE>): every depth from 1 on in this one launch
            CurveFuse fz{L.seg_tail.as<unsigned long long>() + 3, (uint32_t)L.depth};
            fused = L.depth > 0 && curve_fuse(s->dev, L.n);
            HIPCHK(launch_extend(dl, s->d_dev.as<const DevScene>(), L.rp, *L.cur, L.view, L.n, hit,
                                 (uint32_t)shard_cap, cnt, L.depth == 0,
                                 reinterpret_cast<unsigned int*>(L.seg_tail.as<unsigned long long>() + 1),
                                 fused ? &fz : nullptr, L.stream));
        }
        if (s->profiling) HIPCHK(hipEventRecord(L.ev[1], L.stream));
        uint32_t* surv = cnt + 4 * kShards * kCntStride;
        for (int mt = 0; mt < 4 && !fused; ++mt) {         // (a fused launch shades its hits itself: no queues)
            if (!(s->dev.mat_mask & (1 << mt))) continue;
            const QView qv{cnt + mt * kShards * kCntStride, (uint32_t)shard_cap};
            HIPCHK(launch_shade(mt, s->dev, s->d_dev.as<const DevScene>(), L.rp, *L.cur, hit, pt, qv, L.n, *L.nxt, surv,
                                (uint32_t)shard_cap, (uint32_t)L.depth, L.stream));
        }
        if (s->profiling) HIPCHK(hipEventRecord(L.ev[2], L.stream));
        HIPCHK(hipMemcpyAsync(L.h_counts + L.depth * kCountsPerIter, cnt, kCountsPerIter * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, L.stream));
        HIPCHK(hipEventRecord(L.ev_cnt, L.stream));
        L.state = Lane::RUNNING;
        L.seq = seq++;
        return 0;
    };
    // The iteration's counts have arrived: take its statistics, move on.
    auto advance = [&](Lane& L) -> int {
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
        const uint32_t* row = L.h_counts + L.depth * kCountsPerIter;
        uint32_t n = 0;
        for (int x = 0; x < kShards; ++x) {
            const uint32_t c_x = row[4 * kShards * kCntStride + x * kCntStride];
            if (c_x > shard_cap) return fail("internal: shard overflow");
            n += c_x;
        }
        uint64_t hits = 0;
        // a hit-queue counter can pass its shard's capacity (k_extend_curves' items then spill into the next
        // shard): what the queue holds is the clamped count
        for (int k = 0; k < 4 * kShards; ++k) hits += std::min<uint32_t>(row[k * kCntStride], (uint32_t)shard_cap);
        (L.depth == 0 ? s->stats.shade_hits_d0 : s->stats.shade_hits) += hits;
        s->stats.shade_survivors += n;
        L.view = QView{L.counts.as<uint32_t>() + L.depth * kCountsPerIter + 4 * kShards * kCntStride,
                       (uint32_t)shard_cap};
        std::swap(L.cur, L.nxt);
#ifdef RT_STATS
        static const bool dbg_depth = std::getenv("RTAMD_DEBUG_DEPTH") != nullptr;   // stats builds: live paths per depth
        if (dbg_depth) std::fprintf(stderr, "depth-count lane %d chunk %d depth %d in %u out %u\n", L.index, L.chunk,
                                    L.depth, L.n, n);
#endif
        L.n = n;
        ++L.depth;
        return step(L);
    };
    auto start = [&](Lane& L, int ch) -> int {
        const int done = ch * (int)chunk;
        L.chunk = ch;
        L.S = (uint32_t)std::min<int>((int)chunk, spp_count - done);
        RenderParams& rp = L.rp;
        rp = RenderParams{};
        rp.nx = (uint32_t)nx; rp.ny = (uint32_t)ny; rp.npix = npix;
        rp.inx = 1.0 / (double)nx; rp.iny = 1.0 / (double)ny;
        rp.spp0 = (uint32_t)(spp_begin + done); rp.k0 = k0; rp.k1 = k1;
        rp.pixlist = px.pix;
        rp.sb = L.sb.as<double>();
        rp.B = npix * L.S;
        rp.compact = px.compact ? 1u : 0u;
        rp.exact_libm = exact_libm ? 1u : 0u;
        HIPCHK(hipMemsetAsync(L.counts.p, 0, kIters * kCountsPerIter * sizeof(uint32_t), L.stream));
        const uint32_t tail = tail_paths(*c, rp.B, nchunks, curve_kernel_scene(s->dev));
        L.fused_camera = s->cam_lds != 0 && rp.B > tail;     // the tail kernel starts from raygen's state
        if (!L.fused_camera) HIPCHK(launch_raygen(s->dev, rp, L.A, L.stream));
        L.cur = &L.A;
        L.nxt = &L.B;
        L.view = QView{nullptr, (uint32_t)scap};         // raygen output: contiguous
        L.n = rp.B;
        L.depth = 0;
        s->stats.paths += rp.B;
        return step(L);
    };

    int next_chunk = 0, next_acc = 0;
    Lane* last_acc = nullptr;
    while (next_acc < nchunks) {
        bool progressed = false;
        for (int li = 0; li < nlanes; ++li) {           // accumulate in chunk order
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
        for (int li = 0; li < nlanes; ++li) {           // idle lanes take the next chunk
            Lane& L = *c->lanes[li];
            if (L.state != Lane::IDLE || next_chunk >= nchunks) continue;
            if (int rc = start(L, next_chunk++)) return rc;
            progressed = true;
        }
        for (int li = 0; li < nlanes; ++li) {           // lanes whose counts have arrived
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
        for (int li = 0; li < nlanes; ++li) {
            Lane& L = *c->lanes[li];
            if (L.state == Lane::RUNNING && (!oldest || L.seq < oldest->seq)) oldest = &L;
        }
        if (!oldest) return fail("internal: render lanes stalled");
        HIPCHK(hipEventSynchronize(oldest->ev_cnt));
    }
    for (int li = 0; li < nlanes; ++li) HIPCHK(hipStreamSynchronize(c->lanes[li]->stream));
    drain.armed = false;
    {
        uint32_t f = 0;
        HIPCHK(take_fault(&f));
        if (f) return fail(fault_text(f));
        unsigned long long cs[2];
        HIPCHK(take_curve_stats(cs));
        s->stats.curve_pooled_batches = cs[0];
        s->stats.curve_flat_pooled = cs[1];
    }
    for (int li = 0; li < nlanes; ++li) {
        Lane& L = *c->lanes[li];
        unsigned long long ctl[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpy(ctl, L.seg_tail.p, sizeof ctl, hipMemcpyDeviceToHost));
        if (ctl[2]) return fail("internal: a persistent kernel's LDS allocation was too small (flags " +
                                std::to_string(ctl[2]) + ")");
        s->stats.segments += ctl[0] + ctl[3];
        s->stats.extend_rays += ctl[3];                // the fused curve extend's segments past its launch's rays
        for (size_t k = 0; k < L.n_fin; ++k) {
            float a = 0;
            HIPCHK(hipEventElapsedTime(&a, L.ev_fin[k].first, L.ev_fin[k].second));
            s->stats.ms_finish += a;
        }
    }
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
    HIPCHK(hipSetDevice(c->device));
    uint32_t stale = 0;
    HIPCHK(take_fault(&stale));
    DevBuf d_rays, d_t, d_mat;
    HIPCHK(d_rays.ensure((size_t)n * 7 * sizeof(double)));
    HIPCHK(d_t.ensure((size_t)n * sizeof(double)));
    HIPCHK(d_mat.ensure((size_t)n * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(d_rays.p, rays, (size_t)n * 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (walk == RT_WALK_HBM)
        HIPCHK(launch_hit_rays(s->dev, d_rays.as<const double>(), (uint32_t)n, d_t.as<double>(), d_mat.as<int32_t>(),
                               c->stream));
    else
        HIPCHK(launch_hit_rays_lds(s->dev, walk == RT_WALK_LDS_TIME0, walk == RT_WALK_LDS_TIME0 ? s->ext_lds : s->cam_lds,
                                   d_rays.as<const double>(), (uint32_t)n, d_t.as<double>(), d_mat.as<int32_t>(),
                                   c->stream));
    HIPCHK(hipMemcpyAsync(out_t, d_t.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_mat, d_mat.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    uint32_t f = 0;
    HIPCHK(take_fault(&f));
    if (f) return fail(fault_text(f));
    return 0;
}

int rt_hit_rays_stream(int scene, const double* rays, int n, uint64_t seed, double* out_t, int32_t* out_mat,
                       int32_t* out_draws) {
    LOCK_SCENE(s, scene);
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    if (n < 0) return fail("ray count must be >= 0");
    if (n > 0 && (!rays || !out_t || !out_mat || !out_draws)) return fail("null pointer");
    CTX_OF(c, s);
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    uint32_t stale = 0;
    HIPCHK(take_fault(&stale));
    DevBuf d_rays, d_t, d_mat, d_draws;
    HIPCHK(d_rays.ensure((size_t)n * 7 * sizeof(double)));
    HIPCHK(d_t.ensure((size_t)n * sizeof(double)));
    HIPCHK(d_mat.ensure((size_t)n * sizeof(int32_t)));
    HIPCHK(d_draws.ensure((size_t)n * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(d_rays.p, rays, (size_t)n * 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_hit_rays_stream(s->dev, d_rays.as<const double>(), (uint32_t)n, (uint32_t)seed, (uint32_t)(seed >> 32),
                                  d_t.as<double>(), d_mat.as<int32_t>(), d_draws.as<int32_t>(), c->stream));
    HIPCHK(hipMemcpyAsync(out_t, d_t.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_mat, d_mat.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_draws, d_draws.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    uint32_t f = 0;
    HIPCHK(take_fault(&f));
    if (f) return fail(fault_text(f));
    return 0;
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
    HIPCHK(hipSetDevice(c->device));
    uint32_t stale = 0;
    HIPCHK(take_fault(&stale));
    const size_t n3 = (size_t)n * 3 * sizeof(double), n1 = (size_t)n * sizeof(double);
    DevBuf d_pts, d_dirs, d_out, d_pdf, d_pdfd, d_draws;
    HIPCHK(d_pts.ensure(n3));
    HIPCHK(d_out.ensure(n3));
    HIPCHK(d_pdf.ensure(n1));
    HIPCHK(d_draws.ensure((size_t)n * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(d_pts.p, points, n3, hipMemcpyHostToDevice, c->stream));
    if (dirs) {
        HIPCHK(d_dirs.ensure(n3));
        HIPCHK(d_pdfd.ensure(n1));
        HIPCHK(hipMemcpyAsync(d_dirs.p, dirs, n3, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(launch_light_probe(s->dev, s->d_dev.as<const DevScene>(), scene_exact_libm(*c, *s), d_pts.as<const double>(),
                              dirs ? d_dirs.as<const double>() : nullptr, (uint32_t)n, (uint32_t)seed, (uint32_t)(seed >> 32),
                              d_out.as<double>(), d_pdf.as<double>(), dirs ? d_pdfd.as<double>() : nullptr,
                              d_draws.as<int32_t>(), c->stream));
    HIPCHK(hipMemcpyAsync(out_dir, d_out.p, n3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_pdf, d_pdf.p, n1, hipMemcpyDeviceToHost, c->stream));
    if (dirs) HIPCHK(hipMemcpyAsync(out_pdf_dirs, d_pdfd.p, n1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(out_draws, d_draws.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    uint32_t f = 0;
    HIPCHK(take_fault(&f));
    if (f) return fail(fault_text(f));
    return 0;
}

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
    if (mode != RT_STEP_STEP && mode != RT_STEP_TAIL) return fail("rt_step_rays: unknown mode " + std::to_string(mode));
    if (extend == RT_STEP_EXTEND_LDS && depth == 0)
        return fail("rt_step_rays: the LDS extend serves depth >= 1 only (depth 0 is k_extend or k_camera)");
    if (extend == RT_STEP_EXTEND_LDS && s->ext_lds == 0)
        return fail("rt_step_rays: this scene's time-0 tree does not run from LDS (rt_scene_info.extend_lds_bytes is 0)");
    if (curve_kernel_scene(s->dev))
        return fail("rt_step_rays: this scene's renders take the persistent curve kernel, which the probe does not drive");
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
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    {
        uint32_t stale = 0;
        HIPCHK(take_fault(&stale));
        const char* e = std::getenv("RTAMD_REJECT_CAP");
        HIPCHK(set_test_caps(e ? std::max(0, std::atoi(e)) : 4096, 0u));
    }
    // the layout of a render of n paths in one chunk (render_impl)
    const size_t cap = (size_t)n;
    const size_t gmax = std::min<size_t>(4096, (cap + 255) / 256 + kShards);
    const size_t slack = 4 * 32 * gmax + 256;
    const size_t shard_cap = (cap + kShards - 1) / kShards + slack;
    const size_t scap = shard_cap * kShards;
    constexpr int kCountsPerIter = 5 * kShards * kCntStride;
    DevBuf b_a, b_b, b_hit, b_sb, b_cnt, b_ctl, b_pix;
    HIPCHK(b_a.ensure(scap * kStateBytesA));
    HIPCHK(b_b.ensure(scap * kStateBytesA));            // (either pool may be the depth's input: both carved alike)
    HIPCHK(b_hit.ensure(scap * kHitBytesPerPath));
    HIPCHK(b_sb.ensure(cap * 3 * sizeof(double)));
    HIPCHK(b_cnt.ensure(2 * kCountsPerIter * sizeof(uint32_t)));     // row 0: the previous depth's, row 1: this one's
    HIPCHK(b_ctl.ensure(4 * sizeof(unsigned long long)));
    HIPCHK(b_pix.ensure(cap * sizeof(uint32_t)));
    PathState A = carve_state(b_a.p, scap, true), B = carve_state(b_b.p, scap, true);
    PathState* cur = (depth & 1) ? &B : &A;             // a chunk starts in pool A and swaps every depth
    PathState* nxt = (depth & 1) ? &A : &B;

    // host images of the input state
    std::vector<uint32_t> h_pix(cap), slot_of(cap), h_prev(kCountsPerIter, 0u);
    for (size_t k = 0; k < cap; ++k) h_pix[k] = pix ? pix[k] : (uint32_t)k;
    std::vector<RayRec> h_ray(scap);
    std::vector<PathRec> h_path(scap);
    std::vector<double> h_tm(scap, 0.0);
    std::vector<uint32_t> h_rng0(scap, 0u);
    std::memset(h_ray.data(), 0, scap * sizeof(RayRec));
    std::memset(h_path.data(), 0, scap * sizeof(PathRec));
    for (size_t k = 0; k < cap; ++k) {
        size_t slot = k;
        if (depth > 0) {
            const size_t shard = (k / 256) % kShards;
            slot = shard * shard_cap + h_prev[(4 * kShards + shard) * kCntStride]++;
        }
        slot_of[k] = (uint32_t)slot;
        const double* r = rays + 7 * k;
        RayRec R{};
        R.ox = r[0]; R.oy = r[1]; R.oz = r[2]; R.dx = r[3]; R.dy = r[4]; R.dz = r[5];
        h_ray[slot] = R;
        if (depth == 0) {
            h_tm[slot] = r[6];
            h_rng0[slot] = ctr_in[k];
        } else {
            PathRec P{};
            P.tr = T_in[3 * k]; P.tg = T_in[3 * k + 1]; P.tb = T_in[3 * k + 2];
            P.wid = (uint32_t)k; P.rng = ctr_in[k];
            h_path[slot] = P;
        }
    }
    std::vector<uint32_t> key_of(scap, 0xFFFFFFFFu);      // input slot -> record
    for (size_t k = 0; k < cap; ++k) key_of[slot_of[k]] = (uint32_t)k;
    std::vector<uint64_t> h_sb(cap * 3, (uint64_t)RT_STEP_SENTINEL);

    HIPCHK(hipMemcpyAsync(cur->ray, h_ray.data(), scap * sizeof(RayRec), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cur->path, h_path.data(), scap * sizeof(PathRec), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cur->tm, h_tm.data(), scap * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cur->rng0, h_rng0.data(), scap * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(nxt->ray, 0, scap * sizeof(RayRec), st));
    HIPCHK(hipMemsetAsync(nxt->path, 0xFF, scap * sizeof(PathRec), st));
    HIPCHK(hipMemcpyAsync(b_pix.p, h_pix.data(), cap * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b_sb.p, h_sb.data(), cap * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b_cnt.p, 0, 2 * kCountsPerIter * sizeof(uint32_t), st));
    HIPCHK(hipMemcpyAsync(b_cnt.p, h_prev.data(), kCountsPerIter * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(b_hit.p, 0, scap * kHitBytesPerPath, st));
    HIPCHK(hipMemsetAsync(b_ctl.p, 0, 4 * sizeof(unsigned long long), st));

    RenderParams rp{};
    rp.nx = (uint32_t)n; rp.ny = 1u; rp.npix = (uint32_t)n;
    rp.inx = 1.0 / (double)n; rp.iny = 1.0;
    rp.spp0 = smp; rp.k0 = (uint32_t)seed; rp.k1 = (uint32_t)(seed >> 32);
    rp.pixlist = b_pix.as<const uint32_t>();
    rp.sb = b_sb.as<double>();
    rp.B = (uint32_t)n;
    rp.compact = 0u;
    rp.exact_libm = scene_exact_libm(*c, *s) ? 1u : 0u;
    // the survivor view of the previous depth (raygen's output is contiguous)
    const QView view = depth == 0 ? QView{nullptr, (uint32_t)scap}
                                  : QView{b_cnt.as<uint32_t>() + 4 * kShards * kCntStride, (uint32_t)shard_cap};
    uint32_t* cnt = b_cnt.as<uint32_t>() + kCountsPerIter;
    unsigned long long* ctl = b_ctl.as<unsigned long long>();
    const HitBuf hit{b_hit.as<HitRec>() + scap, (uint32_t)scap, b_hit.as<HitPt>()};
    const size_t tree0_budget = s->ext_lds ? (size_t)32 << 10 : 0;
    const bool ext_lds = extend == RT_STEP_EXTEND_LDS;
    const bool pt = s->point_hits && !point_hits_off() && ext_lds;

    if (mode == RT_STEP_TAIL) {
        const FinishInst fi = finish_instance(s->dev, rp, tree0_budget);
        const int32_t row[6] = {1, fi.f, fi.tl, fi.ls, fi.solo ? 1 : 0, fi.ex ? 1 : 0};
        std::memcpy(out_inst, row, sizeof row);
        HIPCHK(launch_finish(s->dev, s->d_dev.as<const DevScene>(), rp, *cur, view, (uint32_t)n, ctl, tree0_budget,
                             (uint32_t)depth, st));
    } else {
        if (ext_lds)
            HIPCHK(launch_extend_lds(s->dev, rp, *cur, view, (uint32_t)n, hit, pt, (uint32_t)shard_cap, cnt,
                                     s->ext_lds_blocks, ctl + 2, st));
        else
            HIPCHK(launch_extend(s->dev, s->d_dev.as<const DevScene>(), rp, *cur, view, (uint32_t)n, hit,
                                 (uint32_t)shard_cap, cnt, depth == 0, reinterpret_cast<unsigned int*>(ctl + 1), nullptr, st));
        uint32_t* surv = cnt + 4 * kShards * kCntStride;
        for (int mt = 0; mt < 4; ++mt) {
            if (!(s->dev.mat_mask & (1 << mt))) continue;
            const ShadeInst si = shade_instance(mt, s->dev, rp, pt && mt == MAT_LAMBERTIAN);
            const int32_t row[6] = {1, si.tl, si.ls, si.ll ? 1 : 0, si.ex ? 1 : 0, si.pt ? 1 : 0};
            std::memcpy(out_inst + 8 * mt, row, sizeof row);
            const QView qv{cnt + mt * kShards * kCntStride, (uint32_t)shard_cap};
            HIPCHK(launch_shade(mt, s->dev, s->d_dev.as<const DevScene>(), rp, *cur, hit, pt, qv, (uint32_t)n, *nxt, surv,
                                (uint32_t)shard_cap, (uint32_t)depth, st));
        }
    }
    // read everything back
    std::vector<uint32_t> h_cnt(kCountsPerIter);
    std::vector<HitRec> h_hit(5 * scap);
    std::vector<LeafInfo> h_leaves((size_t)std::max(0, s->dev.n_leaves));
    HIPCHK(hipMemcpyAsync(h_cnt.data(), cnt, kCountsPerIter * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_sb.data(), b_sb.p, cap * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (mode == RT_STEP_STEP) {
        HIPCHK(hipMemcpyAsync(h_ray.data(), nxt->ray, scap * sizeof(RayRec), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_path.data(), nxt->path, scap * sizeof(PathRec), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_hit.data(), b_hit.p, scap * kHitBytesPerPath, hipMemcpyDeviceToHost, st));
        if (!h_leaves.empty())
            HIPCHK(hipMemcpyAsync(h_leaves.data(), s->dev.leaves, h_leaves.size() * sizeof(LeafInfo), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    {
        uint32_t f = 0;
        HIPCHK(take_fault(&f));
        if (f) return fail(fault_text(f));
        unsigned long long h_ctl[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpy(h_ctl, b_ctl.p, sizeof h_ctl, hipMemcpyDeviceToHost));
        if (h_ctl[2]) return fail("internal: a persistent kernel's LDS allocation was too small (flags " +
                                  std::to_string(h_ctl[2]) + ")");
    }
    for (size_t k = 0; k < cap; ++k) {
        bool wrote = false;
        for (int c3 = 0; c3 < 3; ++c3) wrote = wrote || h_sb[3 * k + c3] != (uint64_t)RT_STEP_SENTINEL;
        out_status[k] = wrote ? RT_STEP_WROTE : 0;
        std::memcpy(out_color + 3 * k, &h_sb[3 * k], 3 * sizeof(double));
    }
    if (mode == RT_STEP_TAIL) return 0;
    for (size_t k = 0; k < cap; ++k) { out_t[k] = 0.0; out_mat[k] = -1; }
    uint32_t total = 0;
    for (int x = 0; x < kShards; ++x) {
        const uint32_t cx = h_cnt[(4 * kShards + x) * kCntStride];
        if (cx > shard_cap) return fail("internal: shard overflow");
        total += cx;
        for (uint32_t j = 0; j < cx; ++j) {
            const size_t slot = (size_t)x * shard_cap + j;
            const PathRec& P = h_path[slot];
            if (P.wid >= (uint32_t)n) return fail("rt_step_rays: a survivor carries work id " + std::to_string(P.wid));
            const size_t k = P.wid;
            if ((out_status[k] & 255) < 255) ++out_status[k];
            const RayRec& R = h_ray[slot];
            const double ray6[6] = {R.ox, R.oy, R.oz, R.dx, R.dy, R.dz};
            std::memcpy(out_ray + 6 * k, ray6, sizeof ray6);
            out_T[3 * k] = P.tr; out_T[3 * k + 1] = P.tg; out_T[3 * k + 2] = P.tb;
            out_ctr[k] = P.rng;
        }
    }
    *out_survivors = total;
    // the hit queues: HitBuf's layout (queue m of HitRec at stride (1 + m); the point records from the start)
    const HitPt* h_pt = reinterpret_cast<const HitPt*>(h_hit.data());
    for (int mt = 0; mt < 4; ++mt)
        for (int x = 0; x < kShards; ++x) {
            const uint32_t cx = std::min<uint32_t>(h_cnt[(mt * kShards + x) * kCntStride], (uint32_t)shard_cap);
            for (uint32_t j = 0; j < cx; ++j) {
                const size_t q = (size_t)x * shard_cap + j;
                int32_t leaf; uint32_t slot; double t;
                if (pt && mt == MAT_LAMBERTIAN) { leaf = h_pt[q].leaf; slot = h_pt[q].slot; t = std::nan(""); }
                else { const HitRec& H = h_hit[(size_t)(1 + mt) * scap + q]; leaf = H.leaf; slot = H.slot; t = H.t; }
                if (slot >= scap || key_of[slot] == 0xFFFFFFFFu || leaf < 0 || leaf >= s->dev.n_leaves)
                    return fail("rt_step_rays: a hit queue holds a record of no input path");
                out_t[key_of[slot]] = t;
                out_mat[key_of[slot]] = h_leaves[leaf].mat;
            }
        }
    return 0;
}

int rt_curve_depth_probe(int ctx, int n, const double* cps, const double* eps8, int32_t* out_depth) {
    LOCK_CTX(c, ctx);
    if (n < 0) return fail("curve count must be >= 0");
    if (n == 0) return 0;
    if (!cps || !eps8 || !out_depth) return fail("null pointer");
    HIPCHK(hipSetDevice(c->device));
    DevBuf d_cps, d_eps, d_out;
    HIPCHK(d_cps.ensure((size_t)n * 12 * sizeof(double)));
    HIPCHK(d_eps.ensure((size_t)n * sizeof(double)));
    HIPCHK(d_out.ensure((size_t)n * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(d_cps.p, cps, (size_t)n * 12 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_eps.p, eps8, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_curve_depth(d_cps.as<const double>(), d_eps.as<const double>(), (uint32_t)n, d_out.as<int32_t>(),
                              c->stream));
    HIPCHK(hipMemcpyAsync(out_depth, d_out.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

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
