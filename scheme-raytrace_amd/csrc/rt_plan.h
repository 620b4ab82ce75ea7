// rt_plan.h — the render scheduler's arithmetic (rt_render.cpp) and the layout of a lane's pools, as pure
// functions and constants: how many paths a pool holds, how a render cuts into chunks and lanes, where the
// tail kernel takes over, how one pool is carved into shards, queues and counters.  Host code only (no HIP):
// tests/csrc/plan_check.cpp compiles it with g++ and sweeps it; rt_render.cpp and rt_probe.cpp (rt_step_rays)
// lay their pools out through it, so the probe's layout is a render's by construction.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "rt_device.h"

namespace rtamd {

constexpr int kLanes = 4;                  // most lanes a render may use (RT_OPT_LANES)

// ------------------------------------------------------------ pool sizing
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
#ifndef RT_F32_RECORDS
static_assert(kPoolBytesPerPath == 276, "a lane's pools per path");
#endif
// free_bytes: the device's free memory (0: unknown); opt_max_paths: RT_OPT_MAX_PATHS (0: sized from it)
inline size_t pool_cap_for(const size_t free_bytes, const int lanes, const int64_t opt_max_paths) {
    if (opt_max_paths > 0) return opt_max_paths < 1024 ? 1024 : (size_t)opt_max_paths;
    size_t v = (size_t)384 << 20;
    if (free_bytes > 0) {
        const size_t fit = free_bytes / 100 * 65 / ((size_t)std::max(1, lanes) * kPoolBytesPerPath);
        if (fit < v) v = fit;
    }
    return v < ((size_t)1 << 20) ? ((size_t)1 << 20) : v;
}

// ------------------------------------------------------------ chunks and lanes
// Chunks of samples: as few as the pool cap allows, but at least two (one
// per render lane) and an even count when the samples allow, so the two
// lanes end together (a frame of three chunks would leave one lane alone
// for a third of it).  A floor of four cost 6.5 % on a 1/8-frame shard
// (680x381x1024 spp, the per-rank work at 8 GPUs) and 2.4 % at 1/4
// (profiles/r02/mc/).
// chunk: passes per chunk (the last one may hold fewer); lanes_for_scene: the lanes the scene's renders take
struct RenderPlan { uint32_t chunk; int nchunks, nlanes; };
inline RenderPlan plan_render(const uint32_t npix, const int spp_count, const size_t pool_cap, const int lanes_for_scene) {
    uint32_t chunk = (uint32_t)std::max<size_t>(1, pool_cap / npix);
    if (chunk > (uint32_t)spp_count) chunk = (uint32_t)spp_count;
    {
        const int min_chunks = lanes_for_scene;         // one chunk per lane at least
        int n = (int)((spp_count + chunk - 1) / chunk);
        if (n < min_chunks) n = std::min(min_chunks, spp_count);
        if (n > 1 && (n & 1) && n < spp_count) ++n;
        chunk = (uint32_t)((spp_count + n - 1) / n);
    }
    const int nchunks = (int)((spp_count + chunk - 1) / chunk);
    const int nlanes = std::max(1, std::min(std::min(kLanes, lanes_for_scene), nchunks));
    return RenderPlan{chunk, nchunks, nlanes};
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
struct TailOpts {
    bool wavefront_only;                       // RT_OPT_TAIL_OFF
    int64_t opt_tail_paths, opt_tail_div;      // RT_OPT_TAIL_PATHS, RT_OPT_TAIL_DIV (0: the rule above)
    bool curves;                               // a curve-kernel scene
};
inline uint32_t tail_paths(const TailOpts& o, const uint32_t B, const int nchunks) {
    if (o.wavefront_only) return 0u;
    if (o.opt_tail_paths <= 0 && o.opt_tail_div <= 0 && !o.curves) {
        // (bounded: a large single chunk — one render lane, e.g. Cornell at 256 spp, 268M paths — keeps B/256;
        // B/4 there handed a quarter of the paths to the tail kernel: 100.6 of 213 ms)
        if (nchunks == 1) return std::max<uint32_t>(std::max<uint32_t>(32768u, std::min<uint32_t>(B / 4u, 524288u)), B / 256u);
        return std::max<uint32_t>(std::max<uint32_t>(32768u, std::min<uint32_t>(B / 64u, 262144u)), B / 256u);
    }
    const uint32_t thr = o.opt_tail_paths > 0 ? (uint32_t)std::min<int64_t>(o.opt_tail_paths, 0xFFFFFFFFll) : 32768u;
    // B/256 with 288M-path pools (+0.9 % over B/128, profiles/r02/tail*/; B/128 was best with 96M pools)
    const uint32_t div = o.opt_tail_div > 0 ? (uint32_t)std::min<int64_t>(o.opt_tail_div, 0xFFFFFFFFll) : 256u;
    return std::max<uint32_t>(thr, B / div);
}

// ------------------------------------------------------------ one lane's pools
// cap: the paths of one chunk.  sharded compaction (rt_device.h kShards): shard capacity bounds what the
// blocks of one shard can append in one wavefront step (extend: one item
// per thread; the four shade kernels: grid-stride over at most 4096 blocks).  scap: the slots of a pool,
// every shard at its capacity; the *_bytes: what a lane's state pools, hit queues and sample colours take
struct PoolLayout { size_t cap, shard_cap, scap, state_a_bytes, state_b_bytes, hit_bytes, sb_bytes; };
// slack_override (0 = none; the test switch RTAMD_SHARD_SLACK): a smaller slack drives k_extend_curves' hit
// appends past their wave's shard (wave_append<true> spills into the next one); 256 still bounds the shade
// kernels' survivors
inline PoolLayout pool_layout(const size_t cap, const size_t slack_override) {
    const size_t gmax = std::min<size_t>(4096, (cap + 255) / 256 + kShards);
    size_t slack = 4 * 32 * gmax + 256;
    if (slack_override) slack = std::max<size_t>(256, slack_override);
    const size_t shard_cap = (cap + kShards - 1) / kShards + slack;
    const size_t scap = shard_cap * kShards;
    return PoolLayout{cap, shard_cap, scap, scap * kStateBytesA, scap * kStateBytesB, scap * kHitBytesPerPath,
                      cap * 3 * sizeof(double)};
}

// depth0: pool A, which also holds raygen's time and draw counter (pool B: null, never read)
inline PathState carve_state(void* base, size_t cap, const bool depth0) {
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
// the four material hit queues (sharded like the survivors) in a buffer of hit_bytes: HitBuf's layout
inline HitBuf hit_buf(void* base, const PoolLayout& lay) {
    return HitBuf{static_cast<HitRec*>(base) + lay.scap, (uint32_t)lay.scap, static_cast<HitPt*>(base)};
}

// A wavefront iteration's counters, one row per depth: [material][shard] hit counts, then the survivors'
constexpr int kCountsPerIter = 5 * kShards * kCntStride;   // 4 material hit queues + survivors, 8 shards each
constexpr int kIters = kMaxDepth + 4;
inline uint32_t* hit_counts(uint32_t* row, const int mat) { return row + mat * kShards * kCntStride; }
inline uint32_t* survivor_counts(uint32_t* row) { return row + 4 * kShards * kCntStride; }
inline uint32_t shard_count(const uint32_t* counters, const int shard) { return counters[shard * kCntStride]; }

// The control words of a lane (Lane::seg_tail): the tail kernel's segments, the next tail path / curve
// claim, the persistent kernels' LDS errors, the fused curve extend's continuation segments
enum LaneCtl { kCtlSegments = 0, kCtlClaim = 1, kCtlLdsErr = 2, kCtlFuseSegs = 3, kCtlWords = 4 };

// The slot rt_step_rays puts input record k at: raygen's output (depth 0) is contiguous; a deeper depth's
// input is the previous one's survivors, dealt here to shard (k / 256) % kShards as blocks of 256 threads
// would append them.  survivors: that previous depth's survivor counters, which this advances.
inline size_t step_slot(const size_t k, const int depth, const PoolLayout& lay, uint32_t* survivors) {
    if (depth == 0) return k;
    const size_t shard = (k / 256) % kShards;
    return shard * lay.shard_cap + survivors[shard * kCntStride]++;
}

}  // namespace rtamd
