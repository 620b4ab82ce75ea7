// plan_check.cpp — the render scheduler's arithmetic and pool layout (scheme-raytrace_amd/csrc/rt_plan.h)
// against the formulas the scheduler had inline before they were moved there, restated here literally as the
// specification (ref_*), over grids of sizes; and the layout's own invariants (no overlap, alignment, bounds).
// Host code with its own main, compiled with g++ under ASan / UBSan (tests/test_plan_host.py).  Prints one JSON
// object: per section its failed checks (none expected) and the pinned values the test compares.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../../scheme-raytrace_amd/csrc/rt_plan.h"

using namespace rtamd;

namespace {
std::vector<std::string> g_fail;                     // the current section's failed checks
#define CHECK(cond) do { if (!(cond)) g_fail.push_back(std::string(#cond) + " @" + std::to_string(__LINE__)); } while (0)
bool g_first = true;
void section(const char* name, const std::string& values) {
    std::printf("%s\"%s\": {\"failed\": [", g_first ? "{" : ", ", name);
    for (size_t i = 0; i < g_fail.size() && i < 8; ++i) std::printf("%s\"%s\"", i ? ", " : "", g_fail[i].c_str());
    std::printf("], \"nfailed\": %zu, \"values\": [%s]}", g_fail.size(), values.c_str());
    g_fail.clear();
    g_first = false;
}

// ---------------------------------------------------------------- the specification
struct RefLayout { size_t shard_cap, scap; };
RefLayout ref_layout(const size_t cap, const size_t slack_override) {
    const size_t gmax = std::min<size_t>(4096, (cap + 255) / 256 + 8);
    size_t slack = 4 * 32 * gmax + 256;
    if (slack_override) slack = std::max<size_t>(256, slack_override);
    const size_t shard_cap = (cap + 8 - 1) / 8 + slack;
    return RefLayout{shard_cap, shard_cap * 8};
}
struct RefPlan { uint32_t chunk; int nchunks, nlanes; };
RefPlan ref_plan(const uint32_t npix, const int spp_count, const size_t cap_paths, const int lanes_for) {
    uint32_t chunk = (uint32_t)std::max<size_t>(1, cap_paths / npix);
    if (chunk > (uint32_t)spp_count) chunk = (uint32_t)spp_count;
    {
        const int min_chunks = lanes_for;
        int n = (int)((spp_count + chunk - 1) / chunk);
        if (n < min_chunks) n = std::min(min_chunks, spp_count);
        if (n > 1 && (n & 1) && n < spp_count) ++n;
        chunk = (uint32_t)((spp_count + n - 1) / n);
    }
    const int nchunks = (int)((spp_count + chunk - 1) / chunk);
    const int nlanes = std::max(1, std::min(std::min(4, lanes_for), nchunks));
    return RefPlan{chunk, nchunks, nlanes};
}
uint32_t ref_tail(const bool wavefront_only, const int64_t opt_tail_paths, const int64_t opt_tail_div, const uint32_t B,
                  const int nchunks, const bool curves) {
    if (wavefront_only) return 0u;
    if (opt_tail_paths <= 0 && opt_tail_div <= 0 && !curves) {
        if (nchunks == 1) return std::max<uint32_t>(std::max<uint32_t>(32768u, std::min<uint32_t>(B / 4u, 524288u)), B / 256u);
        return std::max<uint32_t>(std::max<uint32_t>(32768u, std::min<uint32_t>(B / 64u, 262144u)), B / 256u);
    }
    const uint32_t thr = opt_tail_paths > 0 ? (uint32_t)std::min<int64_t>(opt_tail_paths, 0xFFFFFFFFll) : 32768u;
    const uint32_t div = opt_tail_div > 0 ? (uint32_t)std::min<int64_t>(opt_tail_div, 0xFFFFFFFFll) : 256u;
    return std::max<uint32_t>(thr, B / div);
}
size_t ref_pool_cap(const size_t free_b, const int lanes, const int64_t opt_max_paths) {
    if (opt_max_paths > 0) return opt_max_paths < 1024 ? 1024 : (size_t)opt_max_paths;
    size_t v = (size_t)384 << 20;
    if (free_b > 0) {
        const size_t fit = free_b / 100 * 65 / ((size_t)std::max(1, lanes) * 276);
        if (fit < v) v = fit;
    }
    return v < ((size_t)1 << 20) ? ((size_t)1 << 20) : v;
}

// ---------------------------------------------------------------- sections
void check_pool_layout() {
    const size_t caps[] = {1, 255, 256, 257, 2047, 2048, 92160, (size_t)1 << 20, 24883200, (size_t)384 << 20};
    char* const base = reinterpret_cast<char*>(uintptr_t(1) << 20);      // an address to carve; never dereferenced
    for (size_t cap : caps)
        for (size_t ovr : {(size_t)0, (size_t)1, (size_t)256, (size_t)1000}) {
            const PoolLayout L = pool_layout(cap, ovr);
            const RefLayout R = ref_layout(cap, ovr);
            CHECK(L.cap == cap && L.shard_cap == R.shard_cap && L.scap == R.scap);
            CHECK(L.state_a_bytes == R.scap * 92 && L.state_b_bytes == R.scap * 80);
            CHECK(L.hit_bytes == R.scap * 80 && L.sb_bytes == cap * 24);
            CHECK(L.scap >= cap && L.scap < ((size_t)1 << 32));
            // carve_state: four arrays of scap elements, in order, none overlapping, inside the pool
            for (bool depth0 : {true, false}) {
                const PathState st = carve_state(base, L.scap, depth0);
                const size_t ray = (size_t)(reinterpret_cast<char*>(st.ray) - base);
                const size_t path = (size_t)(reinterpret_cast<char*>(st.path) - base);
                CHECK(ray == 0 && path >= ray + L.scap * sizeof(RayRec) && path % sizeof(PathRec) == 0);
                if (!depth0) {
                    CHECK(st.tm == nullptr && st.rng0 == nullptr);
                    CHECK(path + L.scap * sizeof(PathRec) <= L.state_b_bytes);
                    continue;
                }
                const size_t tm = (size_t)(reinterpret_cast<char*>(st.tm) - base);
                const size_t rng0 = (size_t)(reinterpret_cast<char*>(st.rng0) - base);
                CHECK(tm >= path + L.scap * sizeof(PathRec) && tm % sizeof(double) == 0);
                CHECK(rng0 >= tm + L.scap * sizeof(double) && rng0 % sizeof(uint32_t) == 0);
                CHECK(rng0 + L.scap * sizeof(uint32_t) <= L.scap * kStateBytesA);
            }
            // hit_buf: five strides of 16 B; the point records over the first two, queue m of HitRec at stride 1 + m
            const HitBuf hb = hit_buf(base, L);
            CHECK(hb.stride == L.scap && reinterpret_cast<char*>(hb.hp) == base);
            CHECK(reinterpret_cast<char*>(hb.h) == base + L.scap * 16);
            CHECK(reinterpret_cast<char*>(hb.hp + L.scap) == base + 2 * L.scap * 16);
            CHECK(reinterpret_cast<char*>(hb.h + 4 * (size_t)hb.stride) == base + L.hit_bytes && L.hit_bytes == 5 * L.scap * 16);
        }
    // the counter rows: four material blocks and the survivors', kShards counters each, a 128-B line apart
    std::vector<uint32_t> row(kCountsPerIter, 0u);
    for (int m = 0; m < 4; ++m) CHECK(hit_counts(row.data(), m) == row.data() + m * 256);
    CHECK(survivor_counts(row.data()) == row.data() + 1024 && kCountsPerIter == 1280 && kIters == 104);
    for (int x = 0; x < kShards; ++x) survivor_counts(row.data())[x * 32] = 100u + x;
    for (int x = 0; x < kShards; ++x) CHECK(shard_count(survivor_counts(row.data()), x) == 100u + x);
    CHECK(kCtlSegments == 0 && kCtlClaim == 1 && kCtlLdsErr == 2 && kCtlFuseSegs == 3 && kCtlWords == 4);
    section("pool_layout", "");
}

void check_plan_render() {
    const uint32_t npixs[] = {1, 4096, 30720, 2073600};
    const size_t caps[] = {1024, 92160, (size_t)1 << 20, (size_t)384 << 20};
    std::vector<int> spps;
    for (int s = 1; s <= 40; ++s) spps.push_back(s);
    spps.push_back(1024);
    for (uint32_t npix : npixs)
        for (int spp : spps)
            for (size_t cap : caps)
                for (int lanes = 1; lanes <= 4; ++lanes) {
                    const RenderPlan P = plan_render(npix, spp, cap, lanes);
                    const RefPlan R = ref_plan(npix, spp, cap, lanes);
                    CHECK(P.chunk == R.chunk && P.nchunks == R.nchunks && P.nlanes == R.nlanes);
                    CHECK((int64_t)(P.nchunks - 1) * P.chunk < spp && spp <= (int64_t)P.nchunks * P.chunk);
                    CHECK(1 <= P.nlanes && P.nlanes <= std::min(lanes, P.nchunks));
                }
    std::string v;
    const struct { uint32_t npix; int spp; size_t cap; int lanes; } pinned[] = {
        {30720, 24, 92160, 2}, {30720, 9, 92160, 2}, {30720, 1, 92160, 2}, {4096, 2, 1024, 2}};
    for (const auto& p : pinned) {
        const RenderPlan P = plan_render(p.npix, p.spp, p.cap, p.lanes);
        v += (v.empty() ? "[" : ", [") + std::to_string(P.chunk) + ", " + std::to_string(P.nchunks) + ", " +
             std::to_string(P.nlanes) + "]";
    }
    section("plan_render", v);
}

void check_tail_paths() {
    const uint32_t Bs[] = {1, 32768, 131072, 2073600, 8294400, 268435456, 0xFFFFFFFFu};
    for (uint32_t B : Bs)
        for (int nchunks : {1, 2, 6})
            for (bool off : {false, true})
                for (int64_t tp : {(int64_t)0, (int64_t)1000, (int64_t)1 << 30, (int64_t)1 << 40})
                    for (int64_t td : {(int64_t)0, (int64_t)128, (int64_t)1 << 40})
                        for (bool curves : {false, true}) {
                            CHECK(tail_paths(TailOpts{off, tp, td, curves}, B, nchunks) == ref_tail(off, tp, td, B, nchunks, curves));
                            if (off) CHECK(tail_paths(TailOpts{off, tp, td, curves}, B, nchunks) == 0u);
                            if (!off && tp == 0 && td == 128)
                                CHECK(tail_paths(TailOpts{off, tp, td, curves}, B, nchunks) == std::max<uint32_t>(32768u, B / 128u));
                        }
    const TailOpts none{false, 0, 0, false}, curves{false, 0, 0, true};
    const std::string v = std::to_string(tail_paths(none, 2073600u, 1)) + ", " + std::to_string(tail_paths(none, 8294400u, 2)) +
                          ", " + std::to_string(tail_paths(none, 268435456u, 1)) + ", " +
                          std::to_string(tail_paths(curves, 2073600u, 1)) + ", " + std::to_string(tail_paths(curves, 2073600u, 2));
    section("tail_paths", v);
}

void check_pool_cap() {
    const size_t frees[] = {0, 1, (size_t)1 << 29, (size_t)1 << 30, (size_t)64 << 30, 288000000000ull, (size_t)1 << 42};
    for (size_t f : frees)
        for (int lanes = 0; lanes <= 4; ++lanes)
            for (int64_t opt : {(int64_t)0, (int64_t)1, (int64_t)500, (int64_t)1024, (int64_t)5000000})
                CHECK(pool_cap_for(f, lanes, opt) == ref_pool_cap(f, lanes, opt));
    CHECK(pool_cap_for(288000000000ull, 2, 0) == std::min<size_t>(288000000000ull / 100 * 65 / (2 * 276), (size_t)384 << 20));
    const std::string v = std::to_string(pool_cap_for(0, 2, 500)) + ", " + std::to_string(pool_cap_for(0, 2, 0)) + ", " +
                          std::to_string(pool_cap_for((size_t)1 << 30, 2, 0)) + ", " +
                          std::to_string(pool_cap_for((size_t)1 << 30, 4, 0)) + ", " +
                          std::to_string(pool_cap_for(288000000000ull, 2, 0));
    section("pool_cap_for", v);
}

void check_step_slot() {
    for (size_t n : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)2049})
        for (int depth : {0, 1}) {
            const PoolLayout L = pool_layout(n, 0);
            std::vector<uint32_t> row(kCountsPerIter, 0u);
            std::vector<size_t> slot(n);
            std::set<size_t> seen;
            for (size_t k = 0; k < n; ++k) {
                slot[k] = step_slot(k, depth, L, survivor_counts(row.data()));
                CHECK(slot[k] < L.scap);
                seen.insert(slot[k]);
                if (depth == 0) CHECK(slot[k] == k);
                else CHECK(slot[k] / L.shard_cap == (k / 256) % 8);
            }
            CHECK(seen.size() == n);
            size_t sum = 0;
            for (int x = 0; x < kShards; ++x) {
                const uint32_t cx = shard_count(survivor_counts(row.data()), x);
                CHECK(cx <= L.shard_cap);
                sum += cx;
            }
            CHECK(sum == (depth == 0 ? 0 : n));       // depth 0 is contiguous: no shard counters
            for (size_t i = 0; i < 1024; ++i) CHECK(row[i] == 0u);     // the hit counters are not touched
            if (depth >= 1)
                for (size_t k = 0; k + 256 * 8 < n; ++k) CHECK(slot[k] / L.shard_cap == slot[k + 256 * 8] / L.shard_cap);
        }
    section("step_slot", "");
}
}  // namespace

int main() {
    check_pool_layout();
    check_plan_render();
    check_tail_paths();
    check_pool_cap();
    check_step_slot();
    std::printf("}\n");
    return 0;
}
