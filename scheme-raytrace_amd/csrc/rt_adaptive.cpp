// rt_adaptive.cpp — adaptive sampling (include/rt.h): the selection of the not-converged pixels, the
// driver that renders them round by round, and the pixel-list render and per-count resolve entry points.
#include <algorithm>
#include <chrono>
#include <cmath>

#include "rt_host.h"
#include "rt_launch.h"

using namespace rtamd;

namespace {
int check_rule(double tol, double flr) {
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail("tol must be finite and >= 0");
    if (!(flr >= 0.0) || !std::isfinite(flr)) return fail("floor must be finite and >= 0");
    return 0;
}
int check_adaptive(const rt_adaptive* p) {
    if (!p) return fail("null rt_adaptive parameters");
    if (p->min_spp < 2) return fail("min_spp must be >= 2 (the variance of the mean needs two samples)");
    if (p->max_spp < p->min_spp) return fail("max_spp must be >= min_spp");
    if (p->max_spp > 0x7FFFFFFFu) return fail("max_spp out of range");
    if (p->batch_spp < 1) return fail("batch_spp must be >= 1");
    return check_rule(p->tol, p->floor);
}
// the not-converged entries of pix_in (null: 0..n-1) into pix_out, their number and the capped ones'
// to the host: three launches, one 16-byte copy, one synchronise
int select_impl(Context* c, const uint32_t* pix_in, uint32_t n, const double* accum, const double* accum2,
                const uint32_t* count, double tol, double flr, uint32_t max_spp, uint32_t* pix_out, int64_t* out_n,
                int64_t* out_capped, hipStream_t st) {
    HIPCHK(c->sel_scratch.ensure(std::max<size_t>(1, 3 * (size_t)select_blocks(n)) * sizeof(uint32_t)));
    HIPCHK(c->sel_words.ensure(3 * sizeof(unsigned long long)));
    unsigned long long* words = c->sel_words.as<unsigned long long>();
    HIPCHK(launch_select(pix_in, n, accum, accum2, count, tol, flr, max_spp, c->sel_scratch.as<uint32_t>(), words, pix_out, st));
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, words, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[0] > n || h[1] > h[0]) return fail("internal: the selection's counters are out of range");
    *out_n = (int64_t)h[0];
    *out_capped = (int64_t)h[1];
    return 0;
}
double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
// The adaptive driver: round 0 = passes [0, min_spp) of every pixel, each later round the next batch_spp
// passes (the last cut at max_spp) of the still-active list; after every round the selection into the
// other list buffer.  Stops when the list is empty or max_spp is reached.
int adaptive_impl(Scene* s, Context* c, int nx, int ny, const rt_adaptive& p, uint64_t seed, double* accum, double* accum2,
                  uint32_t* count, hipStream_t st, rt_adaptive_result* out) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    HIPCHK(hipSetDevice(c->device));
    if (!st) st = c->stream;
    const std::vector<uint32_t> pl = make_pixlist(nx, ny, full_frame(ny));
    const size_t npx = pl.size();
    for (DevBuf& b : c->sel_list) HIPCHK(b.ensure(npx * sizeof(uint32_t)));
    HIPCHK(hipMemsetAsync(accum, 0, npx * 3 * sizeof(double), st));
    HIPCHK(hipMemsetAsync(accum2, 0, npx * 3 * sizeof(double), st));
    HIPCHK(hipMemsetAsync(count, 0, npx * sizeof(uint32_t), st));
    HIPCHK(hipMemcpyAsync(c->sel_list[0].p, pl.data(), npx * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    rt_adaptive_result r{};
    rt_stats total{};
    int cur = 0;
    int64_t active = (int64_t)npx, capped = 0;
    uint32_t done = 0;
    while (active > 0 && done < p.max_spp) {
        const uint32_t passes = done == 0 ? p.min_spp : std::min(p.batch_spp, p.max_spp - done);
        const PixSet px{c->sel_list[cur].as<const uint32_t>(), (uint32_t)active, false, accum2, count};
        if (int rc = render_impl(s, nx, ny, px, (int)done, (int)passes, seed, accum, st)) return rc;
        total.segments += s->stats.segments;
        total.paths += s->stats.paths;
        total.extend_rays += s->stats.extend_rays;
        total.finish_paths += s->stats.finish_paths;
        total.chunks += s->stats.chunks;
        total.lanes = std::max(total.lanes, s->stats.lanes);
        total.max_depth_seen = std::max(total.max_depth_seen, s->stats.max_depth_seen);
        done += passes;
        r.samples += (uint64_t)active * passes;
        r.rounds += 1;
        const auto ts = std::chrono::steady_clock::now();
        if (int rc = select_impl(c, px.pix, px.n, accum, accum2, count, p.tol, p.floor, p.max_spp,
                                 c->sel_list[cur ^ 1].as<uint32_t>(), &active, &capped, st))
            return rc;
        r.ms_select += ms_since(ts);
        cur ^= 1;
    }
    r.pixels_capped = (uint64_t)capped;
    r.pixels_converged = (uint64_t)npx - (uint64_t)capped;
    r.ms_total = ms_since(t0);
    total.ms_total = r.ms_total;
    s->stats = total;                                  // rt_get_stats: the rounds together
    if (out) *out = r;
    return 0;
}
}  // namespace

extern "C" {

int rt_render_pixels_device(int scene, int nx, int ny, const uint32_t* pix_device, int64_t n, int spp_begin, int spp_count,
                            uint64_t seed, double* accum, double* accum2, uint32_t* count, void* stream) {
    if (int rc = check_frame(nx, ny)) return rc;
    if (!pix_device) return fail("null pixel list");
    if (!accum) return fail("null accum");
    if (n < 0 || n > (int64_t)nx * ny) return fail("pixel list length " + std::to_string(n) + " outside 0 .. nx*ny");
    if (spp_begin < 0 || spp_count < 0) return fail("spp_begin/spp_count must be >= 0");
    LOCK_SCENE(s, scene);
    CTX_OF(c, s);
    if (n == 0 || spp_count == 0) return 0;
    CTX_STREAM(c, st, stream);
    // the list's range, read only, before any kernel writes through it
    HIPCHK(c->sel_words.ensure(3 * sizeof(unsigned long long)));
    uint32_t* d_max = reinterpret_cast<uint32_t*>(c->sel_words.as<unsigned long long>() + 2);
    HIPCHK(launch_check_pixels(pix_device, (uint32_t)n, d_max, st));
    uint32_t h_max = 0;
    HIPCHK(hipMemcpyAsync(&h_max, d_max, sizeof h_max, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h_max >= (uint32_t)(nx * ny))
        return fail("pixel list entry " + std::to_string(h_max) + " is outside the frame (nx*ny = " +
                    std::to_string(nx * ny) + ")");
    const PixSet px{pix_device, (uint32_t)n, false, accum2, count};
    return render_impl(s, nx, ny, px, spp_begin, spp_count, seed, accum, st);
}

int rt_adaptive_select_device(int ctx, const uint32_t* pix_in, int64_t n, const double* accum, const double* accum2,
                              const uint32_t* count, double tol, double floor, uint32_t max_spp, uint32_t* pix_out,
                              int64_t* out_n, int64_t* out_capped, void* stream) {
    if (!accum || !accum2 || !count || !pix_out || !out_n || !out_capped) return fail("null pointer");
    if (n < 0 || n >= (1ll << 31)) return fail("pixel list length " + std::to_string(n) + " out of range");
    if (int rc = check_rule(tol, floor)) return rc;
    if (pix_in == pix_out) return fail("pix_out must not be pix_in");
    LOCK_CTX(c, ctx);
    *out_n = 0;
    *out_capped = 0;
    if (n == 0) return 0;
    CTX_STREAM(c, st, stream);
    return select_impl(c, pix_in, (uint32_t)n, accum, accum2, count, tol, floor, max_spp, pix_out, out_n, out_capped, st);
}

int rt_render_adaptive_device(int scene, int nx, int ny, const rt_adaptive* p, uint64_t seed, double* accum, double* accum2,
                              uint32_t* count, void* stream, rt_adaptive_result* out) {
    if (int rc = check_frame(nx, ny)) return rc;
    if (int rc = check_adaptive(p)) return rc;
    if (!accum || !accum2 || !count) return fail("null buffer");
    LOCK_SCENE(s, scene);
    CTX_OF(c, s);
    return adaptive_impl(s, c, nx, ny, *p, seed, accum, accum2, count, (hipStream_t)stream, out);
}

int rt_render_adaptive(int scene, int nx, int ny, const rt_adaptive* p, uint64_t seed, double* accum_host,
                       double* accum2_host, uint32_t* count_host, rt_adaptive_result* out) {
    if (int rc = check_frame(nx, ny)) return rc;
    if (int rc = check_adaptive(p)) return rc;
    if (!accum_host || !accum2_host || !count_host) return fail("null buffer");
    LOCK_SCENE(s, scene);
    CTX_OF(c, s);
    HIPCHK(hipSetDevice(c->device));
    const size_t npx = (size_t)nx * ny;
    HIPCHK(c->accum_tmp.ensure(npx * 3 * sizeof(double)));
    HIPCHK(c->accum2_tmp.ensure(npx * 3 * sizeof(double)));
    HIPCHK(c->count_tmp.ensure(npx * sizeof(uint32_t)));
    if (int rc = adaptive_impl(s, c, nx, ny, *p, seed, c->accum_tmp.as<double>(), c->accum2_tmp.as<double>(),
                               c->count_tmp.as<uint32_t>(), c->stream, out))
        return rc;
    HIPCHK(hipMemcpyAsync(accum_host, c->accum_tmp.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(accum2_host, c->accum2_tmp.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(count_host, c->count_tmp.p, npx * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int rt_resolve_u8_counts(const double* accum, const uint32_t* count, int nx, int ny, uint8_t* out) {
    if (!accum || !count || !out) return fail("null buffer");
    if (nx <= 0 || ny <= 0) return fail("image size must be positive");
    const size_t n = (size_t)nx * ny * 3;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t cnt = count[i / 3];
        if (cnt == 0) { out[i] = 0; continue; }
        const double c = std::sqrt(accum[i] / (double)cnt);
        const double m = (1.0 < c) ? 1.0 : c;
        out[i] = (uint8_t)std::floor(255.99 * m);
    }
    return 0;
}

int rt_resolve_u8_counts_device(int ctx, const double* accum, const uint32_t* count, int nx, int ny, uint8_t* out,
                                void* stream) {
    if (!accum || !count || !out) return fail("null buffer");
    if (int rc = check_frame(nx, ny)) return rc;
    LOCK_CTX(c, ctx);
    CTX_STREAM(c, st, stream);
    HIPCHK(launch_resolve_u8_counts(accum, count, (uint32_t)((size_t)nx * ny * 3), out, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
