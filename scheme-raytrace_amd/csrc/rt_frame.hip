// rt_frame.hip — CDNA4 (gfx950) frame-buffer kernels: what runs on the accumulators and pixel lists
// around a render.  None of them touches path state, the fault word or the scene (those are
// rt_kernels.hip's).
//
//   k_accumulate per-pixel running sum in sample     main.scm:480,488
//               order (deterministic, no atomics)
//   k_resolve_u8 correct-gamma + quantise            main.scm:481-491
//   k_scatter_pixels  the frame-end gather's placement of a shard's pixels
//
// Adaptive sampling (an extension, include/rt.h; *max-sample*, main.scm:433, is unused in the reference):
//   k_accumulate_moments  k_accumulate plus the samples' squares and the pixel's sample count
//   k_select_count / _scan / _scatter  stable compaction of the not-converged pixels of a list
//   k_check_pixels        a caller's pixel list's largest entry (read only)
//   k_resolve_u8_counts   k_resolve_u8 with each pixel's own sample count
//
// Denoiser (an extension, include/rt.h "denoiser"):
//   k_denoise_prepare     per pixel: the guide record (normal, depth, hit fraction) and the demodulated
//                         signal with the variance of its mean
//   k_denoise_atrous<LAST> one a-trous iteration over ping-pong signal buffers; the last one remodulates
#include <hip/hip_runtime.h>
#include "rt_device.h"
#include "rt_launch.h"
#include "rt_wave.h"

namespace rtamd {

// =====================================================================
// k_accumulate — *raw-data* running sum, samples added in order
// =====================================================================
__global__ __launch_bounds__(256) void k_accumulate(const RenderParams rp, uint32_t S,
                                                    double* __restrict__ accum) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= rp.npix) return;
    const uint32_t j = rp.compact ? q : rp.pixlist[q];
    double a0 = accum[3u * j], a1 = accum[3u * j + 1], a2 = accum[3u * j + 2];
    for (uint32_t s = 0; s < S; ++s) {                   // sample order per channel, as before
        const double* r = rp.sb + 3u * ((size_t)s * rp.npix + q);
        a0 = a0 + r[0]; a1 = a1 + r[1]; a2 = a2 + r[2];
    }
    accum[3u * j] = a0; accum[3u * j + 1] = a1; accum[3u * j + 2] = a2;
}

// main.scm:481-491 — sqrt(sum/count), floor(255.99*min(1,c))
__global__ __launch_bounds__(256) void k_resolve_u8(const double* __restrict__ accum, uint32_t n,
                                                    double count, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double c = sqrt(accum[i] / count);
    const double m = (1.0 < c) ? 1.0 : c;
    out[i] = (uint8_t)floor(255.99 * m);
}

// ------------------------------------------------------------ launchers
#define HIP_RETURN_IF(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)
hipError_t launch_accumulate(const RenderParams& rp, uint32_t S, double* accum, hipStream_t s) {
    const uint32_t blocks = (rp.npix + 255u) / 256u;
    hipLaunchKernelGGL(k_accumulate, dim3(blocks), dim3(256), 0, s, rp, S, accum);
    return hipGetLastError();
}
// the frame-end gather's placement (rt_gather_shards): shard pixel q's three sums to image pixel pix[q]
__global__ __launch_bounds__(256) void k_scatter_pixels(const double* __restrict__ src, const uint32_t* __restrict__ pix,
                                                        uint32_t n, double* __restrict__ frame) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n) return;
    const size_t j = pix[q];
    frame[3 * j] = src[3 * (size_t)q];
    frame[3 * j + 1] = src[3 * (size_t)q + 1];
    frame[3 * j + 2] = src[3 * (size_t)q + 2];
}
hipError_t launch_scatter_pixels(const double* src, const uint32_t* pix, uint32_t n, double* frame, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_scatter_pixels, dim3((n + 255u) / 256u), dim3(256), 0, s, src, pix, n, frame);
    return hipGetLastError();
}
hipError_t launch_resolve_u8(const double* accum, uint32_t n, int count, uint8_t* out, hipStream_t s) {
    const uint32_t blocks = (n + 255u) / 256u;
    hipLaunchKernelGGL(k_resolve_u8, dim3(blocks), dim3(256), 0, s, accum, n, (double)count, out);
    return hipGetLastError();
}

// =====================================================================
// Adaptive sampling (include/rt.h, "adaptive sampling"): per-pixel second
// moments and sample counts, the stop rule, the stable compaction of the
// still-active pixel list, the list's range check and the per-count resolve
// =====================================================================
// k_accumulate's loop for listed pixel q (j = rp.pixlist[q], never compact), which also adds each
// colour's square to accum2 (the product rounded, then the add, in sample order) and S to count[j];
// accum2 and count may each be null
__global__ __launch_bounds__(256) void k_accumulate_moments(const RenderParams rp, uint32_t S, double* __restrict__ accum,
                                                            double* __restrict__ accum2, uint32_t* __restrict__ count) {
#pragma clang fp contract(off)
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= rp.npix) return;
    const size_t j = rp.pixlist[q];
    double a0 = accum[3u * j], a1 = accum[3u * j + 1], a2 = accum[3u * j + 2];
    double b0 = 0.0, b1 = 0.0, b2 = 0.0;
    if (accum2) { b0 = accum2[3u * j]; b1 = accum2[3u * j + 1]; b2 = accum2[3u * j + 2]; }
    for (uint32_t s = 0; s < S; ++s) {
        const double* r = rp.sb + 3u * ((size_t)s * rp.npix + q);
        const double x0 = r[0], x1 = r[1], x2 = r[2];
        a0 = a0 + x0; a1 = a1 + x1; a2 = a2 + x2;
        const double p0 = x0 * x0, p1 = x1 * x1, p2 = x2 * x2;
        b0 = b0 + p0; b1 = b1 + p1; b2 = b2 + p2;
    }
    accum[3u * j] = a0; accum[3u * j + 1] = a1; accum[3u * j + 2] = a2;
    if (accum2) { accum2[3u * j] = b0; accum2[3u * j + 1] = b1; accum2[3u * j + 2] = b2; }
    if (count) count[j] = count[j] + S;
}

// The stop rule of include/rt.h, in its operation order: the squared standard error of the pixel mean,
// summed over the channels, against (tol * max(mean of the channel sum, floor))^2.  The clamp of a
// variance rounded below zero is written d < 0 ? 0 : d, so a NaN moment stays a NaN, and a NaN compares
// false (not converged); so does n < 2 (0 / 0).
__device__ __forceinline__ bool px_converged(const double* __restrict__ accum, const double* __restrict__ accum2,
                                             const uint32_t cnt, const size_t j, const double tol, const double flr) {
#pragma clang fp contract(off)
    const double n = (double)cnt;
    const double nn = n * (n - 1.0);
    const double s0 = accum[3u * j], s1 = accum[3u * j + 1], s2 = accum[3u * j + 2];
    const double d0 = accum2[3u * j] - (s0 * s0) / n;
    const double d1 = accum2[3u * j + 1] - (s1 * s1) / n;
    const double d2 = accum2[3u * j + 2] - (s2 * s2) / n;
    const double v0 = (d0 < 0.0 ? 0.0 : d0) / nn;
    const double v1 = (d1 < 0.0 ? 0.0 : d1) / nn;
    const double v2 = (d2 < 0.0 ? 0.0 : d2) / nn;
    const double e2 = (v0 + v1) + v2;
    const double m = ((s0 + s1) + s2) / n;
    const double b = m > flr ? m : flr;
    const double r = tol * b;
    return e2 <= r * r;
}

// The selection: pix_out = the entries of pix_in that are not converged, in pix_in's order (a stable
// compaction, so the 16x16-tile order of the list survives).  Three launches — per-block counts, an
// exclusive scan of them by one block, the scatter — and no block ever waits on another.  A block
// covers kSelBlock consecutive entries, wave w of it entries [256 w, 256 w + 256) in four rounds of 64,
// so list order is (block, wave, round, lane).
constexpr uint32_t kSelBlock = 1024u;
struct SelArgs {
    const uint32_t* pix_in;        // null: entry i is pixel i
    uint32_t n;
    const double* accum;
    const double* accum2;
    const uint32_t* count;
    double tol, flr;
    uint32_t max_spp;
};
// entry i's verdict: bit 0 = kept (not converged), bit 1 = kept with its count at max_spp (capped)
__device__ __forceinline__ uint32_t sel_entry(const SelArgs& a, const uint32_t i, uint32_t& j) {
    j = 0u;
    if (i >= a.n) return 0u;
    j = a.pix_in ? a.pix_in[i] : i;
    const uint32_t cnt = a.count[j];
    if (px_converged(a.accum, a.accum2, cnt, j, a.tol, a.flr)) return 0u;
    return cnt >= a.max_spp ? 3u : 1u;
}
__global__ __launch_bounds__(256) void k_select_count(const SelArgs a, uint32_t* __restrict__ blk_keep,
                                                      uint32_t* __restrict__ blk_cap) {
    __shared__ uint32_t s_keep[4], s_cap[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t base = blockIdx.x * kSelBlock + wave * 256u + lane;
    uint32_t keep = 0u, cap = 0u;                       // wave-uniform
    for (uint32_t r = 0; r < 4u; ++r) {
        uint32_t j;
        const uint32_t v = sel_entry(a, base + r * 64u, j);
        keep += (uint32_t)__popcll(__ballot(v & 1u));
        cap += (uint32_t)__popcll(__ballot(v & 2u));
    }
    if (lane == 0u) { s_keep[wave] = keep; s_cap[wave] = cap; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        blk_keep[blockIdx.x] = (s_keep[0] + s_keep[1]) + (s_keep[2] + s_keep[3]);
        blk_cap[blockIdx.x] = (s_cap[0] + s_cap[1]) + (s_cap[2] + s_cap[3]);
    }
}
// one block: blk_off[b] = the kept entries of the blocks before b; totals = {kept, capped} of the list
__global__ __launch_bounds__(256) void k_select_scan(const uint32_t* __restrict__ blk_keep, const uint32_t* __restrict__ blk_cap,
                                                     const uint32_t nb, uint32_t* __restrict__ blk_off,
                                                     unsigned long long* __restrict__ totals) {
    __shared__ uint32_t s_wave[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t running = 0u;                              // kept entries before this pass's 256 blocks
    unsigned long long caps = 0ull;
    for (uint32_t b0 = 0; b0 < nb; b0 += 256u) {
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t v = b < nb ? blk_keep[b] : 0u;
        if (b < nb) caps += blk_cap[b];
        uint32_t incl = v;                              // inclusive scan within the wave
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off, 64);
            if (lane >= (uint32_t)off) incl += t;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = 0u;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
        const uint32_t pass = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        if (b < nb) blk_off[b] = running + before + (incl - v);
        running += pass;
        __syncthreads();                                // s_wave is rewritten by the next pass
    }
    for (int off = 32; off > 0; off >>= 1) caps += __shfl_xor(caps, off, 64);
    __shared__ unsigned long long s_caps[4];
    if (lane == 0u) s_caps[wave] = caps;
    __syncthreads();
    if (threadIdx.x == 0u) {
        totals[0] = running;
        totals[1] = (s_caps[0] + s_caps[1]) + (s_caps[2] + s_caps[3]);
    }
}
__global__ __launch_bounds__(256) void k_select_scatter(const SelArgs a, const uint32_t* __restrict__ blk_off,
                                                        uint32_t* __restrict__ pix_out) {
    __shared__ uint32_t s_keep[4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t base = blockIdx.x * kSelBlock + wave * 256u + lane;
    uint32_t jj[4];
    unsigned long long mk[4];
    uint32_t keep = 0u;
    for (uint32_t r = 0; r < 4u; ++r) {
        const uint32_t v = sel_entry(a, base + r * 64u, jj[r]);
        mk[r] = __ballot(v & 1u);
        keep += (uint32_t)__popcll(mk[r]);
    }
    if (lane == 0u) s_keep[wave] = keep;
    __syncthreads();
    uint32_t pos = blk_off[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) pos += s_keep[w];
    for (uint32_t r = 0; r < 4u; ++r) {                  // pos + the wave's kept count <= the list's kept total <= n
        if ((mk[r] >> lane) & 1ull) pix_out[pos + lanes_below(mk[r])] = jj[r];
        pos += (uint32_t)__popcll(mk[r]);
    }
}
hipError_t launch_accumulate_moments(const RenderParams& rp, uint32_t S, double* accum, double* accum2, uint32_t* count,
                                     hipStream_t s) {
    const uint32_t blocks = (rp.npix + 255u) / 256u;
    hipLaunchKernelGGL(k_accumulate_moments, dim3(blocks), dim3(256), 0, s, rp, S, accum, accum2, count);
    return hipGetLastError();
}
uint32_t select_blocks(const uint32_t n) { return (n + kSelBlock - 1u) / kSelBlock; }
// scratch: 3 * select_blocks(n) words; totals: two 64-bit words {kept, capped}
hipError_t launch_select(const uint32_t* pix_in, uint32_t n, const double* accum, const double* accum2, const uint32_t* count,
                         double tol, double flr, uint32_t max_spp, uint32_t* scratch, unsigned long long* totals,
                         uint32_t* pix_out, hipStream_t s) {
    const uint32_t nb = select_blocks(n);
    if (nb == 0u) return hipMemsetAsync(totals, 0, 2 * sizeof(unsigned long long), s);
    const SelArgs a{pix_in, n, accum, accum2, count, tol, flr, max_spp};
    uint32_t *blk_keep = scratch, *blk_cap = scratch + nb, *blk_off = scratch + 2 * (size_t)nb;
    hipLaunchKernelGGL(k_select_count, dim3(nb), dim3(256), 0, s, a, blk_keep, blk_cap);
    HIP_RETURN_IF(hipGetLastError());
    hipLaunchKernelGGL(k_select_scan, dim3(1), dim3(256), 0, s, blk_keep, blk_cap, nb, blk_off, totals);
    HIP_RETURN_IF(hipGetLastError());
    hipLaunchKernelGGL(k_select_scatter, dim3(nb), dim3(256), 0, s, a, blk_off, pix_out);
    return hipGetLastError();
}

// a caller's pixel list, read only: its largest entry into *out_max (zeroed by the host before the launch)
__global__ __launch_bounds__(256) void k_check_pixels(const uint32_t* __restrict__ pix, const uint32_t n,
                                                      uint32_t* __restrict__ out_max) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t v = i < n ? pix[i] : 0u;
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t t = __shfl_xor(v, off, 64);
        v = t > v ? t : v;
    }
    if ((threadIdx.x & 63u) == 0u && v) atomicMax(out_max, v);
}
hipError_t launch_check_pixels(const uint32_t* pix, uint32_t n, uint32_t* out_max, hipStream_t s) {
    HIP_RETURN_IF(hipMemsetAsync(out_max, 0, sizeof(uint32_t), s));
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_check_pixels, dim3((n + 255u) / 256u), dim3(256), 0, s, pix, n, out_max);
    return hipGetLastError();
}

// the resolve with each pixel's own sample count: floor(255.99*min(1, sqrt(sum/count))), 0 for count 0
__global__ __launch_bounds__(256) void k_resolve_u8_counts(const double* __restrict__ accum, const uint32_t* __restrict__ count,
                                                           uint32_t n, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t cnt = count[i / 3u];
    if (cnt == 0u) { out[i] = 0; return; }
    const double c = sqrt(accum[i] / (double)cnt);
    const double m = (1.0 < c) ? 1.0 : c;
    out[i] = (uint8_t)floor(255.99 * m);
}
hipError_t launch_resolve_u8_counts(const double* accum, const uint32_t* count, uint32_t n, uint8_t* out, hipStream_t s) {
    if (n == 0u) return hipSuccess;
    hipLaunchKernelGGL(k_resolve_u8_counts, dim3((n + 255u) / 256u), dim3(256), 0, s, accum, count, n, out);
    return hipGetLastError();
}

// =====================================================================
// Denoiser (include/rt.h, "denoiser"): an edge-avoiding a-trous filter of the demodulated mean, guided
// by the first-hit features and the variance of the mean.  Every expression below is the header's rule
// in its operation order (rtamd.denoise.atrous restates it in NumPy); one lane per pixel, 16x16 blocks.
// =====================================================================
struct alignas(8) DnGuide { double nx, ny, nz, z, h; };          // 40 B
struct alignas(16) DnSignal { double u0, u1, u2, v; };           // 32 B
static_assert(sizeof(DnGuide) == kDenoiseGuideBytes && sizeof(DnSignal) == kDenoiseSignalBytes, "denoiser records");
struct DnArgs {
    uint32_t nx, ny;
    const double* accum;
    const double* accum2;          // nullable
    const uint32_t* count;         // nullable: every pixel has sample_count samples
    double sample_count, feat_count;
    const double* feat;
    double sigma_z, sigma_l, albedo_floor;
    uint32_t normal_squarings;
};
// the B3-spline kernel [1/16, 1/4, 3/8, 1/4, 1/16] at offset d = -2..2 (exact binary fractions)
__device__ __forceinline__ double dn_kernel(const int d) { return d == 0 ? 0.375 : (d == 1 || d == -1) ? 0.25 : 0.0625; }
__device__ __forceinline__ bool dn_finite(const double x) { return fabs(x) < __builtin_inf(); }   // false for NaN
__device__ __forceinline__ bool dn_valid(const DnSignal& s) {
    return dn_finite(s.u0) && dn_finite(s.u1) && dn_finite(s.u2) && dn_finite(s.v);
}
__device__ __forceinline__ double dn_den(const DnArgs& a, const size_t j, const int k) {
    const double al = a.feat[RT_FEATURE_DOUBLES * j + k] / a.feat_count;
    return al > a.albedo_floor ? al : a.albedo_floor;
}
__global__ __launch_bounds__(256) void k_denoise_prepare(const DnArgs a, DnGuide* __restrict__ guide,
                                                         DnSignal* __restrict__ sig) {
#pragma clang fp contract(off)
    const uint32_t x = blockIdx.x * 16u + (threadIdx.x & 15u), y = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (x >= a.nx || y >= a.ny) return;
    const size_t j = (size_t)y * a.nx + x;
    const double n = a.count ? (double)a.count[j] : a.sample_count;
    const double m = a.feat_count;
    const double* f = a.feat + RT_FEATURE_DOUBLES * j;
    guide[j] = DnGuide{f[3] / m, f[4] / m, f[5] / m, f[6] / m, f[7] / m};
    const double nn = n * (n - 1.0);
    double u[3], v = 0.0;
    double e[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k) {
        const double S = a.accum[3u * j + k];
        const double c = n == 0.0 ? 0.0 : S / n;
        const double den = dn_den(a, j, k);
        u[k] = c / den;
        if (a.accum2 && n >= 2.0) {
            const double d = a.accum2[3u * j + k] - (S * S) / n;
            e[k] = ((d < 0.0 ? 0.0 : d) / nn) / (den * den);
        }
    }
    if (a.accum2 && n >= 2.0) v = (e[0] + e[1]) + e[2];
    sig[j] = DnSignal{u[0], u[1], u[2], v};
}
// One iteration at step `step`: taps (dx, dy) in {-2..2}^2 at (x + dx*step, y + dy*step), dy the outer loop.
// Taps come straight from global memory: a pixel's 25 taps are 25 distinct 32-B + 40-B records whatever
// the step, neighbouring lanes read neighbouring records, and the frame's records (72 B per pixel) stay in
// the L2 / Infinity Cache between the taps' re-reads (DESIGN 4.6 has the measured time per iteration).
// LAST: write u * den to out_mean instead of the signal record.
template <bool LAST>
__global__ __launch_bounds__(256) void k_denoise_atrous(const DnArgs a, const uint32_t step,
                                                        const DnGuide* __restrict__ guide, const DnSignal* __restrict__ in,
                                                        DnSignal* __restrict__ out, double* __restrict__ out_mean) {
#pragma clang fp contract(off)
    const uint32_t x = blockIdx.x * 16u + (threadIdx.x & 15u), y = blockIdx.y * 16u + (threadIdx.x >> 4);
    if (x >= a.nx || y >= a.ny) return;
    const size_t j = (size_t)y * a.nx + x;
    const DnSignal sp = in[j];
    DnSignal r = sp;                                       // a pixel that is not valid passes through
    if (dn_valid(sp)) {
        const DnGuide gp = guide[j];
        const double lp = (sp.u0 + sp.u1) + sp.u2;
        const double lden = a.sigma_l * sqrt(sp.v) + 1e-10;
        double W = 0.0, U0 = 0.0, U1 = 0.0, U2 = 0.0, V = 0.0;
        for (int dy = -2; dy <= 2; ++dy) {
            const int64_t yy = (int64_t)y + (int64_t)dy * (int64_t)step;
            if (yy < 0 || yy >= (int64_t)a.ny) continue;
            for (int dx = -2; dx <= 2; ++dx) {
                const int64_t xx = (int64_t)x + (int64_t)dx * (int64_t)step;
                if (xx < 0 || xx >= (int64_t)a.nx) continue;
                const double hk = dn_kernel(dy) * dn_kernel(dx);
                double w;
                DnSignal sq;
                if (dx == 0 && dy == 0) {
                    w = hk;
                    sq = sp;
                } else {
                    const size_t jq = (size_t)yy * a.nx + (size_t)xx;
                    sq = in[jq];
                    if (!dn_valid(sq)) continue;
                    const DnGuide gq = guide[jq];
                    double wn = 1.0;
                    if (!(gp.h == 0.0 && gq.h == 0.0)) {
                        const double g = (gp.nx * gq.nx + gp.ny * gq.ny) + gp.nz * gq.nz;
                        wn = g > 0.0 ? g : 0.0;
                        for (uint32_t t = 0; t < a.normal_squarings; ++t) wn = wn * wn;
                    }
                    const double zm = gp.z > gq.z ? gp.z : gq.z;
                    const double wz = exp(-(fabs(gp.z - gq.z) / (a.sigma_z * zm + 1e-300)));
                    double wl = 1.0;
                    if (a.accum2) {
                        const double lq = (sq.u0 + sq.u1) + sq.u2;
                        wl = exp(-(fabs(lp - lq) / lden));
                    }
                    w = ((hk * wn) * wz) * wl;
                }
                W = W + w;
                U0 = U0 + w * sq.u0; U1 = U1 + w * sq.u1; U2 = U2 + w * sq.u2;
                V = V + (w * w) * sq.v;
            }
        }
        r = DnSignal{U0 / W, U1 / W, U2 / W, V / (W * W)};
    }
    if (LAST) {
        out_mean[3u * j] = r.u0 * dn_den(a, j, 0);
        out_mean[3u * j + 1] = r.u1 * dn_den(a, j, 1);
        out_mean[3u * j + 2] = r.u2 * dn_den(a, j, 2);
    } else {
        out[j] = r;
    }
}
hipError_t launch_denoise(int nx, int ny, const struct rt_denoise& p, const double* accum, const double* accum2,
                          const uint32_t* count, uint32_t sample_count, const double* feat, uint32_t feat_count,
                          void* guide, void* sig_a, void* sig_b, double* out_mean, hipStream_t s) {
    const DnArgs a{(uint32_t)nx, (uint32_t)ny, accum, accum2, count, (double)sample_count, (double)feat_count, feat,
                   p.sigma_z, p.sigma_l, p.albedo_floor, p.normal_squarings};
    const dim3 grid(((uint32_t)nx + 15u) / 16u, ((uint32_t)ny + 15u) / 16u), block(256);
    DnGuide* g = static_cast<DnGuide*>(guide);
    DnSignal* cur = static_cast<DnSignal*>(sig_a);
    DnSignal* nxt = static_cast<DnSignal*>(sig_b);
    hipLaunchKernelGGL(k_denoise_prepare, grid, block, 0, s, a, g, cur);
    HIP_RETURN_IF(hipGetLastError());
    for (uint32_t i = 0; i < p.iterations; ++i) {
        const uint32_t step = 1u << i;
        if (i + 1u == p.iterations)
            hipLaunchKernelGGL((k_denoise_atrous<true>), grid, block, 0, s, a, step, g, cur, nxt, out_mean);
        else
            hipLaunchKernelGGL((k_denoise_atrous<false>), grid, block, 0, s, a, step, g, cur, nxt, out_mean);
        HIP_RETURN_IF(hipGetLastError());
        DnSignal* t = cur; cur = nxt; nxt = t;
    }
    return hipSuccess;
}

}  // namespace rtamd
