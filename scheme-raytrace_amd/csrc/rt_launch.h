// rt_launch.h — the launch interface of librtamd's device translation units: every function the host
// translation units call into rt_kernels.hip (path tracing) and rt_frame.hip (frame buffers), declared
// once.  The device files that define these include it, so a definition that drifts from its
// declaration is a compile or link error (the library links with -z defs), not a load-time one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_device.h"

namespace rtamd {

// ------------------------------------------------------- rt_kernels.hip
hipError_t launch_raygen(const DevScene& sc, const RenderParams& rp, const PathState& st, hipStream_t s);
// in: the survivor queue view of the previous depth (contiguous for raygen's output); counts: this
// iteration's [material][shard] hit counters; claim: the persistent curve kernel's next-ray counter
// (null: per-ray k_extend only); fuse: non-null runs every depth >= 1 in this launch (curve-kernel scenes);
// inst: null, or where the launch leaves the ExtendInst it took
hipError_t launch_extend(const DevScene& sc, const DevScene* scd, const RenderParams& rp, const PathState& st,
                         const QView& in, uint32_t n, const HitBuf& hit, uint32_t shard_cap, uint32_t* counts,
                         bool depth0, unsigned int* claim, const CurveFuse* fuse, hipStream_t s, int* inst = nullptr);
// The extend launch_extend takes: k_extend<F>, k_extend_curves<0>, or k_extend_curves<FUSE> with the device (1)
// or the exact (2) libm.  launch_extend forms this value and picks its kernel from it alone, so what
// rt_step_rays reports is what was launched.
enum ExtendInst { EXTEND_PER_RAY = 0, EXTEND_CURVES = 1, EXTEND_CURVES_FUSED = 2, EXTEND_CURVES_FUSED_EXACT = 3 };
ExtendInst extend_instance(const DevScene& sc, const RenderParams& rp, bool claim, bool fuse);
// mat: the material whose hit queue (qv, at most n_upper hits) is shaded; out / out_counts: the next
// depth's path state and its per-shard survivor counters; pt: the launch that filled the queues wrote the
// lambertian one as point records (launch_camera / launch_extend_lds with pt)
hipError_t launch_shade(int mat, const DevScene& sc, const DevScene* scd, const RenderParams& rp, const PathState& in,
                        const HitBuf& hit, bool pt, const QView& qv, uint32_t n_upper, const PathState& out,
                        uint32_t* out_counts, uint32_t shard_cap, uint32_t depth, hipStream_t s);
// the tail kernel: finishes the n live paths of `in`; seg_count: its segment counter, followed by the
// next-path claim; tree0_budget: LDS bytes the time-0 tree may take (0: not staged)
hipError_t launch_finish(const DevScene& sc, const DevScene* scd, const RenderParams& rp, const PathState& st,
                         const QView& in, uint32_t n, unsigned long long* seg_count, size_t tree0_budget,
                         uint32_t depth, hipStream_t s);
// The template arguments of the k_shade<mat, TL, LS, LL, EX, PT> / k_finish<F, TL, LS, SOLO, EX> instance a
// launch takes.  launch_shade and launch_finish form these records and pick their kernel from them alone, so
// what rt_step_rays reports is what was launched.
struct ShadeInst { int tl, ls; bool ll, ex, pt; };
struct FinishInst { int f, tl, ls; bool solo, ex; };
ShadeInst shade_instance(int mat, const DevScene& sc, const RenderParams& rp, bool pt);
FinishInst finish_instance(const DevScene& sc, const RenderParams& rp, size_t tree0_budget);
// bytes of LDS k_extend_lds needs for the scene's time-0 tree (0 = cannot run)
size_t extend_lds_bytes(const DevScene& sc);
// max_blocks: every block the kernel can keep on the device at once with `lds` bytes of dynamic LDS
hipError_t extend_lds_prepare(const DevScene& sc, size_t lds, uint32_t* max_blocks);
// LDS bytes k_camera needs (0 = cannot run)
size_t camera_lds_bytes(const DevScene& sc);
hipError_t camera_prepare(const DevScene& sc, size_t lds, uint32_t* max_blocks);
// raygen + the depth-0 closest hit in one kernel; lds / max_blocks: camera_lds_bytes / camera_prepare;
// err: the word a block sets when its LDS allocation was too small; pt (scenes point_hits_scene accepts
// only): lambertian hits go to hit.hp as point records and store no ray
hipError_t launch_camera(const DevScene& sc, const RenderParams& rp, const PathState& st, uint32_t n,
                         const HitBuf& hit, bool pt, uint32_t shard_cap, uint32_t* counts, size_t lds, uint32_t max_blocks,
                         unsigned long long* err, hipStream_t s);
// a depth >= 1 extend with the time-0 tree in LDS; max_blocks: extend_lds_prepare's; err as above
hipError_t launch_extend_lds(const DevScene& sc, const RenderParams& rp, const PathState& st, const QView& in,
                             uint32_t n, const HitBuf& hit, bool pt, uint32_t shard_cap, uint32_t* counts,
                             uint32_t max_blocks, unsigned long long* err, hipStream_t s);
// whether the scene's LDS kernels and lambertian shade have point-record instances: a SOLO world (the caller
// checks that no leaf has an instance chain) without the light mixture or image textures
bool point_hits_scene(const DevScene& sc);
bool curve_persistent();                    // the host's check before a fused launch
// rt_curve_depth_probe: bez_maxd on ray-space control points (12 doubles per curve) and 8 eps
hipError_t launch_curve_depth(const double* cps, const double* eps8, uint32_t n, int32_t* out, hipStream_t s);
// rt_f64_probe: rt_f64.h's helper `kind` (RT_F64_*) over n doubles
hipError_t launch_f64_probe(int kind, const double* in, uint32_t n, double* out, hipStream_t s);
// rt_hit_rays: n rays of 7 doubles (origin, direction, time); the closest hit's t and material
hipError_t launch_hit_rays(const DevScene& sc, const double* rays, uint32_t n, double* out_t, int32_t* out_mat,
                           hipStream_t s);
// rt_hit_rays_stream: the same query with ray k on the path stream (k0, k1; pixel k, sample 0) from counter 0;
// out_draws: the random numbers each query took
hipError_t launch_hit_rays_stream(const DevScene& sc, const double* rays, uint32_t n, uint32_t k0, uint32_t k1,
                                  double* out_t, int32_t* out_mat, int32_t* out_draws, hipStream_t s);
// rt_hit_rays_walk's LDS walks: the same rays through k_extend_lds's query (time0: every ray at time +0.0)
// or k_camera's, in the instance those kernels' launchers pick for the scene; lds: the scene's
// extend_lds_bytes (time0) / camera_lds_bytes, not 0
hipError_t launch_hit_rays_lds(const DevScene& sc, bool time0, size_t lds, const double* rays, uint32_t n,
                               double* out_t, int32_t* out_mat, hipStream_t s);
// rt_render_features: passes rp.spp0 .. rp.spp0 + S - 1 of the rp.npix pixels of rp.pixlist, their first-hit
// features added to feat (RT_FEATURE_DOUBLES running sums per image pixel); only nx, ny, inx, iny, npix,
// spp0, k0, k1 and pixlist of rp are read
hipError_t launch_features(const DevScene& sc, const RenderParams& rp, uint32_t S, double* feat, hipStream_t s);
// rt_light_probe: n points (3 doubles each) through the mixture's light sampler and density, point k on the
// path stream (k0, k1; pixel k, sample 0) from counter 0; dirs / out_pdf_dirs null together; exact_libm: the
// sphere sampler's sin / cos as the scene's renders take them.  A scene without light sampling is an error.
hipError_t launch_light_probe(const DevScene& sc, const DevScene* scd, bool exact_libm, const double* points,
                              const double* dirs, uint32_t n, uint32_t k0, uint32_t k1, double* out_dir, double* out_pdf,
                              double* out_pdf_dirs, int32_t* out_draws, hipStream_t s);
// the device fault word: read and clear
hipError_t take_fault(uint32_t* out);
// the batched-curve counters: read and clear
hipError_t take_curve_stats(unsigned long long out[2]);
// test hooks: the samplers' attempt cap and the persistent curve kernel's per-ray iteration cap (0 = the
// scene's bound)
hipError_t set_test_caps(int reject_cap, uint32_t curve_ray_cap);

// --------------------------------------------------------- rt_frame.hip
// S: the chunk's samples per pixel, added to accum in sample order
hipError_t launch_accumulate(const RenderParams& rp, uint32_t S, double* accum, hipStream_t s);
// launch_accumulate for a listed render, which also adds the samples' squares to accum2 and S to
// count (each nullable)
hipError_t launch_accumulate_moments(const RenderParams& rp, uint32_t S, double* accum, double* accum2,
                                     uint32_t* count, hipStream_t s);
// n: the accumulator's doubles (3 per pixel); count: the samples per pixel
hipError_t launch_resolve_u8(const double* accum, uint32_t n, int count, uint8_t* out, hipStream_t s);
// the resolve with each pixel's own sample count
hipError_t launch_resolve_u8_counts(const double* accum, const uint32_t* count, uint32_t n, uint8_t* out,
                                    hipStream_t s);
// the frame-end gather's placement: shard pixel q's three sums to image pixel pix[q]
hipError_t launch_scatter_pixels(const double* src, const uint32_t* pix, uint32_t n, double* frame, hipStream_t s);
// blocks the selection of an n-entry list runs (its scratch is 3 words per block)
uint32_t select_blocks(uint32_t n);
// pix_in: null = entry i is pixel i; scratch: 3 * select_blocks(n) words; totals: two 64-bit words
// {kept, capped}; pix_out: the kept entries in pix_in's order
hipError_t launch_select(const uint32_t* pix_in, uint32_t n, const double* accum, const double* accum2,
                         const uint32_t* count, double tol, double flr, uint32_t max_spp, uint32_t* scratch,
                         unsigned long long* totals, uint32_t* pix_out, hipStream_t s);
// a caller's pixel list, read only: its largest entry into *out_max
hipError_t launch_check_pixels(const uint32_t* pix, uint32_t n, uint32_t* out_max, hipStream_t s);
// rt_denoise: the variance-guided a-trous filter of include/rt.h.  accum2 / count nullable (count null: every
// pixel has sample_count samples); guide: npx 40-byte records, sig_a / sig_b: npx 32-byte records each
// (the context's scratch); out_mean: npx * 3 doubles
constexpr size_t kDenoiseGuideBytes = 40, kDenoiseSignalBytes = 32;
hipError_t launch_denoise(int nx, int ny, const struct rt_denoise& p, const double* accum, const double* accum2,
                          const uint32_t* count, uint32_t sample_count, const double* feat, uint32_t feat_count,
                          void* guide, void* sig_a, void* sig_b, double* out_mean, hipStream_t s);

}  // namespace rtamd
