// rt_denoise.cpp — the denoiser's entry points (include/rt.h): parameter checks, the context's scratch and
// the launches of rt_frame.hip's prepare / a-trous kernels.
#include <cmath>

#include "rt_host.h"
#include "rt_launch.h"

using namespace rtamd;

namespace {
int check_positive(double v, const char* name) {
    if (!std::isfinite(v) || !(v > 0.0)) return fail(std::string(name) + " must be finite and > 0");
    return 0;
}
int check_denoise(int nx, int ny, const struct rt_denoise* p, const double* accum, const double* accum2, const double* feat,
                  uint32_t feat_count, const double* out_mean) {
    if (int rc = check_frame(nx, ny)) return rc;
    if (!p) return fail("null rt_denoise parameters");
    if (!accum || !feat || !out_mean) return fail("null buffer");
    if (p->iterations < 1 || p->iterations > 12) return fail("iterations must be in 1 .. 12");
    if (p->normal_squarings > 16) return fail("normal_squarings must be <= 16");
    if (int rc = check_positive(p->sigma_z, "sigma_z")) return rc;
    if (int rc = check_positive(p->sigma_l, "sigma_l")) return rc;
    if (int rc = check_positive(p->albedo_floor, "albedo_floor")) return rc;
    if (feat_count == 0) return fail("feat_count must be >= 1");
    if (out_mean == accum || out_mean == accum2 || out_mean == feat) return fail("out_mean must not alias an input");
    return 0;
}
int denoise_impl(Context* c, int nx, int ny, const struct rt_denoise& p, const double* accum, const double* accum2,
                 const uint32_t* count, uint32_t sample_count, const double* feat, uint32_t feat_count, double* out_mean,
                 hipStream_t st) {
    const size_t npx = (size_t)nx * ny;
    for (DevBuf& b : c->dn_signal) HIPCHK(b.ensure(npx * kDenoiseSignalBytes));
    HIPCHK(c->dn_guide.ensure(npx * kDenoiseGuideBytes));
    HIPCHK(launch_denoise(nx, ny, p, accum, accum2, count, sample_count, feat, feat_count, c->dn_guide.p, c->dn_signal[0].p,
                          c->dn_signal[1].p, out_mean, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
}  // namespace

extern "C" {

int rt_denoise_device(int ctx, int nx, int ny, const struct rt_denoise* p, const double* accum, const double* accum2,
                      const uint32_t* count, uint32_t sample_count, const double* feat, uint32_t feat_count, double* out_mean,
                      void* stream) {
    if (int rc = check_denoise(nx, ny, p, accum, accum2, feat, feat_count, out_mean)) return rc;
    LOCK_CTX(c, ctx);
    CTX_STREAM(c, st, stream);
    return denoise_impl(c, nx, ny, *p, accum, accum2, count, sample_count, feat, feat_count, out_mean, st);
}

int rt_denoise(int ctx, int nx, int ny, const struct rt_denoise* p, const double* accum, const double* accum2, const uint32_t* count,
               uint32_t sample_count, const double* feat, uint32_t feat_count, double* out_mean) {
    if (int rc = check_denoise(nx, ny, p, accum, accum2, feat, feat_count, out_mean)) return rc;
    LOCK_CTX(c, ctx);
    HIPCHK(hipSetDevice(c->device));
    const size_t npx = (size_t)nx * ny;
    DevBuf d_accum, d_accum2, d_count, d_feat, d_out;
    HIPCHK(d_accum.ensure(npx * 3 * sizeof(double)));
    HIPCHK(d_feat.ensure(npx * RT_FEATURE_DOUBLES * sizeof(double)));
    HIPCHK(d_out.ensure(npx * 3 * sizeof(double)));
    HIPCHK(hipMemcpyAsync(d_accum.p, accum, npx * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(d_feat.p, feat, npx * RT_FEATURE_DOUBLES * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (accum2) {
        HIPCHK(d_accum2.ensure(npx * 3 * sizeof(double)));
        HIPCHK(hipMemcpyAsync(d_accum2.p, accum2, npx * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    if (count) {
        HIPCHK(d_count.ensure(npx * sizeof(uint32_t)));
        HIPCHK(hipMemcpyAsync(d_count.p, count, npx * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    if (int rc = denoise_impl(c, nx, ny, *p, d_accum.as<double>(), accum2 ? d_accum2.as<double>() : nullptr,
                              count ? d_count.as<uint32_t>() : nullptr, sample_count, d_feat.as<double>(), feat_count,
                              d_out.as<double>(), c->stream))
        return rc;
    HIPCHK(hipMemcpyAsync(out_mean, d_out.p, npx * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
