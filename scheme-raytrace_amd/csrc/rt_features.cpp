// rt_features.cpp — first-hit feature buffers (include/rt.h): albedo, normal, depth and coverage summed
// over the camera samples a render of the same passes takes (k_features, rt_kernels.hip).
#include <algorithm>
#include <cstdlib>

#include "rt_host.h"
#include "rt_launch.h"

using namespace rtamd;

namespace {
int check_features(int nx, int ny, int spp_begin, int spp_count, const double* feat) {
    if (int rc = check_frame(nx, ny)) return rc;
    if (!feat) return fail("null feature buffer");
    if (spp_begin < 0 || spp_count < 0) return fail("spp_begin/spp_count must be >= 0");
    if ((uint64_t)spp_begin + (uint64_t)spp_count > 0xFFFFFFFFull) return fail("sample index out of range");
    return 0;
}
// passes spp_begin .. spp_begin+spp_count-1 of the n pixels of `pix` (device; checked or the scene's own
// list) into feat, on st; synchronises st and reports device faults as a render does
int features_impl(Scene* s, int nx, int ny, const uint32_t* pix, uint32_t n, int spp_begin, int spp_count, uint64_t seed,
                  double* feat, hipStream_t st) {
    {
        uint32_t stale = 0;
        HIPCHK(take_fault(&stale));                  // a fault word left by another context's failed launch
        const char* e = std::getenv("RTAMD_REJECT_CAP");            // the render's test hooks (render_impl)
        const char* rc = std::getenv("RTAMD_CURVE_RAY_CAP");
        HIPCHK(set_test_caps(e ? std::max(0, std::atoi(e)) : 4096, rc ? (uint32_t)std::strtoul(rc, nullptr, 10) : 0u));
    }
    RenderParams rp{};
    rp.nx = (uint32_t)nx; rp.ny = (uint32_t)ny; rp.npix = n;
    rp.inx = 1.0 / (double)nx; rp.iny = 1.0 / (double)ny;
    rp.spp0 = (uint32_t)spp_begin; rp.k0 = (uint32_t)seed; rp.k1 = (uint32_t)(seed >> 32);
    rp.pixlist = pix;
    HIPCHK(launch_features(s->dev, rp, (uint32_t)spp_count, feat, st));
    HIPCHK(hipStreamSynchronize(st));
    uint32_t f = 0;
    HIPCHK(take_fault(&f));
    if (f) return fail(fault_text(f));
    return 0;
}
}  // namespace

extern "C" {

int rt_render_features_device(int scene, int nx, int ny, const uint32_t* pix_device, int64_t n, int spp_begin, int spp_count,
                              uint64_t seed, double* feat_device, void* stream) {
    if (int rc = check_features(nx, ny, spp_begin, spp_count, feat_device)) return rc;
    if (pix_device && (n < 0 || n > (int64_t)nx * ny))
        return fail("pixel list length " + std::to_string(n) + " outside 0 .. nx*ny");
    LOCK_SCENE(s, scene);
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    CTX_OF(c, s);
    if ((pix_device && n == 0) || spp_count == 0) return 0;
    CTX_STREAM(c, st, stream);
    PixSet px{pix_device, (uint32_t)n, false, nullptr, nullptr};
    if (pix_device) {
        // the list's range, read only, before the kernel that writes through it
        HIPCHK(c->sel_words.ensure(3 * sizeof(unsigned long long)));
        uint32_t* d_max = reinterpret_cast<uint32_t*>(c->sel_words.as<unsigned long long>() + 2);
        HIPCHK(launch_check_pixels(pix_device, (uint32_t)n, d_max, st));
        uint32_t h_max = 0;
        HIPCHK(hipMemcpyAsync(&h_max, d_max, sizeof h_max, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (h_max >= (uint32_t)(nx * ny))
            return fail("pixel list entry " + std::to_string(h_max) + " is outside the frame (nx*ny = " +
                        std::to_string(nx * ny) + ")");
    } else if (int rc = pixset_of(s, nx, ny, full_frame(ny), false, &px)) {
        return rc;
    }
    return features_impl(s, nx, ny, px.pix, px.n, spp_begin, spp_count, seed, feat_device, st);
}

int rt_render_features(int scene, int nx, int ny, int spp_begin, int spp_count, uint64_t seed, double* feat_host) {
    if (int rc = check_features(nx, ny, spp_begin, spp_count, feat_host)) return rc;
    LOCK_SCENE(s, scene);
    if (!s->committed) return fail("scene not committed (rt_scene_commit)");
    CTX_OF(c, s);
    if (spp_count == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    PixSet px{nullptr, 0, false, nullptr, nullptr};
    if (int rc = pixset_of(s, nx, ny, full_frame(ny), false, &px)) return rc;
    const size_t bytes = (size_t)nx * ny * RT_FEATURE_DOUBLES * sizeof(double);
    DevBuf d_feat;
    HIPCHK(d_feat.ensure(bytes));
    HIPCHK(hipMemcpyAsync(d_feat.p, feat_host, bytes, hipMemcpyHostToDevice, c->stream));
    if (int rc = features_impl(s, nx, ny, px.pix, px.n, spp_begin, spp_count, seed, d_feat.as<double>(), c->stream)) return rc;
    HIPCHK(hipMemcpyAsync(feat_host, d_feat.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
