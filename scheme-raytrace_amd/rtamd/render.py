"""The pixel driver: trace-all / trace-line / save-as-ppm (main.scm:439-491).

``Renderer`` owns the reference's globals *size-x*, *size-y*, *raw-data*
(running f64 sum, nx*ny*3, y-up rows) and *image* (u8).  ``trace_all(scene,
sample_count)`` is one pass exactly like the reference's: it adds sample
number ``sample_count`` (1-based) to every pixel and re-resolves the image
with sqrt(sum/sample_count).  ``trace_line(scene, y, sample_count)`` is the
reference's per-row pass (main.scm:452-469) and ``animate(scene)`` its GLUT
display step (main.scm:533-544: one row per call, then the next pass).
``render(scene, spp)`` runs many passes in one GPU call (same result as spp
successive trace_all calls).  ``render_adaptive(scene, tol, ...)`` is an
extension: passes per pixel until its estimated error is below ``tol``.
``render_features(scene, spp)`` and ``denoise(**params)`` are extensions too:
the first-hit feature buffers of the camera samples, and the variance-guided
a-trous filter of the running sums they guide (include/rt.h, "denoiser").
"""
import numpy as np

from . import gpu
from .denoise import DEFAULTS as DENOISE_DEFAULTS

DEFAULT_SEED = 0x5EED0002


class Renderer:
    def __init__(self, nx, ny, seed=DEFAULT_SEED, ctx=None):
        self.size_x, self.size_y = int(nx), int(ny)
        self.seed = int(seed)
        self.ctx = ctx
        self.raw_data = np.zeros(self.size_x * self.size_y * 3, dtype=np.float64)
        self.image = np.zeros(self.size_x * self.size_y * 3, dtype=np.uint8)
        # render_adaptive only: the running sums of the samples' squares and each pixel's sample count
        self.raw_data2 = np.zeros(self.size_x * self.size_y * 3, dtype=np.float64)
        self.counts = np.zeros(self.size_x * self.size_y, dtype=np.uint32)
        self.adaptive = False         # raw_data2 / counts hold the last render's moments (render_adaptive)
        # render_features: the running sums of the first-hit features (albedo 3, normal 3, t, hits per pixel)
        self.features = np.zeros(self.size_x * self.size_y * 8, dtype=np.float64)
        self.feature_count = 0
        self.denoised = None          # denoise(): the filtered mean radiance, nx*ny*3
        self.sample_count = 0
        self.current_y = 0            # *current-y* (main.scm:431)
        self.anim_sample_count = 1    # *sample-count* (main.scm:531)

    def trace_all(self, scene, sample_count):
        """main.scm:471-491 — one sample per pixel (pass `sample_count`)."""
        if sample_count < 1:
            raise ValueError("sample-count is 1-based")
        gpu.render_host(scene, self.size_x, self.size_y, sample_count - 1, 1, self.seed, self.raw_data, self.ctx)
        self.image = gpu.resolve_u8(self.raw_data, self.size_x, self.size_y, sample_count)
        self.sample_count = sample_count
        return self.image

    def trace_line(self, scene, y, sample_count):
        """main.scm:452-469 — sample number `sample_count` (1-based) of row y only,
        and row y of the image re-resolved; animate (main.scm:533-544) calls it
        row by row, so a full sweep equals trace_all(scene, sample_count)."""
        if sample_count < 1:
            raise ValueError("sample-count is 1-based")
        if not 0 <= y < self.size_y:
            raise ValueError("row outside the image")
        gpu.trace_line(scene, self.size_x, self.size_y, y, sample_count, self.seed, self.raw_data, self.image,
                       self.ctx)
        return self.image

    def animate(self, scene):
        """One display callback of main.scm:533-544 with *rendering?* on: trace
        the current row; after the last row start the next sample pass."""
        if self.current_y < self.size_y:
            self.trace_line(scene, self.current_y, self.anim_sample_count)
            self.current_y += 1
        else:
            self.anim_sample_count += 1
            self.current_y = 0
        return self.image

    def render(self, scene, spp, spp_begin=None):
        """Passes spp_begin+1 .. spp_begin+spp in one call (default: continue)."""
        if spp_begin is None:
            spp_begin = self.sample_count
        gpu.render_host(scene, self.size_x, self.size_y, spp_begin, spp, self.seed, self.raw_data, self.ctx)
        self.adaptive = False         # raw_data2 / counts no longer describe raw_data
        self.sample_count = spp_begin + spp
        self.image = gpu.resolve_u8(self.raw_data, self.size_x, self.size_y, self.sample_count)
        return self.image

    def render_adaptive(self, scene, tol, min_spp=16, max_spp=1024, batch_spp=16, floor=0.05):
        """An adaptive render from pass 0 (no counterpart in the reference, whose *max-sample*,
        main.scm:433, is never used): every pixel gets min_spp passes, then batch_spp more per round while
        the standard error of its mean exceeds tol * max(mean, floor), up to max_spp.  Fills raw_data,
        raw_data2 (the squares' sums), counts and image (each pixel resolved with its own count);
        sample_count becomes max(counts).  Returns the result record (rounds, samples, pixels_converged,
        pixels_capped, ms_total, ms_select)."""
        p = gpu.adaptive_params(tol, min_spp, max_spp, batch_spp, floor)
        self.raw_data, self.raw_data2, self.counts, res = gpu.render_adaptive_host(
            scene, self.size_x, self.size_y, p, self.seed, self.ctx)
        self.image = gpu.resolve_u8_counts(self.raw_data, self.counts, self.size_x, self.size_y)
        self.sample_count = int(self.counts.max())
        self.adaptive = True
        return res

    def render_features(self, scene, spp, spp_begin=None):
        """The first-hit features of passes spp_begin+1 .. spp_begin+spp (default: continue after the
        feature passes already taken) added to ``features``: the camera samples render() takes for the
        same passes.  Views: albedo, normal, depth, hit_fraction."""
        if spp_begin is None:
            spp_begin = self.feature_count
        gpu.render_features_host(scene, self.size_x, self.size_y, spp_begin, spp, self.seed, self.features, self.ctx)
        self.feature_count = spp_begin + spp
        return self.features

    def _feature_mean(self, lo, hi):
        if self.feature_count < 1:
            raise ValueError("no feature passes yet (render_features)")
        f = self.features.reshape(self.size_y, self.size_x, 8)[..., lo:hi] / float(self.feature_count)
        return f[..., 0] if hi - lo == 1 else f

    @property
    def albedo(self):
        """(ny, nx, 3), y-up: the mean first-hit texture value (the sky colour where the ray misses)."""
        return self._feature_mean(0, 3)

    @property
    def normal(self):
        """(ny, nx, 3): the mean first-hit normal (not renormalised; 0 for a miss)."""
        return self._feature_mean(3, 6)

    @property
    def depth(self):
        """(ny, nx): the mean first-hit t (0 for a miss)."""
        return self._feature_mean(6, 7)

    @property
    def hit_fraction(self):
        """(ny, nx): the fraction of the feature passes whose camera ray hit something."""
        return self._feature_mean(7, 8)

    def denoise(self, **params):
        """The variance-guided a-trous filter (rt_denoise) of raw_data, guided by ``features``; the moments
        raw_data2 / counts are used when an adaptive render filled them.  params: iterations,
        normal_squarings, sigma_z, sigma_l, albedo_floor (rtamd.denoise.DEFAULTS).  Fills ``denoised``
        (the filtered mean radiance, nx*ny*3) and returns it."""
        if self.feature_count < 1:
            raise ValueError("no feature passes yet (render_features)")
        if self.sample_count < 1:
            raise ValueError("nothing rendered yet")
        p = gpu.denoise_params(**dict(DENOISE_DEFAULTS, **params))
        self.denoised = gpu.denoise_host(self.size_x, self.size_y, p, self.raw_data,
                                         self.raw_data2 if self.adaptive else None,
                                         self.counts if self.adaptive else None, self.sample_count, self.features,
                                         self.feature_count, self.ctx)
        return self.denoised

    def denoised_image(self):
        """``denoised`` resolved like the image (sqrt, 8 bits)."""
        if self.denoised is None:
            raise ValueError("no denoised frame yet (denoise)")
        return gpu.resolve_u8(self.denoised, self.size_x, self.size_y, 1)

    def save_denoised_as_ppm(self, path="denoised.ppm"):
        write_ppm(path, self.denoised_image(), self.size_x, self.size_y)

    def save_as_ppm(self, path="test.ppm"):
        """main.scm:439-450 — P3, rows written top-down (flipping y-up rows)."""
        write_ppm(path, self.image, self.size_x, self.size_y)


def write_ppm(path, image, nx, ny):
    img = np.asarray(image, dtype=np.uint8).reshape(ny, nx, 3)
    with open(path, "w") as f:
        f.write("P3\n %d %d\n255\n" % (nx, ny))
        for y in range(ny):
            row = img[ny - y - 1]
            f.write("".join("%d %d %d\n" % (int(p[0]), int(p[1]), int(p[2])) for p in row))
