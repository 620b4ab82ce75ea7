#!/usr/bin/env python3
"""What the feature buffers and the denoiser cost and buy: one JSON line per figure.

usage: python tools/denoise_report.py [--config C2|C4] [--nx N --ny N] [--repeats 3] [--out FILE]

  features   `passes` feature passes (rt_render_features_device) against the same passes of rt_render_device:
             same process, alternating, `repeats` times each; ms per pass
  denoise    rt_denoise_device at the defaults with 1 .. 6 iterations, alternating, `repeats` times each: the
             median of k iterations minus that of k - 1 is the time of the step-2^(k-1) launch; against the
             iteration's algorithmic bytes (72 B read per pixel once + 32 B written) as achieved bytes/s
  payoff     RMSE and gamma-space RMSE (sqrt of the clamped mean, as the resolve) of the noisy mean and of the
             denoised one at 16 / 64 / 256 passes, against a uniform render of 4 x 256 passes with another
             seed; features from 16 passes and from all passes
  tuning     the 16-pass RMSE for other parameter values than the defaults, one changed at a time
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scheme-raytrace_amd"))

CONFIGS = {"C2": ("cover", 1920, 1080), "C4": ("cornell", 1024, 1024)}
SEED, REF_SEED = 0x5EED0002, 0x5EED00AD
COUNTS = (16, 64, 256)
ITER_BYTES = 72 + 32          # per pixel and iteration: guide 40 B + signal 32 B read once, signal 32 B written
TUNING = [dict(sigma_l=1.0), dict(sigma_l=2.0), dict(sigma_l=8.0), dict(sigma_z=0.03), dict(sigma_z=0.3),
          dict(normal_squarings=5), dict(normal_squarings=9), dict(iterations=4), dict(iterations=6),
          dict(albedo_floor=1e-3), dict(albedo_floor=0.05)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="C2", choices=sorted(CONFIGS))
    p.add_argument("--nx", type=int, default=0)
    p.add_argument("--ny", type=int, default=0)
    p.add_argument("--passes", type=int, default=16, help="passes per timed features / render call")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None, help="also append the lines to this file")
    a = p.parse_args()
    import numpy as np
    import torch
    from rtamd import denoise, gpu, scenes

    name, nx, ny = CONFIGS[a.config]
    nx, ny = a.nx or nx, a.ny or ny
    npx = nx * ny
    scene = scenes.SCENES[name](nx, ny)
    ctx = gpu.default_context(0)
    gpu.upload(scene, ctx)
    f64 = dict(dtype=torch.float64, device="cuda")
    acc, acc2, out = (torch.zeros(npx * 3, **f64) for _ in range(3))
    cnt = torch.zeros(npx, dtype=torch.int32, device="cuda")
    feat16, featN = torch.zeros(npx * 8, **f64), torch.zeros(npx * 8, **f64)
    pix = torch.from_numpy(gpu.shard_pixels(nx, ny, 0, 1).view(np.int32).copy()).cuda()
    head = {"config": a.config, "scene": name, "nx": nx, "ny": ny}

    def emit(kind, **kv):
        line = json.dumps(dict(head, figure=kind, **kv))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    def median(ms):
        return sorted(ms)[len(ms) // 2]

    def spread(ms):
        return {"ms": [round(x, 3) for x in ms], "ms_median": round(median(ms), 3), "ms_range": round(max(ms) - min(ms), 3)}

    def alternate(variants):
        ms = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                ms[k].append(timed(fn))
        return ms

    def features(buf, spp):
        buf.zero_()
        gpu.render_features_device(scene, nx, ny, 0, spp, SEED, buf.data_ptr(), ctx=ctx)

    def moments(spp):
        for t in (acc, acc2, cnt):
            t.zero_()
        gpu.render_pixels_device(scene, nx, ny, pix.data_ptr(), npx, 0, spp, SEED, acc.data_ptr(), acc2.data_ptr(),
                                 cnt.data_ptr(), ctx=ctx)

    def filt(fbuf, m, **kv):
        gpu.denoise_device(nx, ny, gpu.denoise_params(**dict(denoise.DEFAULTS, **kv)), acc.data_ptr(), acc2.data_ptr(),
                           cnt.data_ptr(), 0, fbuf.data_ptr(), m, out.data_ptr(), ctx=ctx)

    def uniform(spp, seed=SEED):
        acc.zero_()
        gpu.render_device(scene, nx, ny, 0, spp, seed, acc.data_ptr(), ctx=ctx)

    P = a.passes
    uniform(P)                                       # pools sized, kernels loaded
    features(feat16, 16)
    moments(16)
    filt(feat16, 16)

    # ---- features against a render of the same passes
    ms = alternate({"features": lambda: features(featN, P), "render": lambda: uniform(P)})
    emit("features", passes=P, ms_per_pass=round(median(ms["features"]) / P, 4),
         render_ms_per_pass=round(median(ms["render"]) / P, 4),
         vs_render=round(median(ms["features"]) / median(ms["render"]), 4),
         features=spread(ms["features"]), render=spread(ms["render"]))

    # ---- the denoiser, per iteration
    moments(16)
    ms = alternate({k: (lambda k=k: filt(feat16, 16, iterations=k)) for k in range(1, 7)})
    for k in range(1, 7):
        extra = {}
        if k > 1:
            step_ms = median(ms[k]) - median(ms[k - 1])
            extra = {"step": 1 << (k - 1), "step_ms": round(step_ms, 4),
                     "step_gbytes_per_s": round(npx * ITER_BYTES / (step_ms * 1e-3) / 1e9, 1) if step_ms > 0 else None}
        emit("denoise", iterations=k, algorithmic_bytes_per_iteration=npx * ITER_BYTES, **spread(ms[k]), **extra)

    # ---- what the filter buys
    uniform(4 * max(COUNTS), REF_SEED)
    ref = acc.cpu().numpy() / (4 * max(COUNTS))

    def errors(img):
        g = lambda x: np.sqrt(np.clip(x, 0.0, 1.0))
        return {"rmse": float(np.sqrt(np.mean((img - ref) ** 2))), "rmse_gamma": float(np.sqrt(np.mean((g(img) - g(ref)) ** 2)))}

    features(feat16, 16)
    for n in COUNTS:
        moments(n)
        noisy = errors(acc.cpu().numpy() / n)
        features(featN, n)
        filt(feat16, 16)
        d16 = errors(out.cpu().numpy())
        filt(featN, n)
        dN = errors(out.cpu().numpy())
        emit("payoff", passes=n, noisy=noisy, denoised_features16=d16, denoised_features_all=dN)
        if n == COUNTS[0]:
            for kv in TUNING:
                filt(feat16, 16, **kv)
                emit("tuning", passes=n, changed=kv, **errors(out.cpu().numpy()))


if __name__ == "__main__":
    main()
