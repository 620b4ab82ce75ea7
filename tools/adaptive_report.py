#!/usr/bin/env python3
"""What adaptive sampling costs and buys ("Adaptive sampling"): one JSON line per figure.

usage: python tools/adaptive_report.py [--config C2|C4] [--nx N --ny N --max-spp N] [--repeats 3] [--out FILE]

  overhead   the adaptive call with min_spp == max_spp (one round: moments + one selection), and with
             min = batch = 64, tol = 1e-30 (every round runs, nearly every pixel stays active), against
             rt_render_device of the same passes: same process, alternating, `repeats` times each
  payoff     at a tol (found by bisection) where the mean count is about max_spp / 2, for rounds of 16 and
             of 64 passes: wall time, total samples, and the error of accum / count against a uniform
             render of 4 x max_spp passes with another seed (RMSE, and the channel sum's error relative to
             b = max(channel sum, floor), the quantity tol bounds: RMS and 99th percentile); beside it a
             uniform render of the same total sample budget
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scheme-raytrace_amd"))

CONFIGS = {"C2": ("cover", 1920, 1080, 1024), "C4": ("cornell", 1024, 1024, 256)}
SEED, REF_SEED = 0x5EED0002, 0x5EED00AD


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="C2", choices=sorted(CONFIGS))
    p.add_argument("--nx", type=int, default=0)
    p.add_argument("--ny", type=int, default=0)
    p.add_argument("--max-spp", type=int, default=0)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None, help="also append the lines to this file")
    a = p.parse_args()
    import numpy as np
    import torch
    from rtamd import gpu, scenes

    name, nx, ny, M = CONFIGS[a.config]
    nx, ny, M = a.nx or nx, a.ny or ny, a.max_spp or M
    npx = nx * ny
    scene = scenes.SCENES[name](nx, ny)
    ctx = gpu.default_context(0)
    gpu.upload(scene, ctx)
    acc = torch.zeros(npx * 3, dtype=torch.float64, device="cuda")
    acc2 = torch.zeros(npx * 3, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(npx, dtype=torch.int32, device="cuda")
    head = {"config": a.config, "scene": name, "nx": nx, "ny": ny, "max_spp": M}

    def emit(kind, **kv):
        line = json.dumps(dict(head, figure=kind, **kv))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    def uniform(spp, seed=SEED):
        acc.zero_()
        gpu.render_device(scene, nx, ny, 0, spp, seed, acc.data_ptr(), ctx=ctx)

    def adaptive(tol, mn, mx, batch):
        return gpu.render_adaptive_device(scene, nx, ny, gpu.adaptive_params(tol, mn, mx, batch, 0.05), SEED,
                                          acc.data_ptr(), acc2.data_ptr(), cnt.data_ptr(), ctx=ctx)

    def spread(ms):
        return {"ms": [round(x, 2) for x in ms], "ms_median": round(sorted(ms)[len(ms) // 2], 2),
                "ms_spread": round(max(ms) - min(ms), 2)}

    uniform(min(M, 16))                              # pools sized, kernels loaded
    adaptive(0.0, 2, 2, 1)

    # ---- overhead of the machinery
    variants = {"uniform": lambda: uniform(M),
                "one_round": lambda: adaptive(0.0, M, M, 1),
                "every_round_batch64": lambda: adaptive(1e-30, min(64, M), M, 64)}
    ms = {k: [] for k in variants}
    last = {}
    for _ in range(a.repeats):
        for k, fn in variants.items():               # alternating
            t, r = timed(fn)
            ms[k].append(t)
            last[k] = r
    base = sorted(ms["uniform"])[len(ms["uniform"]) // 2]
    for k in variants:
        extra = {}
        if last[k]:
            extra = {"rounds": last[k]["rounds"], "samples": last[k]["samples"],
                     "ms_select": round(last[k]["ms_select"], 3)}
        emit("overhead", variant=k, vs_uniform=round(sorted(ms[k])[len(ms[k]) // 2] / base, 4), **spread(ms[k]), **extra)

    # ---- payoff at a mean count of about max_spp / 2, for rounds of 16 and of 64 passes
    uniform(4 * M, REF_SEED)
    ref = acc.cpu().numpy().reshape(-1, 3) / (4 * M)
    ref_b = np.maximum(ref.sum(axis=1), 0.05)          # the rule's b = max(mean of the channel sum, floor)

    def errors(mean_img):
        """RMSE per channel value, and the RMS of the channel sum's error relative to b (what tol bounds)."""
        return {"rmse_vs_4x": float(np.sqrt(np.mean((mean_img - ref) ** 2))),
                "rel_rms_vs_4x": float(np.sqrt(np.mean(((mean_img.sum(axis=1) - ref.sum(axis=1)) / ref_b) ** 2))),
                "rel_p99_vs_4x": float(np.percentile(np.abs(mean_img.sum(axis=1) - ref.sum(axis=1)) / ref_b, 99))}

    mn = min(16, M)
    for batch in (16, 64):
        lo, hi = 1e-4, 1.0                           # mean count falls as tol rises
        tol, res = None, None
        for _ in range(12):
            tol = (lo * hi) ** 0.5
            res = adaptive(tol, mn, M, batch)
            mean = res["samples"] / npx
            if abs(mean - M / 2) <= 0.05 * M:
                break
            if mean > M / 2:
                lo = tol
            else:
                hi = tol
        t_ad = []
        for _ in range(a.repeats):
            t, res = timed(lambda: adaptive(tol, mn, M, batch))
            t_ad.append(t)
        c = cnt.cpu().numpy().astype(np.float64)
        emit("payoff", variant="adaptive", tol=tol, min_spp=mn, batch_spp=batch, rounds=res["rounds"],
             samples=res["samples"], mean_count=round(res["samples"] / npx, 2), pixels_capped=res["pixels_capped"],
             ms_select=round(res["ms_select"], 3), **errors(acc.cpu().numpy().reshape(-1, 3) / c[:, None]), **spread(t_ad))
        spp_u = max(1, int(round(res["samples"] / npx)))
        t_un = []
        for _ in range(a.repeats):
            t, _ = timed(lambda: uniform(spp_u))
            t_un.append(t)
        emit("payoff", variant="uniform_same_budget", batch_spp=batch, spp=spp_u, samples=spp_u * npx,
             **errors(acc.cpu().numpy().reshape(-1, 3) / spp_u), **spread(t_un))
    t_full, _ = timed(lambda: uniform(M))
    emit("payoff", variant="uniform_max_spp", spp=M, samples=M * npx, ms=[round(t_full, 2)],
         **errors(acc.cpu().numpy().reshape(-1, 3) / M))


if __name__ == "__main__":
    main()
