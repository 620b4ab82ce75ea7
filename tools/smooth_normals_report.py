#!/usr/bin/env python3
"""What per-vertex shading normals cost: icosphere(level) (level 5: 20 480 triangles), metal,
radius 90 in the Cornell room (its six rects, no boxes), shaded flat and smooth.

usage: python tools/smooth_normals_report.py [--nx 512 --ny 512 --spp 16] [--rounds 3] [--repeats 1] [--level 5]
           [--parent path/to/librtamd_base.so] [--out profiles/smooth_normals/report.txt]

  flat     the mesh without normals (rt_add_mesh): DevScene::tri_smooth = 0, the hit record tests the flag only
  smooth   the mesh with radial normals (rt_add_mesh_normals)
  parent   the flat scene on a library built from the parent commit (--parent), which has no shading normals

Each variant is rendered in a process of its own (RTAMD_LIB selects the library): a warm-up, then `repeats`
timed renders.  The processes alternate parent / flat / smooth, `rounds` times, so drift of the machine hits
the variants alike (the default: 3 rounds of one render, the median of 3).  Reported per variant: the median and
the range of all its timed renders in ms per pass and Mrays/s (ray segments per second), the segment count and a
checksum of the frame (flat and parent must agree).
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0703


def child(a):
    sys.path.insert(0, os.path.join(ROOT, "scheme-raytrace_amd"))
    import torch
    from rtamd import gpu, scenes        # (a --parent library lacks rt_add_mesh_normals: rtamd._lib.OPTIONAL; it renders flat)
    sc = scenes.cornell_smooth(a.nx, a.ny, level=a.level, smooth=a.variant == "smooth")
    acc = torch.zeros(a.nx * a.ny * 3, dtype=torch.float64, device="cuda")

    def render():
        acc.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = gpu.render_device(sc, a.nx, a.ny, 0, a.spp, SEED, acc.data_ptr())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, int(gpu.stats(h).segments)

    _, segs = render()                                                       # warm-up (sizes the path pools)
    ms = [render()[0] for _ in range(a.repeats)]
    ti = gpu.tree_info(gpu.upload(sc))
    print(json.dumps({"ms": ms, "segments": segs, "tri_leaves": ti["tri_leaves"],
                      "sha": hashlib.sha1(acc.cpu().numpy().tobytes()).hexdigest()[:16]}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nx", type=int, default=512)
    p.add_argument("--ny", type=int, default=512)
    p.add_argument("--spp", type=int, default=16)
    p.add_argument("--repeats", type=int, default=1)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--level", type=int, default=5)
    p.add_argument("--parent", default=None, help="a librtamd.so built from the parent commit (flat scene only)")
    p.add_argument("--out", default=None, help="also write the report to this file")
    p.add_argument("--child", action="store_true")
    p.add_argument("--variant", default="flat")
    a = p.parse_args()
    if a.child:
        return child(a)
    variants = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("flat", None), ("smooth", None)]
    res = {}
    for r in range(a.rounds):
        for name, lib in variants:
            env = dict(os.environ)
            if lib:
                env["RTAMD_LIB"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--variant", "flat" if name == "parent" else name,
                                  "--nx", str(a.nx), "--ny", str(a.ny), "--spp", str(a.spp), "--repeats", str(a.repeats),
                                  "--level", str(a.level)], env=env, capture_output=True, text=True, timeout=600)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
            if out.returncode != 0 or not line:
                print("variant %s failed (exit %d):\n%s" % (name, out.returncode, out.stderr[-3000:]), flush=True)
                sys.exit(1)                                                  # nothing more is started on the GPU
            d = json.loads(line[-1])
            e = res.setdefault(name, {"ms": [], "segments": d["segments"], "sha": set(), "tri_leaves": d["tri_leaves"]})
            e["ms"] += d["ms"]
            e["sha"].add(d["sha"])
            print("round %d %-7s %s ms" % (r, name, " ".join("%.2f" % m for m in d["ms"])), flush=True)
    lines = ["icosphere(%d) in the Cornell room, %dx%dx%d, %d rounds of %d timed renders per variant (after a warm-up each)"
             % (a.level, a.nx, a.ny, a.spp, a.rounds, a.repeats)]
    for name, _ in variants:
        e = res[name]
        per = [m / a.spp for m in e["ms"]]
        mr = [e["segments"] / m / 1e3 for m in e["ms"]]
        lines.append("%-7s tri_leaves %6d segments %9d  ms/pass median %.4f range %.4f .. %.4f  Mrays/s median %.1f range %.1f .. %.1f  "
                     "sha %s" % (name, e["tri_leaves"], e["segments"], statistics.median(per), min(per), max(per),
                                 statistics.median(mr), min(mr), max(mr), ",".join(sorted(e["sha"]))))
    if a.parent:
        f, q = statistics.median(res["flat"]["ms"]), statistics.median(res["parent"]["ms"])
        spread = (max(res["parent"]["ms"]) - min(res["parent"]["ms"])) / q
        lines.append("flat vs parent: %+.2f %% in the median ms (the parent's own spread: %.2f %% of its median); frames %s"
                     % (100.0 * (f - q) / q, 100.0 * spread, "equal" if res["flat"]["sha"] == res["parent"]["sha"] else "DIFFER"))
    s, f = statistics.median(res["smooth"]["ms"]), statistics.median(res["flat"]["ms"])
    lines.append("smooth vs flat: %+.2f %% in the median ms, %+.2f %% segments" %
                 (100.0 * (s - f) / f, 100.0 * (res["smooth"]["segments"] - res["flat"]["segments"]) / res["flat"]["segments"]))
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
