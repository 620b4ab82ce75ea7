#!/usr/bin/env python3
"""Throughput and tree sizes of triangle scenes: one JSON line per scene.

usage: python tools/triangles_report.py [--nx 512 --ny 512 --spp 16] [--repeats 3] [--level 5] [--out FILE]

  ball_mesh       icosphere(level) (level 5: 20 480 triangles), lambertian, radius 90 in the Cornell room (its
                  six rects, no boxes)
  ball_sphere     the analytic sphere of that radius in the same room, for comparison
  cornell_mesh    the Cornell room with every rect and box face as two triangles (36 triangles)
  cornell_lifted  the same room in rects and boxes

Every scene is rendered `repeats` times after a warm-up: median and range of ms per pass and of Mrays/s (ray
segments per second), and what rt_get_tree_info and rt_get_scene_info report about its tree and commit.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scheme-raytrace_amd"))

SEED = 0x5EED0603


def room_with(nx, ny, ball):
    from rtamd import scene as g, scenes
    room = list(scenes.SCENES["cornell_lifted"](nx, ny).obj_list[:6])
    return g.make_scene(room + [ball], scenes.cornell_camera_for(nx, ny), g.sky_color)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nx", type=int, default=512)
    p.add_argument("--ny", type=int, default=512)
    p.add_argument("--spp", type=int, default=16)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--level", type=int, default=5)
    p.add_argument("--out", default=None, help="also append the lines to this file")
    a = p.parse_args()
    import torch
    from rtamd import gpu, mesh, scene as g, scenes

    ctx = gpu.default_context(0)
    acc = torch.zeros(a.nx * a.ny * 3, dtype=torch.float64, device="cuda")
    grey = g.make_lambertian(g.constant_texture((0.5, 0.5, 0.5)))
    c, r = (278.0, 120.0, 278.0), 90.0
    vs, fs = mesh.icosphere(a.level, radius=r, center=c)
    cases = [("ball_mesh", room_with(a.nx, a.ny, g.make_mesh(vs, fs, grey))),
             ("ball_sphere", room_with(a.nx, a.ny, g.make_sphere(c, r, grey))),
             ("cornell_mesh", scenes.SCENES["cornell_mesh"](a.nx, a.ny)),
             ("cornell_lifted", scenes.SCENES["cornell_lifted"](a.nx, a.ny))]

    def render(sc):
        acc.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = gpu.render_device(sc, a.nx, a.ny, 0, a.spp, SEED, acc.data_ptr(), ctx=ctx)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, int(gpu.stats(h).segments)

    for name, sc in cases:
        h = gpu.upload(sc, ctx)
        ti, si = gpu.tree_info(h), gpu.scene_info(h)
        _, segs = render(sc)                                    # warm-up
        ms = [render(sc)[0] for _ in range(a.repeats)]
        per = [m / a.spp for m in ms]
        mr = [segs / m / 1e3 for m in ms]
        line = {"scene": name, "nx": a.nx, "ny": a.ny, "spp": a.spp, "repeats": a.repeats, "segments": segs,
                "tri_leaves": ti["tri_leaves"], "generic_leaves": ti["generic_leaves"], "sphere_leaves": ti["sphere_leaves"],
                "group_leaves": ti["group_leaves"], "tree_nodes": ti["nodes"], "tree_depth": ti["depth"],
                "commit_ms": round(si["commit_ms"], 2), "commit_sah_ms": round(si["commit_sah_ms"], 2),
                "ms_per_pass": round(statistics.median(per), 4), "ms_per_pass_range": [round(min(per), 4), round(max(per), 4)],
                "mrays_s": round(statistics.median(mr), 1), "mrays_s_range": [round(min(mr), 1), round(max(mr), 1)]}
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
