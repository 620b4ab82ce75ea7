#!/usr/bin/env python3
"""What a media forest buys: scenes.next_week with the book's two constant media, rendered
with the segments' trees and with the brute-force groups; one JSON line per commit.

usage: python tools/bvh_media_report.py [--tree DIR] [--label NAME] [--nx 512 --ny 512 --spp 16]
                                        [--repeats 3] [--out FILE]

  --tree DIR   the checkout whose package and library are measured (default: this one).  A checkout from
               before media forests has no scenes.SCENES["next_week_media"]: the same object list is then put
               together here from its scenes.next_week, and its commit scans the groups.

Protocol of tools/bvh_generic_report.py: a warm-up render, then `repeats` timed ones per commit, alternating
where a build offers both commits (the forest, and the groups with RTAMD_BVH_GENERIC_MIN out of reach);
median and range of ms per pass and of Mrays/s (ray segments per second); the frame as a hash of the
accumulator's bytes and the segment count, to compare across lines and builds.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ENV = "RTAMD_BVH_GENERIC_MIN"
SEED = 0x5EED0506


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    p.add_argument("--label", default="this")
    p.add_argument("--nx", type=int, default=512)
    p.add_argument("--ny", type=int, default=512)
    p.add_argument("--spp", type=int, default=16)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None, help="also append the lines to this file")
    a = p.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "scheme-raytrace_amd"))
    import torch
    from rtamd import gpu, scenes
    from rtamd import scene as g
    from rtamd import vec as v

    def make(nx, ny):
        if "next_week_media" in scenes.SCENES:
            return scenes.SCENES["next_week_media"](nx, ny)
        base = scenes.next_week(nx, ny)
        objs = list(base.obj_list)
        glass = objs[5]
        assert glass.kind == "sphere" and glass.args[1] == 70
        objs[6:6] = [g.make_constant_medium(g.make_sphere(glass.args[0], 70, g.make_dielectric(1.5)), 0.2,
                                            g.constant_texture(v.vec3(0.2, 0.4, 0.9))),
                     g.make_constant_medium(g.make_sphere(v.vec3(0, 0, 0), 5000, g.make_dielectric(1.5)), 0.0001,
                                            g.constant_texture(v.vec3(1, 1, 1)))]
        return g.make_scene(objs, base.camera, base.sky_function, perlin=base.perlin)

    ctx = gpu.default_context(0)
    acc = torch.zeros(a.nx * a.ny * 3, dtype=torch.float64, device="cuda")

    def commit(groups):
        if groups:
            os.environ[ENV] = "1000000000"
        sc = make(a.nx, a.ny)
        h = gpu.upload(sc, ctx)
        os.environ.pop(ENV, None)
        return sc, h

    def render(sc):
        acc.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = gpu.render_device(sc, a.nx, a.ny, 0, a.spp, SEED, acc.data_ptr())
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, int(gpu.stats(h).segments), hashlib.sha1(acc.cpu().numpy().tobytes()).hexdigest()[:16]

    commits = [("tree", *commit(False))]
    ti = gpu.tree_info(commits[0][2])
    if ti.get("segment_trees", 0) > 0:
        commits.append(("groups", *commit(True)))
    else:
        commits[0] = ("groups",) + commits[0][1:]
    first = {name: render(sc) for name, sc, _ in commits}                   # warm-up, and the frames to compare
    ms = {name: [] for name, _, _ in commits}
    for _ in range(a.repeats):
        for name, sc, _ in commits:
            ms[name].append(render(sc)[0])
    for name, _, h in commits:
        _, segs, frame = first[name]
        per = [m / a.spp for m in ms[name]]
        mr = [segs / m / 1e3 for m in ms[name]]
        info = gpu.tree_info(h)
        line = {"scene": "next_week_media", "build": a.label, "commit": name, "nx": a.nx, "ny": a.ny, "spp": a.spp,
                "repeats": a.repeats, "segments": segs, "frame": frame,
                "ms_per_pass": round(statistics.median(per), 4), "ms_per_pass_range": [round(min(per), 4), round(max(per), 4)],
                "mrays_s": round(statistics.median(mr), 1), "mrays_s_range": [round(min(mr), 1), round(max(mr), 1)],
                "tree_info": {k: info[k] for k in ("sphere_leaves", "generic_leaves", "group_leaves", "nodes", "depth",
                                                   "nodes0", "depth0", "segments", "segment_trees") if k in info}}
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
