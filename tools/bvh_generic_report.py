#!/usr/bin/env python3
"""Where the world tree overtakes the brute-force groups for rects and instanced spheres: one
JSON line per scene size.

usage: python tools/bvh_generic_report.py [--nx 512 --ny 512 --spp 16] [--repeats 3] [--out FILE]
                                           [--boxes 4,16,...] [--spheres 64,256,...]

  box_field  n boxes (6 n rects) of seeded random heights on a square, under make-bvh-node, gradient sky
  cluster    n small spheres, each under translate o rotate-y (one instance chain), over a ground rect

Each scene is committed twice in one process — with the tree (RTAMD_BVH_GENERIC_MIN=1, read at commit) and
with the groups (the threshold out of reach) — and rendered alternately, `repeats` times each after a
warm-up: median and range of ms per pass and of Mrays/s (ray segments per second), and whether the two
frames are the same bit for bit.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scheme-raytrace_amd"))

ENV = "RTAMD_BVH_GENERIC_MIN"
SEED = 0x5EED0409


def box_field(nx, ny, n):
    from rtamd import scene as g, scenes, vec as v
    from rtamd.rng import HostStream
    side = max(1, int(round(n ** 0.5)))
    rr = HostStream(0x5EED040A)
    w = 8.0 / side
    boxes = []
    for i in range(side):
        for j in range(side):
            x0, z0 = -4 + i * w, -4 + j * w
            mat = g.make_lambertian(g.constant_texture(v.vec3(0.2 + 0.6 * rr(), 0.2 + 0.6 * rr(), 0.2 + 0.6 * rr())))
            boxes.append(g.make_box(v.vec3(x0, 0, z0), v.vec3(x0 + w, 0.2 + 0.8 * rr(), z0 + w), mat))
    return g.make_scene([g.make_bvh_node(boxes, 0, 1)], scenes.camera_for(nx, ny), g.sky_color), 6 * side * side


def cluster(nx, ny, n):
    from rtamd import scene as g, scenes, vec as v
    from rtamd.rng import HostStream
    rr = HostStream(0x5EED040B)
    mats = [g.make_lambertian(g.constant_texture(v.vec3(0.7, 0.6, 0.5))),
            g.make_metal(g.constant_texture(v.vec3(0.8, 0.8, 0.9)), 0.1), g.make_dielectric(1.5)]
    r = 1.2 / n ** (1.0 / 3.0)
    sph = [g.translate(g.rotate_y(g.make_sphere(v.vec3(4 * rr(), 0.2 + 2 * rr(), 4 * rr()), r * (0.3 + 0.4 * rr()),
                                                mats[i % 3]), 15), v.vec3(-2.5, 0, -2))
           for i in range(n)]
    ground = g.make_xz_rect(-6, 6, -6, 6, 0, g.make_lambertian(g.constant_texture(v.vec3(0.4, 0.5, 0.3))))
    return g.make_scene([ground, g.make_bvh_node(sph, 0, 1)], scenes.camera_for(nx, ny), g.sky_color), n + 1


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nx", type=int, default=512)
    p.add_argument("--ny", type=int, default=512)
    p.add_argument("--spp", type=int, default=16)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--boxes", default="4,16,64,256,1024,4096")
    p.add_argument("--spheres", default="64,256,1024,4096")
    p.add_argument("--out", default=None, help="also append the lines to this file")
    a = p.parse_args()
    import torch
    from rtamd import gpu

    ctx = gpu.default_context(0)
    acc = torch.zeros(a.nx * a.ny * 3, dtype=torch.float64, device="cuda")

    def commit(make, n, tree):
        os.environ[ENV] = "1" if tree else "1000000000"
        sc, leaves = make(a.nx, a.ny, n)
        h = gpu.upload(sc, ctx)
        del os.environ[ENV]
        return sc, h, leaves

    def render(sc):
        acc.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = gpu.render_device(sc, a.nx, a.ny, 0, a.spp, SEED, acc.data_ptr())
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, int(gpu.stats(h).segments), acc.clone()

    def summary(ms, segs):
        per = [m / a.spp for m in ms]
        mr = [segs / m / 1e3 for m in ms]
        return {"ms_per_pass": round(statistics.median(per), 4), "ms_per_pass_range": [round(min(per), 4), round(max(per), 4)],
                "mrays_s": round(statistics.median(mr), 1), "mrays_s_range": [round(min(mr), 1), round(max(mr), 1)]}

    for kind, make, sizes in (("box_field", box_field, a.boxes), ("cluster", cluster, a.spheres)):
        for n in [int(x) for x in sizes.split(",") if x]:
            tree, ht, leaves = commit(make, n, True)
            grp, hg, _ = commit(make, n, False)
            ti = gpu.tree_info(ht)
            assert ti["generic_leaves"] > 0 and gpu.tree_info(hg)["generic_leaves"] == 0
            _, segs_t, img_t = render(tree)                      # warm-up (and the frames to compare)
            _, segs_g, img_g = render(grp)
            ms_t, ms_g = [], []
            for _ in range(a.repeats):
                ms_t.append(render(tree)[0])
                ms_g.append(render(grp)[0])
            line = {"scene": kind, "n": n, "generic_leaves": ti["generic_leaves"], "group_leaves_off": leaves,
                    "nx": a.nx, "ny": a.ny, "spp": a.spp, "repeats": a.repeats, "segments": segs_t,
                    "same_frame": bool(torch.equal(img_t, img_g)) and segs_t == segs_g,
                    "tree": summary(ms_t, segs_t), "groups": summary(ms_g, segs_g),
                    "tree_nodes": ti["nodes"], "tree_depth": ti["depth"]}
            line["speedup"] = round(line["groups"]["ms_per_pass"] / line["tree"]["ms_per_pass"], 3)
            s = json.dumps(line)
            print(s, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(s + "\n")


if __name__ == "__main__":
    main()
