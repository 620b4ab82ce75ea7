#!/usr/bin/env python3
"""What sampling a list of lights costs: ms per pass, Mrays/s and the noise of the frame.

usage: python tools/light_list_report.py [--nx 512 --ny 512 --spp 16] [--repeats 3] [--out FILE]

  cornell_mixture        cornell-box, its lamp the single light (rt_set_light_sampling)
  lamp_two_half_rects    the same room, the lamp sampled as two half rects (a list of 2)
  lamp_two_triangles     the same room, the lamp sampled as its two triangles (a list of 2)
  cornell_mesh_lights    the room as 36 triangles, its lamp mesh as the list
  ball_k_list, k = 0..3  an emissive icosphere(k) (20 .. 1280 triangles) in the lifted room (its six rects), the
                         ball's mesh as the list
  ball_k_off             the same scene with light sampling off

Every scene is rendered `repeats` times after a warm-up: the median (and range) of ms per pass and of Mrays/s
(ray segments per second).  The time is host wall time around the render call and a synchronise, so renders of
a few ms carry launch and synchronise overhead.  Then `spp` single passes give the frame mean of A = mean over channels of
min(x, 1) per sample and the standard error of that mean (the statistic of tests/test_gpu_light_list.py).  The
pdf loop visits every light of the list for every lambertian bounce, so the cost is linear in the list's
length; the table says where that starts to matter.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scheme-raytrace_amd"))

SEED = 0x5EED0702


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nx", type=int, default=512)
    p.add_argument("--ny", type=int, default=512)
    p.add_argument("--spp", type=int, default=16)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=None, help="also write the table to this file")
    a = p.parse_args()
    import numpy as np
    import torch
    from rtamd import gpu, mesh, scene as g, scenes

    nx, ny = a.nx, a.ny
    ctx = gpu.default_context(0)
    acc = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda")
    emit = g.make_diffuse_light(g.constant_texture((3, 3, 3)))
    box = scenes.cornell_box(nx, ny)

    def room(**kw):
        return g.make_scene(box.obj_list, box.camera, box.sky_function, **kw)

    halves = [g.flip_normals(g.make_xz_rect(213, 278, 227, 332, 554, emit)), g.flip_normals(g.make_xz_rect(278, 343, 227, 332, 554, emit))]
    vs, fs, _ = mesh.rect_quad(1, 213, 343, 227, 332, 554, True)
    tris = [g.make_triangle(vs[f[0]], vs[f[1]], vs[f[2]], emit) for f in fs]
    cases = [("cornell_mixture", scenes.cornell_mixture(nx, ny), 1), ("lamp_two_half_rects", room(lights=halves), 2),
             ("lamp_two_triangles", room(lights=tris), 2), ("cornell_mesh_lights", scenes.SCENES["cornell_mesh_lights"](nx, ny), 2)]
    lifted = list(scenes.SCENES["cornell_lifted"](nx, ny).obj_list[:6])
    for k in range(4):
        bv, bf = mesh.icosphere(k, radius=90.0, center=(278.0, 120.0, 278.0))
        ball = g.make_mesh(bv, bf, emit)
        cam = scenes.cornell_camera_for(nx, ny)
        cases.append(("ball_%d_list" % k, g.make_scene(lifted + [ball], cam, g.sky_color, lights=[ball]), len(bf)))
        cases.append(("ball_%d_off" % k, g.make_scene(lifted + [ball], cam, g.sky_color), 0))

    def render(sc, first, passes):
        acc.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = gpu.render_device(sc, nx, ny, first, passes, SEED, acc.data_ptr(), ctx=ctx)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, int(gpu.stats(h).segments)

    lines = ["%dx%dx%d, median of %d after a warm-up; A = mean over channels of min(x, 1) per sample, over %d single passes"
             % (nx, ny, a.spp, a.repeats, a.spp),
             "ms/pass is host wall time (a whole render call and a device synchronise, divided by the passes): renders of "
             "a few ms include launch and synchronise overhead, so read small differences between the small scenes with that in mind;",
             "Mrays/s = the render's ray segments over that time (a scene whose paths end sooner traces fewer segments per pass)",
             "%-22s %6s %10s %19s %10s %17s %9s %10s" % ("scene", "lights", "ms/pass", "range", "Mrays/s", "range", "mean A", "se")]
    for name, sc, m in cases:
        _, segs = render(sc, 0, a.spp)                              # warm-up
        ms = [render(sc, 0, a.spp)[0] for _ in range(a.repeats)]
        per = [x / a.spp for x in ms]
        mr = [segs / x / 1e3 for x in ms]
        S = np.zeros(nx * ny)
        Q = np.zeros(nx * ny)
        for k in range(a.spp):
            render(sc, k, 1)
            s = np.minimum(acc.cpu().numpy().reshape(-1, 3), 1.0).mean(axis=1)
            S += s
            Q += s * s
        mean = S / a.spp
        var_mean = (Q / a.spp - mean * mean) * (a.spp / (a.spp - 1.0)) / a.spp
        lines.append("%-22s %6d %10.4f %8.4f .. %8.4f %10.1f %7.1f .. %7.1f %9.6f %10.3e"
                     % (name, m, statistics.median(per), min(per), max(per), statistics.median(mr), min(mr), max(mr),
                        mean.mean(), np.sqrt(var_mean.sum() / mean.size ** 2)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
