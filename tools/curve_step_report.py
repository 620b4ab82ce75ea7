#!/usr/bin/env python3
"""profiles/curve_step/report.txt: the curve step records of tests/curve_step_cases.py, per scene, class and mode, with
the comparisons of tests/test_gpu_curve_step.py counted instead of asserted.  Needs a GPU.
usage: python tools/curve_step_report.py [out.txt]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "scheme-raytrace_amd", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))

import numpy as np  # noqa: E402

import curve_step_cases as cc  # noqa: E402
import oracle  # noqa: E402
import scatter_cases as sc  # noqa: E402
import test_gpu_curve_step as t  # noqa: E402
from rtamd import gpu  # noqa: E402

EXTEND = {0: "k_extend<F>", 1: "k_extend_curves<0>", 2: "k_extend_curves<1> (fused, device libm)",
          3: "k_extend_curves<2> (fused, exact libm)"}


def main(out):
    oracle.lib()
    ctx = gpu.default_context(0)
    lines = ["# one step (RT_STEP_STEP + RT_STEP_EXTEND_HBM, exact libm) against orc_step: records, the oracle's curve hits,",
             "# differing fields (of %d per record: %s), the extend that ran" % (len(t.FIELDS), ", ".join(t.FIELDS)),
             "%-15s %-11s %-6s %7s %10s %9s  %s" % ("scene", "class", "mode", "records", "curve hits", "differing", "instance")]
    for name in list(cc.CASES) + list(cc.GROUP_CASES):
        ctx.reset_options()
        ctx.set_option("exact_libm", "exact")
        for cls, r in cc.records(oracle, name).items():
            depth = 0 if cls == "moving" else 1
            T = sc.throughputs(len(r), depth)
            e = t.expect(oracle, name, r.rays, r.ctr, depth, T)
            got = t.step(cc.scene(name), r.rays, r.ctr, depth, T)
            bad = t.compare(got, e, len(r), cls in t.EXACT_MAT)
            lines.append("%-15s %-11s %-6s %7d %10d %9d  %s" % (
                name, cls, "step", len(r), int(cc.curve_hits(name, e.rows, r.rays).sum()),
                sum(int(b.sum()) for b in bad.values()), EXTEND[got.extend]))
    lines += ["", "# RT_STEP_FUSED and RT_STEP_TAIL against RT_STEP_STEP iterated to the paths' ends: records whose colour differs;",
              "# fused: the launch's continuation segments / the iteration's"]
    for name, (depth, n) in t.FUSED_RUNS.items():
        rays, ctr = cc.mixed(oracle, name)
        pick = np.linspace(0, len(rays) - 1, n).astype(int)
        rays, ctr = rays[pick], ctr[pick]
        T = sc.throughputs(n, 1)
        for libm in ("exact", "device"):
            ctx.reset_options()
            ctx.set_option("exact_libm", libm)
            want, segs = t.iterate_steps(cc.scene(name), rays, ctr, depth, T)
            f = t.step(cc.scene(name), rays, ctr, depth, T, mode=gpu.STEP_FUSED)
            lines.append("%-15s %-11s %-6s %7d %10s %9d  %s, depth %d on, %s libm, segments %d / %d" % (
                name, "mixed", "fused", n, "-", int((~sc.same_bits(f.color, want).all(axis=1)).sum()), EXTEND[f.extend],
                depth, libm, f.survivors, segs))
            if depth == 1:
                tail = t.step(cc.scene(name), rays, ctr, depth, T, mode=gpu.STEP_TAIL)
                lines.append("%-15s %-11s %-6s %7d %10s %9d  k_finish<F %d, TL %d, LS %d, SOLO %d, EX %d>, %s libm" % (
                    (name, "mixed", "tail", n, "-", int((~sc.same_bits(tail.color, want).all(axis=1)).sum())) +
                    tuple(int(x) for x in tail.finish) + (libm,)))
    ctx.reset_options()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "curve_step", "report.txt"))
