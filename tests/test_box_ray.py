"""The f32 box-ray setup of the BVH walks (scheme-raytrace_amd/csrc/rt_boxray.h) is a conservative cull
inside the margin commit widens the boxes by (2^-21 R, rt_build.cpp world_tree): the same header compiled
by g++ against the exact slab interval in long double (tests/csrc/box_ray_check.cpp), with the reciprocal
as the host computes it and one ulp either side of it."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_f32_box_ray_culls_no_hit(tmp_path):
    exe = str(tmp_path / "box_ray_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                           os.path.join(HERE, "csrc", "box_ray_check.cpp")])
    run = subprocess.run([exe, "-21"], capture_output=True, text=True)
    out = run.stdout.strip().splitlines()
    print("\n".join(out[-12:]))
    cases, hits, culled = (int(x) for x in out[-1].split())
    # per R: 2^20 seeded triples and 6 x 2^17 adversarial ones; well over a third of them must be exact hits
    assert cases == 2 * ((1 << 20) + 6 * (1 << 17))
    assert hits > cases // 3
    assert culled == 0 and run.returncode == 0, out
