"""bench.py's --dump-outputs writer (dump_outputs): the frame accumulator as
float64 and the resolved image as float32, whole while both fit the size
budget and at one fixed, seeded subset of the pixels beyond it; and a plain
one-GPU run of bench.py itself, whose dumped frame is the frame
rt_render_device gives."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs(nx, ny, seed):
    rng = np.random.RandomState(seed)
    return rng.random_sample(nx * ny * 3) * 1024.0, rng.randint(0, 256, nx * ny * 3).astype(np.uint8)


def test_dump_small_frame_is_written_whole(tmp_path):
    nx, ny = 37, 21
    frame, image = _outputs(nx, ny, 1)
    bench.dump_outputs(str(tmp_path / "o"), frame, image, nx, ny)
    assert sorted(os.listdir(tmp_path / "o")) == ["frame.npy", "image.npy"]
    f, i = np.load(tmp_path / "o" / "frame.npy"), np.load(tmp_path / "o" / "image.npy")
    assert f.dtype == np.float64 and i.dtype == np.float32 and f.shape == i.shape == (nx * ny, 3)
    assert np.array_equal(f.ravel(), frame) and np.array_equal(i.ravel(), image.astype(np.float32))


def test_dump_large_frame_is_a_fixed_sample_within_the_budget(tmp_path):
    nx, ny = 1920, 1080                      # the benchmark's frame: 36 B per pixel exceeds the budget
    frame, image = _outputs(nx, ny, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame, image, nx, ny)
    size = sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a"))
    assert size <= bench.DUMP_BUDGET_BYTES == 64 * 10 ** 6
    f, i = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "a" / "image.npy")
    assert f.dtype == np.float64 and i.dtype == np.float32 and f.shape == i.shape
    assert nx * ny // 2 < f.shape[0] < nx * ny
    # the same pixels on every run, the same rows of both arrays, in ascending pixel order
    assert np.array_equal(f, np.load(tmp_path / "b" / "frame.npy"))
    assert np.array_equal(i, np.load(tmp_path / "b" / "image.npy"))
    idx = np.sort(np.random.RandomState(bench.DUMP_SEED).permutation(nx * ny)[:f.shape[0]])
    assert np.array_equal(f, frame.reshape(-1, 3)[idx])
    assert np.array_equal(i, image.reshape(-1, 3)[idx].astype(np.float32))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_frame(sched, tmp_path):
    """A plain run (no --full) in a fresh child process: --steps sets the timed steps, the line carries the
    headline fields and ms_per_step and none of the --full legs, and the dumped outputs are what one
    rt_render_device + rt_resolve_u8_device call with the same arguments gives, bit for bit."""
    import torch
    from rtamd import gpu, scenes
    nx, ny, spp, seed = 96, 54, 3, 0x5EED0002
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--spp", str(spp), "--nx", str(nx), "--ny", str(ny), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["metric"] == bench.metric_for("cover", nx, ny, spp)
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value = segments / time: the line's own counters give it back from ms_per_step (rounded to 1 us)
    segs = d["extend_rays_per_step"] + d["tail_segments_per_step"]
    assert d["value"] == pytest.approx(segs / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    for k in ("cpu_baseline", "parity", "parity_frame", "roofline", "roofline_frame", "roofline_shade"):
        assert d[k] is None, k
    frame = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda")
    image = torch.zeros(nx * ny * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu.render_device(scenes.random_scene(nx, ny), nx, ny, 0, spp, seed, frame.data_ptr(), ctx=sched)
    torch.cuda.synchronize()
    gpu.resolve_u8_device(frame.data_ptr(), nx, ny, spp, image.data_ptr(), ctx=sched)
    torch.cuda.synchronize()
    assert np.array_equal(np.load(out / "frame.npy").ravel(), frame.cpu().numpy())
    assert np.array_equal(np.load(out / "image.npy").ravel(), image.cpu().numpy().astype(np.float32))
