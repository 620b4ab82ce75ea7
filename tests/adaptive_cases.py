"""Shared by test_adaptive_host.py and test_gpu_adaptive.py: the adaptive cases and the oracle's per-pass
colours for them (computed once per session)."""
import functools

import numpy as np

from conftest import host_threads
from rtamd import scenes

SEED = 0x5EED0002
#: scene name, nx, ny
CASES = [("cornell", 48, 48), ("cover", 64, 36), ("curves_small", 48, 32)]
#: the rounds and the stop rule every case runs with
MIN_SPP, BATCH_SPP, MAX_SPP, TOL, FLOOR = 4, 4, 24, 0.2, 0.05


@functools.lru_cache(maxsize=None)
def scene_of(name, nx, ny):
    return scenes.SCENES[name](nx, ny)


@functools.lru_cache(maxsize=None)
def oracle_scene(name, nx, ny):
    import oracle
    return oracle.build_scene(scene_of(name, nx, ny))


@functools.lru_cache(maxsize=None)
def oracle_passes(name, nx, ny):
    """The oracle's colours of passes 0 .. MAX_SPP-1, one read-only (npix, 3) array per pass."""
    o = oracle_scene(name, nx, ny)
    out = []
    for k in range(MAX_SPP):
        a, _ = o.render(nx, ny, k, 1, SEED, nthreads=host_threads())
        a = a.reshape(-1, 3)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def tile_order(nx, ny):
    """The full-frame pixel list (16x16 tiles, row-major tile order) the adaptive render starts from."""
    from rtamd import gpu
    return gpu.shard_pixels(nx, ny, 0, 1)
