"""Frame digests of every scene in rtamd.scenes.SCENES, to compare two builds of the library bit for bit:
NX x NY (default 96x64), SPP passes (default 4), fixed seed.  Per scene one line with four SHA-256:
  default   the accumulator under the library's own schedule (at the default size: the tail kernel alone)
  tail      the accumulator with every path of depth >= 1 in the tail kernel (RT_OPT_TAIL_PATHS above any pool)
  wavefront the accumulator with the tail kernel off (RT_OPT_TAIL_OFF): the extend and shade kernels at every depth
  features  the feature buffer of rt_render_features
Run on the GPU box, once per build: [RTAMD_LIB=path/to/librtamd.so NX=96 NY=64 SPP=4] python tools/frame_digests.py
[scene ...]; the lines of two builds must be equal (diff the outputs)."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scheme-raytrace_amd"))
from rtamd import gpu, scenes  # noqa: E402

nx, ny, spp = int(os.environ.get("NX", 96)), int(os.environ.get("NY", 64)), int(os.environ.get("SPP", 4))
seed = 0x5EED0002
ctx = gpu.default_context()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def frame(sc, tail_paths, tail_off=0):
    ctx.set_option("tail_paths", tail_paths)
    ctx.set_option("tail_off", tail_off)
    acc = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda")
    gpu.render_device(sc, nx, ny, 0, spp, seed, acc.data_ptr())
    torch.cuda.synchronize()
    return acc.cpu().numpy()


for name in sys.argv[1:] or list(scenes.SCENES):
    sc = scenes.SCENES[name](nx, ny)
    default = sha(frame(sc, 0))
    tail = sha(frame(sc, 1 << 30))
    wave = sha(frame(sc, 0, 1))
    ctx.set_option("tail_off", 0)
    feat = np.zeros(nx * ny * 8, dtype=np.float64)
    gpu.render_features_host(sc, nx, ny, 0, spp, seed, feat)
    print("%-16s %dx%dx%d default %s tail %s wavefront %s features %s"
          % (name, nx, ny, spp, default, tail, wave, sha(feat)), flush=True)
