#!/usr/bin/env python3
"""Per-kernel register / spill / LDS / scratch figures from the device
assembly (make -C scheme-raytrace_amd/csrc asm -> rt_kernels.s, rt_frame.s).
usage: python tools/kernel_regs.py [file.s ...] [name-filter]   (default: both files)
The last column is a hash of the kernel's instruction text with the function-numbered local labels
(.LBB<n>_, .Lfunc_end<n>, .Lpost_getpc<n>, ...) normalised, so two builds' kernels compare whatever else the files hold."""
import hashlib
import re
import sys


def text_hashes(s):
    """kernel name -> hash of its body (label line to .Lfunc_end), local label numbers dropped"""
    out = {}
    for m in re.finditer(r"^(\w+):.*?\n(.*?)^\.Lfunc_end\d+:", s, re.M | re.S):
        body = re.sub(r"\.L(BB|func_begin|func_end|JTI|tmp|post_getpc)\d+", r".L\1", m.group(2))
        body = "\n".join(ln.split(";")[0].rstrip() for ln in body.splitlines())      # comments name the labels too
        out[m.group(1)] = hashlib.sha1(body.encode()).hexdigest()[:12]
    return out


def kernels(path):
    s = open(path).read()
    meta = s[s.index("amdhsa.kernels:"):]
    out = {}
    hashes = text_hashes(s[:s.index("amdhsa.kernels:")])
    for blk in re.split(r"\n  - ", meta)[1:]:
        m = re.search(r"^    \.name:\s+(\S+)", blk, re.M)
        if not m:
            continue
        f = {k: int(re.search(r"^    \.%s:\s+(\d+)" % k, blk, re.M).group(1))
             for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
                       "group_segment_fixed_size", "private_segment_fixed_size")
             if re.search(r"^    \.%s:" % k, blk, re.M)}
        f["text"] = hashes.get(m.group(1), "-")
        out[m.group(1)] = f
    return out


if __name__ == "__main__":
    paths = [a for a in sys.argv[1:] if a.endswith(".s")]
    flt = "".join([a for a in sys.argv[1:] if not a.endswith(".s")][:1])
    found = {}
    for path in paths or ["scheme-raytrace_amd/csrc/rt_kernels.s", "scheme-raytrace_amd/csrc/rt_frame.s"]:
        found.update(kernels(path))
    for name, f in sorted(found.items()):
        if flt in name:
            print("%-90s vgpr %3d agpr %3d sgpr %3d spill %3d+%d lds %6d scratch %4d text %s" % (
                name[:90], f.get("vgpr_count", 0), f.get("agpr_count", 0), f.get("sgpr_count", 0),
                f.get("vgpr_spill_count", 0), f.get("sgpr_spill_count", 0),
                f.get("group_segment_fixed_size", 0), f.get("private_segment_fixed_size", 0), f["text"]))
