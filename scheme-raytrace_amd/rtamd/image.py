"""Image textures on the host: the NumPy restatement of the library's lookup
and u, v rules (include/rt.h, "image textures"; t:image-texture,
texture.scm:36-50 with repairs R4 and R5 of DESIGN.md §2), and a PPM reader,
so that what ``Renderer.save_as_ppm`` writes can be used as a texture.

An image is ``nx * ny`` texels of 3 bytes, row 0 first, row 0 the top (v = 1).
"""
import numpy as np


def as_texels(data, nx, ny):
    """``data`` (bytes or a uint8 array of nx*ny*3) as a flat uint8 array."""
    nx, ny = int(nx), int(ny)
    if nx < 1 or ny < 1:
        raise ValueError("image-texture: nx and ny must be at least 1")
    if isinstance(data, (bytes, bytearray, memoryview)):
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
    else:
        arr = np.asarray(data)
        if arr.dtype != np.uint8:
            raise TypeError("image-texture: data must be bytes or a uint8 array (got %s)" % arr.dtype)
        arr = np.ascontiguousarray(arr).ravel()
    if arr.size != nx * ny * 3:
        raise ValueError("image-texture: data must hold nx*ny*3 = %d bytes (got %d)" % (nx * ny * 3, arr.size))
    return arr


def texel_index(nx, ny, u, v):
    """The texel (ii, jj) a hit with (u, v) reads: i = u*nx, j = (1-v)*ny - 0.001, each clamped to
    [0, n-1] the way the reference clamps it (a NaN lands on 0), then floored (R4)."""
    u = np.asarray(u, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        i = u * float(nx)
        j = (1.0 - v) * float(ny) - 0.001
        i = np.where(i >= 0.0, i, 0.0)
        j = np.where(j >= 0.0, j, 0.0)
        i = np.where(i > float(nx - 1), float(nx - 1), i)
        j = np.where(j > float(ny - 1), float(ny - 1), j)
    return np.floor(i).astype(np.int64), np.floor(j).astype(np.int64)


def lookup(data, nx, ny, u, v):
    """The texture's value at (u, v): arrays in, (..., 3) float64 out, byte / 255.0 per channel."""
    tex = as_texels(data, nx, ny).reshape(ny, nx, 3)
    ii, jj = texel_index(nx, ny, u, v)
    return tex[jj, ii].astype(np.float64) / 255.0


def rect_uv(a, b, a0, a1, b0, b1):
    """A rect hit's (u, v) from its in-plane coordinates (XY: x, y; XZ: x, z; YZ: y, z) on the
    instance-local ray, geometry.scm:388-389, 407-408, 426-427."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return (a - float(a0)) / (float(a1) - float(a0)), (b - float(b0)) / (float(b1) - float(b0))


def sphere_uv(n):
    """A sphere hit's (u, v) from its unit normal n = (p - centre(time)) * (1 / radius), (..., 3) (R5)."""
    n = np.asarray(n, dtype=np.float64)
    phi = np.arctan2(n[..., 2], n[..., 0])
    y = n[..., 1]
    y = np.where(y < -1.0, -1.0, np.where(y > 1.0, 1.0, y))
    theta = np.arcsin(y)
    return 1.0 - (phi + np.pi) / (2.0 * np.pi), (theta + np.pi / 2.0) / np.pi


def _ppm_tokens(buf, pos, count):
    """``count`` whitespace-separated header tokens from buf[pos:], skipping # comments; returns
    (tokens, the position just after the last token)."""
    out = []
    n = len(buf)
    while len(out) < count:
        while pos < n and buf[pos:pos + 1].isspace():
            pos += 1
        if pos >= n:
            raise ValueError("read_ppm: truncated header")
        if buf[pos:pos + 1] == b"#":
            while pos < n and buf[pos:pos + 1] not in (b"\n", b"\r"):
                pos += 1
            continue
        start = pos
        while pos < n and not buf[pos:pos + 1].isspace() and buf[pos:pos + 1] != b"#":
            pos += 1
        out.append(buf[start:pos])
    return out, pos


def read_ppm(path):
    """A P3 or P6 file with maxval 255 (# comments allowed) -> (data, nx, ny): data a uint8 array of
    nx*ny*3, rows in file order (top row first), as image textures take them."""
    with open(path, "rb") as f:
        buf = f.read()
    (magic, sx, sy, smax), pos = _ppm_tokens(buf, 0, 4)
    if magic not in (b"P3", b"P6"):
        raise ValueError("read_ppm: not a P3 / P6 file (%r)" % magic)
    nx, ny, maxval = int(sx), int(sy), int(smax)
    if nx < 1 or ny < 1:
        raise ValueError("read_ppm: bad image size %d x %d" % (nx, ny))
    if maxval != 255:
        raise ValueError("read_ppm: maxval must be 255 (got %d)" % maxval)
    need = nx * ny * 3
    if magic == b"P6":
        pos += 1                                    # the single whitespace byte after maxval
        if len(buf) - pos < need:
            raise ValueError("read_ppm: truncated raster")
        data = np.frombuffer(buf, dtype=np.uint8, count=need, offset=pos).copy()
    else:
        body = b"\n".join(line.split(b"#", 1)[0] for line in buf[pos:].splitlines())
        vals = np.array(body.split(), dtype=np.int64)
        if vals.size < need:
            raise ValueError("read_ppm: truncated raster")
        vals = vals[:need]
        if vals.min() < 0 or vals.max() > 255:
            raise ValueError("read_ppm: sample outside 0..255")
        data = vals.astype(np.uint8)
    return data, nx, ny
