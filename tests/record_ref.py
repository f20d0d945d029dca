"""The frame recorder's rule (include/dslsph.h: dsl_recorder_set), restated in numpy operation for operation: the frame's
layout, the bounds by the ordered key, the Q16 and float16 encodings, the header, the schedule and the ring.  Every float
operation is float32 and rounded once, as the kernels' are; minimum, maximum and a count do not depend on the order of a
reduction.  The GPU tests hold the library to this bit for bit."""
import struct

import numpy as np

f32 = np.float32
MAGIC = 0x464C5344  # "DSLF"
HEADER = 128
VELOCITY, DENSITY = 1, 2
F32, Q16 = 0, 1


def up128(v: int) -> int:
    return (v + 127) & ~127


def frame_layout(n: int, stride: int, fields: int, encoding: int) -> dict:
    """count M and the planes' byte offsets (None: no such plane); bytes = the end of the last plane rounded up to 128"""
    m = (n + stride - 1) // stride
    w = 2 if encoding == Q16 else 4
    at = HEADER
    out = {"m": m, "pos": at, "vel": None, "rho": None}
    at = up128(at + 3 * w * m)
    if fields & VELOCITY:
        out["vel"] = at
        at = up128(at + 3 * w * m)
    if fields & DENSITY:
        out["rho"] = at
        at = up128(at + w * m)
    out["bytes"] = at
    return out


def order_key(x) -> np.ndarray:
    """the total order on float32 bits: bits ^ (bits >> 31 ? 0xffffffff : 0x80000000), so -0 lies below +0"""
    b = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    return b ^ np.where(b >> 31 != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def key_value(k) -> np.ndarray:
    k = np.asarray(k, dtype=np.uint32)
    return (k ^ np.where(k >> 31 != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(f32)


def bounds(pos):
    """(bounds_min, bounds_max, finite) over the rows whose three coordinates are finite; +inf / -inf with none"""
    pos = np.ascontiguousarray(pos, dtype=f32).reshape(-1, 3)
    ok = np.isfinite(pos).all(axis=1)
    finite = int(ok.sum())
    if finite == 0:
        return np.full(3, np.inf, f32), np.full(3, -np.inf, f32), 0
    k = order_key(pos[ok]).reshape(-1, 3)
    return key_value(k.min(axis=0)), key_value(k.max(axis=0)), finite


def q16(x, lo, hi) -> np.ndarray:
    """one axis: scale = 65535 / (hi - lo) when hi - lo is finite and > 0, else 0; t = (x - lo) * scale; r = rint(t);
    q = r >= 65535 ? 65535 : (r > 0 ? r : 0) -- a NaN falls to 0"""
    x, lo, hi = np.asarray(x, dtype=f32), f32(lo), f32(hi)
    with np.errstate(all="ignore"):
        w = f32(hi - lo)
        scale = f32(f32(65535.0) / w) if np.isfinite(w) and w > 0 else f32(0.0)
        r = np.rint((x - lo).astype(f32) * scale).astype(f32)
        q = np.where(r >= 65535.0, 65535.0, np.where(r > 0.0, r, 0.0))
    return q.astype(np.uint16)


def q16_decode(q, lo, hi) -> np.ndarray:
    """what a reader does: lo + q * ((hi - lo) / 65535), float32"""
    lo, hi = f32(lo), f32(hi)
    with np.errstate(all="ignore"):
        step = f32(f32(hi - lo) / f32(65535.0))
        return (lo + np.asarray(q).astype(f32) * step).astype(f32)


def build_frame(step, positions, velocities=None, densities=None, stride=1, fields=0, encoding=F32, box=None, dt=0.0) -> bytes:
    """the frame of a state in host order (fluid particles only); box None with Q16: the frame's own bounds (auto_box)"""
    pos = np.ascontiguousarray(positions, dtype=f32).reshape(-1, 3)
    n = pos.shape[0]
    lay = frame_layout(n, stride, fields, encoding)
    cap = pos[::stride]
    assert cap.shape[0] == lay["m"]
    bmin, bmax, finite = bounds(cap)
    auto = 1 if (encoding == Q16 and box is None) else 0
    if encoding == Q16:
        lo, hi = (bmin, bmax) if box is None else (np.asarray(box[0], f32), np.asarray(box[1], f32))
    else:
        lo, hi = np.zeros(3, f32), np.zeros(3, f32)
    out = bytearray(lay["bytes"])
    struct.pack_into("<IIQqiiiiii", out, 0, MAGIC, HEADER, lay["bytes"], int(step), n, lay["m"], stride, fields, encoding, auto)
    out[48:60], out[60:72] = lo.astype(f32).tobytes(), hi.astype(f32).tobytes()
    out[72:84], out[84:96] = bmin.tobytes(), bmax.tobytes()
    struct.pack_into("<fi", out, 96, float(f32(dt)), finite)

    def put(at, arr):
        raw = np.ascontiguousarray(arr).tobytes()
        out[at:at + len(raw)] = raw

    if encoding == Q16:
        put(lay["pos"], np.stack([q16(cap[:, a], lo[a], hi[a]) for a in range(3)], axis=1))
    else:
        put(lay["pos"], cap)
    with np.errstate(over="ignore"):
        if fields & VELOCITY:
            v = np.ascontiguousarray(velocities, dtype=f32).reshape(-1, 3)[::stride]
            put(lay["vel"], v.astype(np.float16) if encoding == Q16 else v)
        if fields & DENSITY:
            d = np.ascontiguousarray(densities, dtype=f32).reshape(-1)[::stride]
            put(lay["rho"], d.astype(np.float16) if encoding == Q16 else d)
    return bytes(out)


def parse_header(buf) -> dict:
    v = struct.unpack_from("<IIQqiiiiii", buf, 0)
    names = ("magic", "header_bytes", "frame_bytes", "step", "n_particles", "count", "stride", "fields", "encoding", "auto_box")
    h = dict(zip(names, v))
    for name, at in (("box_min", 48), ("box_max", 60), ("bounds_min", 72), ("bounds_max", 84)):
        h[name] = np.frombuffer(buf, dtype=f32, count=3, offset=at).copy()
    h["dt"], h["finite"] = struct.unpack_from("<fi", buf, 96)
    h["zero"] = bytes(buf[104:128])
    return h


class Ring:
    """the schedule and the ring: step(s) at the top of step s, now() for dsl_record_now, release() for the host's call"""

    def __init__(self, every=1, first_step=0, max_frames=0, slots=4):
        self.every, self.first_step, self.max_frames, self.slots = every, first_step, max_frames, slots
        self.recorded = self.dropped = 0
        self.held = []  # the steps of the unreleased frames, oldest first

    def due(self, s: int) -> bool:
        return s >= self.first_step and (s - self.first_step) % self.every == 0 and (self.max_frames == 0 or self.recorded < self.max_frames)

    def step(self, s: int) -> bool:
        if not self.due(s):
            return False
        if len(self.held) >= self.slots:
            self.dropped += 1  # dropped whole, counted, not a frame
            return False
        self.held.append(s)
        self.recorded += 1
        return True

    def now(self, s: int) -> str:
        if self.max_frames and self.recorded >= self.max_frames:
            return "invalid"
        if len(self.held) >= self.slots:
            return "nomem"
        self.held.append(s)
        self.recorded += 1
        return "ok"

    def release(self) -> int:
        return self.held.pop(0)
