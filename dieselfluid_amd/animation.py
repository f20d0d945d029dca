"""Fluid Animation Export: the frames a recorder packs on the device (include/dslsph.h: dsl_recorder_set; SPHEngine.read_frame)
decoded, and a file of them.  The file is a 16-byte header -- "DSLANIM\\0", u32 version 1, u32 zero -- and then the frames
back to back, exactly as the library wrote them; each finds the next through its frame_bytes.  No GPU is needed to read one."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from ._lib import FrameHeader

FRAME_MAGIC = 0x464C5344  # "DSLF"
FILE_MAGIC = b"DSLANIM\0"
FILE_VERSION = 1
REC_VELOCITY, REC_DENSITY = 1, 2
REC_F32, REC_Q16 = 0, 1


def _up128(v: int) -> int:
    return (v + 127) & ~127


def frame_header(buf) -> FrameHeader:
    """the 128-byte header of a frame, checked: magic, header size, and a frame_bytes the buffer holds"""
    mv = memoryview(buf).cast("B")
    if len(mv) < C.sizeof(FrameHeader):
        raise ValueError("a frame starts with a 128-byte header")
    h = FrameHeader.from_buffer_copy(mv[:C.sizeof(FrameHeader)])
    if h.magic != FRAME_MAGIC or h.header_bytes != 128:
        raise ValueError("not a recorded frame (magic / header size)")
    if h.frame_bytes > len(mv) or h.count < 0 or h.stride < 1 or h.encoding not in (REC_F32, REC_Q16):
        raise ValueError("the frame's header does not fit its buffer")
    return h


def decode_frame(buf) -> dict:
    """a frame as float32 arrays: positions (M, 3), velocities (M, 3) and densities (M,) where recorded, entry m the particle
    with host index m * stride; Q16 positions decoded as lo + q * ((hi - lo) / 65535) against the header's box, float16 planes
    widened.  The header's fields come along under their names."""
    h = frame_header(buf)
    raw = np.frombuffer(memoryview(buf).cast("B"), dtype=np.uint8, count=h.frame_bytes)
    m, q = int(h.count), h.encoding == REC_Q16
    w = 2 if q else 4
    out = {"step": int(h.step), "n_particles": int(h.n_particles), "count": m, "stride": int(h.stride), "fields": int(h.fields),
           "encoding": int(h.encoding), "auto_box": int(h.auto_box), "dt": float(h.dt), "finite": int(h.finite),
           "frame_bytes": int(h.frame_bytes)}
    for name in ("box_min", "box_max", "bounds_min", "bounds_max"):
        out[name] = np.array(getattr(h, name)[:], dtype=np.float32)
    at = 128

    def plane(comps, dtype):
        nonlocal at
        size = comps * w * m
        if at + size > h.frame_bytes:
            raise ValueError("the frame's planes do not fit frame_bytes")
        a = raw[at:at + size].view(dtype).reshape((m, comps) if comps == 3 else (m,))
        at = _up128(at + size)
        return a

    if q:
        lo, hi = out["box_min"], out["box_max"]
        with np.errstate(all="ignore"):
            step = ((hi - lo).astype(np.float32) / np.float32(65535.0)).astype(np.float32)
            out["positions"] = (lo + plane(3, np.uint16).astype(np.float32) * step).astype(np.float32)
    else:
        out["positions"] = plane(3, np.float32).copy()
    if h.fields & REC_VELOCITY:
        out["velocities"] = plane(3, np.float16 if q else np.float32).astype(np.float32)
    if h.fields & REC_DENSITY:
        out["densities"] = plane(1, np.float16 if q else np.float32).astype(np.float32)
    return out


class AnimationWriter:
    """AnimationWriter(path).append(frame) ...  close(): the file header, then every frame as it is"""

    def __init__(self, path):
        self._f = open(path, "wb")
        self._f.write(FILE_MAGIC + struct.pack("<II", FILE_VERSION, 0))
        self.frames = 0

    def append(self, frame):
        h = frame_header(frame)
        self._f.write(memoryview(frame).cast("B")[:h.frame_bytes])
        self.frames += 1

    def close(self):
        if self._f:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def read_animation(path) -> list:
    """the frames of a file, as bytes each (decode_frame reads one)"""
    data = open(path, "rb").read()
    if len(data) < 16 or data[:8] != FILE_MAGIC or struct.unpack_from("<II", data, 8) != (FILE_VERSION, 0):
        raise ValueError("not an animation file (header)")
    frames, at, mv = [], 16, memoryview(data)
    while at < len(data):
        h = frame_header(mv[at:])
        frames.append(bytes(mv[at:at + h.frame_bytes]))
        at += h.frame_bytes
    return frames
