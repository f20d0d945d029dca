"""The frame recorder without a GPU: the layout and sizes as tests/record_ref.py states them, the ordered-key bounds on signed
zeros and on the empty set, the Q16 decode error against a bound derived from the number formats, the animation file's round
trip on reference-built frames, and the names, arities and struct layouts of the new calls across the header, the ctypes
table, the C++ mirror and the Go stub."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import record_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def test_the_layout_and_sizes():
    # F32, everything, 216 particles: 128 + 2592 -> 2720 is no multiple of 128, so the planes start at 128, 2816, 5504
    lay = rr.frame_layout(216, 1, 3, rr.F32)
    assert lay == {"m": 216, "pos": 128, "vel": 2816, "rho": 5504, "bytes": 5504 + 896}
    assert rr.frame_layout(216, 1, 0, rr.F32) == {"m": 216, "pos": 128, "vel": None, "rho": None, "bytes": 2816}
    assert rr.frame_layout(216, 1, rr.DENSITY, rr.Q16) == {"m": 216, "pos": 128, "vel": None, "rho": 1536, "bytes": 2048}
    for n, stride in ((1, 1), (216, 7), (216, 221), (1024, 3), (276, 5)):
        for fields in range(4):
            for enc in (rr.F32, rr.Q16):
                lay = rr.frame_layout(n, stride, fields, enc)
                m, w = -(-n // stride), 4 >> enc
                assert lay["m"] == m and lay["pos"] == 128 and lay["bytes"] % 128 == 0
                ends = [128 + 3 * w * m]
                if fields & 1:
                    assert lay["vel"] % 128 == 0 and 0 <= lay["vel"] - ends[-1] < 128
                    ends.append(lay["vel"] + 3 * w * m)
                if fields & 2:
                    assert lay["rho"] % 128 == 0 and 0 <= lay["rho"] - ends[-1] < 128
                    ends.append(lay["rho"] + w * m)
                assert 0 <= lay["bytes"] - ends[-1] < 128
    # a frame the reference builds has that size, says so, and pads with zeros
    x = np.arange(30, dtype=f32).reshape(10, 3)
    fr = rr.build_frame(7, x, x + 1, x[:, 0], stride=3, fields=3, dt=0.002)
    h = rr.parse_header(fr)
    assert len(fr) == h["frame_bytes"] == rr.frame_layout(10, 3, 3, rr.F32)["bytes"] == 512
    assert (h["magic"], h["header_bytes"], h["step"], h["n_particles"], h["count"], h["stride"], h["fields"], h["encoding"]) == \
        (0x464C5344, 128, 7, 10, 4, 3, 3, 0)
    assert fr[:4] == b"DSLF" and h["zero"] == bytes(24) and h["dt"] == f32(0.002) and h["finite"] == 4
    assert np.array_equal(np.frombuffer(fr, f32, 12, 128).reshape(4, 3), x[::3]) and fr[128 + 48:256] == bytes(80)
    assert np.array_equal(np.frombuffer(fr, f32, 4, 384), x[::3, 0])


def test_the_ordered_key_decides_signed_zeros_and_the_empty_set():
    v = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], f32)
    k = rr.order_key(v)
    assert np.all(np.diff(k.astype(np.int64)) > 0)  # the total order, -0 strictly below +0
    assert np.array_equal(_bits(rr.key_value(k)), _bits(v))
    for col, lo, hi in ((np.array([0.0, -0.0, 0.0], f32), 0x80000000, 0), (np.array([-0.0, -0.0], f32), 0x80000000, 0x80000000),
                        (np.array([0.0, 0.0], f32), 0, 0)):
        x = np.zeros((col.size, 3), f32)
        x[:, 1] = col
        bmin, bmax, finite = rr.bounds(x)
        assert _bits(bmin)[1] == lo and _bits(bmax)[1] == hi and finite == col.size
    # a row with one non-finite coordinate is left out whole; with none left the bounds are +inf / -inf
    x = np.array([[1, 2, 3], [np.nan, -9, 9], [4, np.inf, 0], [0, 1, 5]], f32)
    bmin, bmax, finite = rr.bounds(x)
    assert finite == 2 and list(bmin) == [0, 1, 3] and list(bmax) == [1, 2, 5]
    bmin, bmax, finite = rr.bounds(x[1:3])
    assert finite == 0 and np.all(bmin == np.inf) and np.all(bmax == -np.inf)
    # ... and Q16 against that box is all zeros (hi - lo is not finite: scale 0)
    fr = rr.build_frame(0, x[1:3], encoding=rr.Q16)
    assert not np.frombuffer(fr, np.uint16, 6, 128).any() and rr.parse_header(fr)["auto_box"] == 1


def test_q16_corners_by_hand():
    hi = f32(65535.0) * f32(2.0 ** -17)  # scale = 2^17 exactly: t = x * 2^17 without rounding
    x = np.array([-1.0, 1.0, 1000.5 * 2.0 ** -17, 1001.5 * 2.0 ** -17, 0.0, hi, np.nan, 0.25 * 2.0 ** -17, -0.0], f32)
    assert list(rr.q16(x, 0.0, hi)) == [0, 65535, 1000, 1002, 0, 65535, 0, 0, 0]
    assert not rr.q16(x, 0.25, 0.25).any() and not rr.q16(x, 0.0, np.inf).any() and not rr.q16(x, -0.0, 0.0).any()
    with np.errstate(over="ignore"):
        h = np.array([1.0e-6, 2.0 ** -25, 3.0e-8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65519.996, 65520.0, 7.0e4], f32).astype(np.float16)
    assert [hex(t) for t in h.view(np.uint16)] == ["0x11", "0x0", "0x1", "0x3c00", "0x3c02", "0x7bff", "0x7c00", "0x7c00"]


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-3.7, 12.9), (1000.0, 1000.5), (-1.0e-3, 1.0e-3)])
def test_the_q16_decode_error_is_half_a_step_plus_rounding(lo, hi):
    """For x in [lo, hi]: |decode(q16(x)) - x| <= step / 2 + slack, step = (hi - lo) / 65535.  The slack is what float32
    rounding can add, counted operation by operation with u = 2^-24 and A = max(|lo|, |hi|) (np.spacing(A) >= 2 u |v| for every
    |v| <= A, so u |v| <= spacing(A) / 2):
      encode: x - lo is off by <= spacing(2 A) / 2 = spacing(A); scale by 2 u relative (subtraction and division) and the product
              by u more, which moves t by <= 3 u 65535 ~ 0.012 of a step, before rint -- in all the rounded t may sit up to
              spacing(A) / step + 0.012 steps away from the exact one, so q's centre is off by that much: spacing(A) + 0.012 step;
      decode: step' is off by 2 u relative, q step' by u more: <= 3 u (hi - lo) <= 6 u A <= 3 spacing(A); the final sum by
              spacing(A) / 2.
    Together: slack = 5 spacing(A) + 0.02 step."""
    lo, hi = f32(lo), f32(hi)
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(lo, hi, 200000).astype(f32), np.array([lo, hi], f32)])
    x = np.clip(x, lo, hi)
    q = rr.q16(x, lo, hi)
    back = rr.q16_decode(q, lo, hi)
    step = (float(hi) - float(lo)) / 65535.0
    slack = 5.0 * float(np.spacing(f32(max(abs(lo), abs(hi))))) + 0.02 * step
    err = np.abs(back.astype(np.float64) - x.astype(np.float64)).max()
    print("lo", lo, "hi", hi, "max error", err, "bound", step / 2 + slack)
    assert err <= step / 2 + slack
    assert q.min() == 0 and q.max() == 65535


def test_the_animation_file_round_trip(tmp_path):
    from dieselfluid_amd import animation
    rng = np.random.default_rng(2)
    frames = []
    for s, n in ((0, 216), (3, 236), (6, 1)):
        x, v, d = rng.normal(0, 1, (n, 3)).astype(f32), rng.normal(0, 5, (n, 3)).astype(f32), rng.uniform(900, 1100, n).astype(f32)
        frames.append((rr.build_frame(s, x, v, d, stride=1 + s, fields=3, encoding=rr.F32 if s else rr.Q16, dt=0.001), x, v, d, 1 + s))
    path = str(tmp_path / "run.dslanim")
    with animation.AnimationWriter(path) as w:
        for f in frames:
            w.append(f[0])
        assert w.frames == 3
    raw = open(path, "rb").read()
    assert raw[:16] == b"DSLANIM\0" + struct.pack("<II", 1, 0) and len(raw) == 16 + sum(len(f[0]) for f in frames)
    back = animation.read_animation(path)
    assert back == [f[0] for f in frames]
    for buf, (_, x, v, d, stride) in zip(back, frames):
        fr = animation.decode_frame(buf)
        h = rr.parse_header(buf)
        assert fr["step"] == h["step"] and fr["count"] == -(-x.shape[0] // stride) and fr["positions"].dtype == np.float32
        if fr["encoding"] == rr.F32:
            assert np.array_equal(_bits(fr["positions"]), _bits(x[::stride])) and np.array_equal(_bits(fr["velocities"]), _bits(v[::stride]))
            assert np.array_equal(_bits(fr["densities"]), _bits(d[::stride]))
        else:  # Q16 against the frame's own bounds: half a step plus the slack of the test above
            for a in range(3):
                lo, hi = h["box_min"][a], h["box_max"][a]
                q = np.frombuffer(buf, np.uint16, 3 * fr["count"], 128).reshape(-1, 3)[:, a]
                assert np.array_equal(_bits(fr["positions"][:, a]), _bits(rr.q16_decode(q, lo, hi)))
                step = (float(hi) - float(lo)) / 65535.0
                assert np.abs(fr["positions"][:, a].astype(np.float64) - x[::stride, a]).max() <= step / 2 + 5 * float(np.spacing(max(abs(lo), abs(hi)))) + 0.02 * step
            assert np.array_equal(fr["velocities"], v[::stride].astype(np.float16).astype(f32))
    with pytest.raises(ValueError):
        animation.decode_frame(b"\0" * 200)
    bad = str(tmp_path / "bad.dslanim")
    open(bad, "wb").write(b"DSLANIM\0" + struct.pack("<II", 2, 0))
    with pytest.raises(ValueError):
        animation.read_animation(bad)


def test_the_schedule_and_the_ring_by_hand():
    r = rr.Ring(every=3, first_step=2, max_frames=3, slots=4)
    assert [s for s in range(12) if r.step(s)] == [2, 5, 8] and r.dropped == 0
    r = rr.Ring(slots=2, max_frames=4)
    assert [s for s in range(5) if r.step(s)] == [0, 1] and (r.recorded, r.dropped) == (2, 3)
    assert r.now(5) == "nomem" and r.release() == 0 and r.step(5) and r.held == [1, 5]
    assert not r.step(6) and not r.step(7) and r.dropped == 5
    assert r.release() == 1 and r.release() == 5 and r.now(8) == "ok" and r.now(8) == "invalid" and not r.step(9) and r.dropped == 5


def test_the_bindings_agree_on_the_new_names():
    from dieselfluid_amd import _lib, animation, engine
    header = open(os.path.join(ROOT, "include", "dslsph.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {"dsl_recorder_set": 2, "dsl_record_frame_bytes": 2, "dsl_record_now": 1, "dsl_record_poll": 4, "dsl_record_peek": 3,
            "dsl_record_release": 1, "dsl_record_read": 3}
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(?:int|size_t)\s+(dsl_record\w*)\s*\(([^)]*)\)", code)}
    assert {k: len(v.split(",")) for k, v in decl.items()} == want
    assert {k: len(_lib.EXPORTS[k][1]) for k in want} == want
    assert _lib.EXPORTS["dsl_record_frame_bytes"][0] is C.c_size_t
    opts = {"record_frames": 96, "record_dropped": 97, "record_ready": 98, "record_pack_ms": 99, "record_copy_ms": 100}
    for name, value in opts.items():
        assert re.search(r"\bDSL_OPT_%s\s*=\s*%d\b" % (name.upper(), value), code), name
        assert engine.SPHEngine.OPTIONS[name] == value
    # no kernel id was added
    assert re.search(r"\bDSL_K_COUNT\s*=\s*19\b", code) and re.search(r"\bDSL_K_END\s*=\s*20\b", code)
    assert re.search(r"#define\s+DSL_REC_VELOCITY\s+1\b", code) and re.search(r"#define\s+DSL_REC_DENSITY\s+2\b", code)
    assert re.search(r"\bDSL_REC_F32\s*=\s*0\b", code) and re.search(r"\bDSL_REC_Q16\s*=\s*1\b", code)
    assert (animation.REC_VELOCITY, animation.REC_DENSITY, animation.REC_F32, animation.REC_Q16) == (1, 2, 0, 1) == \
        (rr.VELOCITY, rr.DENSITY, rr.F32, rr.Q16)
    assert animation.FRAME_MAGIC == rr.MAGIC == 0x464C5344
    for name in ("set_recorder", "record_now", "record_poll", "read_frame", "peek_frame", "release_frame", "recorder_spec"):
        assert callable(getattr(engine.SPHEngine, name))
    for name in ("decode_frame", "AnimationWriter", "read_animation"):
        assert callable(getattr(animation, name))
    assert "record.hip" in _lib.UNITS
    # the structs: the header's field order, and the layout a C compiler gives it (first_step on an 8-byte boundary)
    body = re.search(r"typedef struct dsl_recorder \{(.*?)\} dsl_recorder;", code, re.S).group(1)
    names = [n.strip().split("[")[0] for decl_ in body.split(";") if decl_.strip() for n in decl_.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _lib.Recorder._fields_] == ["every", "stride", "fields", "encoding", "slots", "auto_box", "box_min",
                                                               "box_max", "first_step", "max_frames"]
    assert C.sizeof(_lib.Recorder) == 64 and _lib.Recorder.box_min.offset == 24 and _lib.Recorder.first_step.offset == 48
    # the frame header: the offsets the header's table states
    table = {"magic": 0, "header_bytes": 4, "frame_bytes": 8, "step": 16, "n_particles": 24, "count": 28, "stride": 32, "fields": 36,
             "encoding": 40, "auto_box": 44, "box_min": 48, "box_max": 60, "bounds_min": 72, "bounds_max": 84, "dt": 96, "finite": 100,
             "zero": 104}
    assert {f[0]: getattr(_lib.FrameHeader, f[0]).offset for f in _lib.FrameHeader._fields_} == table
    assert C.sizeof(_lib.FrameHeader) == 128
    for off, name in ((8, "frame_bytes"), (16, "step"), (24, "n_particles"), (28, "count"), (72, "bounds_min"), (100, "finite")):
        assert re.search(r"\b%d\s+\w+(\[3\])?\s+%s\b" % (off, name), header), name
    fr = rr.build_frame(5, np.ones((3, 3), f32), dt=0.25)
    h = _lib.FrameHeader.from_buffer_copy(fr[:128])
    assert (h.magic, h.header_bytes, h.frame_bytes, h.step, h.n_particles, h.count, h.stride, h.dt, h.finite) == (rr.MAGIC, 128, 256, 5, 3, 3, 1, 0.25, 3)
    go = open(os.path.join(ROOT, "bindings", "go", "dslsph", "dslsph.go")).read()
    for name in ["C." + k + "(" for k in want] + ["C.DSL_OPT_%s)" % k.upper() for k in opts] + [
            "C.DSL_REC_VELOCITY)", "C.DSL_REC_Q16)", "type Recorder struct", "func (e *Engine) SetRecorder(", "func (e *Engine) RecordNow(",
            "func (e *Engine) PollFrames(", "func (e *Engine) NextFrame(", "func (e *Engine) WriteTo(w io.Writer)", '"io"']:
        assert name in go, name
    for field in ("every", "stride", "fields", "encoding", "slots", "auto_box", "box_min", "box_max", "first_step", "max_frames"):
        assert "d." + field in go, field
    hpp = open(os.path.join(ROOT, "dieselfluid_amd", "host", "dieselfluid.hpp")).read()
    for name in [k + "(" for k in want if k not in ("dsl_record_frame_bytes", "dsl_record_read")] + [
            "struct Recorder", "SetRecorder(", "ClearRecorder(", "RecordNow(", "PollFrames(", "NextFrame(", "WriteAnimation("]:
        assert name in hpp, name
    for field in ("every", "stride", "fields", "encoding", "slots", "auto_box", "box_min", "box_max", "first_step", "max_frames"):
        assert "d." + field in hpp, field
