"""GPU: dsl_field_volume -- SPHField.Interpolate (sph_field.go:124-135) at every point of a regular lattice, evaluated and
left on the device.  The reference is the oracle's field_interpolate at EVERY voxel (scenes.volume_points gives the
coordinates bit for bit); the per-voxel form is also held to dsl_field_interpolate bit for bit in both math modes.

Lattices (tag: scene; origin, step, dims; share of non-zero / zero voxels by the oracle's densities):
  A   reference_scene(12), jittered_lattice(12, 0.2); (-2.3, -2.1, -1.9), (0.37, 0.41, 0.43), (13, 11, 9); 59 % / 41 %
  A2  the same scene, first and last x-planes outside the particle grid's box (+-4); (-4.6, -0.7, -0.5), 0.45, (21, 4, 3);
      43 % / 57 %
  B   dambreak_scene(16), h = 2 dx; -1.5 dx, dx, (27, 23, 19) -- odd, no multiple of a brick edge; 55 % / 45 %; also with
      jitter = 0.4
  C   dambreak_scene(16, h_over_dx=5.0), about 125 particles per cell; -h, h, (9, 9, 6); 23 % / 77 % (densities only: its
      pressures are 7 % non-zero)
Every compared volume is asserted to be at least 20 % non-zero and at least 10 % exactly zero on the oracle's densities.

FAST tolerances against the oracle: 2e-5 of max |oracle| for densities, eight times that for pressures."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

EXACT, FAST = 0, 1
TOL_RHO, TOL_P = 2e-5, 8 * 2e-5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(tag):
    """(params, positions, origin, step, dims); the params are the scene's own (copy before changing the math mode)"""
    from dieselfluid_amd import scenes
    f32 = np.float32
    if tag in ("A", "A2"):
        p, _ = scenes.reference_scene(12)
        pos = helpers.jittered_lattice(12, 0.2)
        if tag == "A":
            return p, pos, (-2.3, -2.1, -1.9), (0.37, 0.41, 0.43), (13, 11, 9)
        return p, pos, (-4.6, -0.7, -0.5), (0.45, 0.45, 0.45), (21, 4, 3)
    if tag in ("B", "Bj"):
        p, pos = scenes.dambreak_scene(16, jitter=0.4 if tag == "Bj" else 0.05)
        dx = f32(1.0 / 16)
        return p, pos, (f32(-1.5) * dx,) * 3, (dx,) * 3, (27, 23, 19)
    assert tag == "C"
    p, pos = scenes.dambreak_scene(16, h_over_dx=5.0)
    return p, pos, (-f32(p.h),) * 3, (f32(p.h),) * 3, (9, 9, 6)


def _points(tag):
    from dieselfluid_amd import scenes
    _p, _pos, origin, step, dims = _case(tag)
    return scenes.volume_points(origin, step, dims)


@functools.lru_cache(maxsize=None)
def _oracle(tag, scalar):
    """the oracle's Interpolate at every voxel, computed once; asserts the cap on what is compared"""
    p, pos, _o, _s, dims = _case(tag)
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos)
    ora.density_all()
    rho = ora.field_interpolate(_points(tag), "density")
    assert np.mean(rho != 0) >= 0.20 and np.mean(rho == 0) >= 0.10, (tag, np.mean(rho != 0), np.mean(rho == 0))
    out = rho if scalar == "densities" else ora.field_interpolate(_points(tag), "pressure")
    out.setflags(write=False)
    assert out.size == dims[0] * dims[1] * dims[2]
    return out


def _engine(tag, math_mode, bricks=None):
    from dieselfluid_amd import SPHEngine, _lib
    p0, pos, origin, step, dims = _case(tag)
    p = _lib.Params.from_buffer_copy(p0)
    p.math_mode = math_mode
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.density_all()
    if bricks is not None:
        eng.set_option("volume_bricks", bricks)
    return eng, origin, step, dims


def _interpolate(eng, pts, scalar):
    """dsl_field_interpolate at every point (it takes at most `capacity` of them per call)"""
    cap = eng.capacity
    return np.concatenate([eng.field_interpolate(pts[k:k + cap], scalar) for k in range(0, pts.shape[0], cap)])


def _same_bits(a, b):
    """bit for bit, NaN where the other is NaN"""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(_bits(np.nan_to_num(a)), _bits(np.nan_to_num(b)))


# ---- 1. EXACT: the volume is dsl_field_interpolate, and the oracle, bit for bit --------------------------------------
@pytest.mark.parametrize("scalar", ["densities", "pressures"])
@pytest.mark.parametrize("tag", ["A", "A2", "B", "Bj"])
def test_exact_volume_is_field_interpolate_and_the_oracle_bit_for_bit(tag, scalar):
    eng, origin, step, dims = _engine(tag, EXACT)
    vol = eng.field_volume(origin, step, dims, scalar)
    assert vol.shape == (dims[2], dims[1], dims[0]) and vol.dtype == np.float32
    assert np.array_equal(_bits(vol).reshape(-1), _bits(_interpolate(eng, _points(tag), scalar)))
    want = _oracle(tag, scalar)
    print(tag, scalar, "EXACT: voxels differing from the oracle:", int(np.sum(_bits(vol).reshape(-1) != _bits(want))))
    assert np.array_equal(_bits(vol).reshape(-1), _bits(want))
    eng.close()


# ---- 2. the reference's LSH neighbours, and boundary particles -------------------------------------------------------
def test_lsh_ref_volume_is_field_interpolate_bit_for_bit():
    from dieselfluid_amd import SPHEngine, scenes
    from dieselfluid_amd.engine import reference_params
    n3 = 8
    p = reference_params(n3)
    p.neigh_mode, p.math_mode = 0, EXACT  # DSL_NEIGH_LSH_REF
    eng = SPHEngine(p)
    eng.set_hash_vectors(po.default_hash_vectors(5))
    eng.upload("positions", helpers.jittered_lattice(n3, 0.25))
    eng.density_all()
    origin, step, dims = (-1.3, -1.2, -1.1), (0.37, 0.41, 0.43), (7, 6, 5)
    pts = scenes.volume_points(origin, step, dims)
    for scalar in ("densities", "pressures"):
        vol = eng.field_volume(origin, step, dims, scalar)
        want = eng.field_interpolate(pts, scalar)
        assert np.any(want != 0)
        assert _same_bits(vol, want)
    eng.set_option("volume_bricks", 1)  # (asked for, but lsh_ref runs the per-voxel form)
    assert _same_bits(eng.field_volume(origin, step, dims), eng.field_interpolate(pts))
    assert eng.get_option("volume_lds_bricks") == 0 and eng.get_option("volume_fallback_bricks") == 0
    eng.close()


@pytest.mark.parametrize("math_mode,bricks", [(EXACT, 0), (FAST, 0), (FAST, 1)])
def test_boundary_particles_volume_is_field_interpolate_bit_for_bit(math_mode, bricks):
    """boundary particles are candidates with density 0: m / 0 = Inf, Inf * 0 = NaN, exactly where dsl_field_interpolate has
    them.  (The brick form walks the same candidates in the same order with the same operations: the same bits.)"""
    from dieselfluid_amd import SPHEngine, scenes
    n3 = 8
    p, pos = scenes.reference_scene(n3)
    p.math_mode = math_mode
    t = np.arange(-1.25, 1.25 + 1e-6, 0.25, dtype=np.float32)
    u, v = np.meshgrid(t, t, indexing="ij")
    plate = np.stack([u.reshape(-1), np.full(u.size, -1.25, np.float32), v.reshape(-1)], axis=-1).astype(np.float32)
    p.capacity = n3 ** 3 + plate.shape[0]
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.density_all()
    eng.add_boundary_particles(plate)
    eng.set_option("volume_bricks", bricks)
    origin, step, dims = (-1.6, -1.7, -1.5), (0.4, 0.3, 0.5), (9, 9, 7)
    pts = scenes.volume_points(origin, step, dims)
    for scalar in ("densities", "pressures"):
        want = eng.field_interpolate(pts, scalar)
        vol = eng.field_volume(origin, step, dims, scalar)
        assert _same_bits(vol, want)
    assert np.any(np.isnan(want)) and np.any(np.isfinite(want) & (want != 0))
    eng.close()


# ---- 3. FAST, both forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bricks", [0, 1])
@pytest.mark.parametrize("tag", ["A", "B", "Bj", "C"])
def test_fast_volume_both_forms(tag, bricks):
    eng, origin, step, dims = _engine(tag, FAST, bricks)
    for scalar in ("densities",) if tag == "C" else ("densities", "pressures"):
        want = _oracle(tag, scalar)
        vol = eng.field_volume(origin, step, dims, scalar)
        err = helpers.rel_err(vol.reshape(-1), want)
        tol = TOL_RHO if scalar == "densities" else TOL_P
        print(tag, scalar, "bricks", bricks, "FAST: max |volume - oracle| / max |oracle| =", err, "tolerance", tol)
        assert err < tol
        if bricks == 0:
            assert np.array_equal(_bits(vol).reshape(-1), _bits(_interpolate(eng, _points(tag), scalar)))
        else:
            assert np.array_equal(_bits(vol), _bits(eng.field_volume(origin, step, dims, scalar)))  # no atomics in the sums
        lds, fallback = eng.get_option("volume_lds_bricks"), eng.get_option("volume_fallback_bricks")
        print(tag, "bricks", bricks, "LDS bricks", lds, "fallback bricks", fallback)
        if bricks == 0:
            assert lds == 0 and fallback == 0
        elif tag in ("B", "Bj"):
            assert lds > 0 and fallback == 0
        elif tag == "C":
            assert fallback > 0  # 125 particles per cell, a brick of 256 voxels at step = h: no image of 160 KiB holds that
    eng.close()


def test_fast_brick_form_has_the_sweep_s_bits():
    """same candidates, same order, same operations: switching the form does not change a bit"""
    eng, origin, step, dims = _engine("Bj", FAST, 1)
    a = eng.field_volume(origin, step, dims, "pressures")
    assert eng.get_option("volume_lds_bricks") > 0
    eng.set_option("volume_bricks", 0)
    assert np.array_equal(_bits(a), _bits(eng.field_volume(origin, step, dims, "pressures")))
    eng.close()
    # ... nor where the bricks inside the fluid take the global sweep (C at a quarter of its step, odd dims: 5 of 150 bricks)
    eng, origin, step, _dims = _engine("C", FAST, 1)
    step, dims = tuple(np.float32(s) / np.float32(4) for s in step), (37, 35, 21)
    a = eng.field_volume(origin, step, dims)
    fallback = eng.get_option("volume_fallback_bricks")
    print("C at step h / 4: LDS bricks", eng.get_option("volume_lds_bricks"), "fallback bricks", fallback)
    assert fallback >= 4
    eng.set_option("volume_bricks", 0)
    b = eng.field_volume(origin, step, dims)
    assert np.mean(b != 0) > 0.1 and np.array_equal(_bits(a), _bits(b))
    eng.close()


# ---- 4. dev_out ------------------------------------------------------------------------------------------------------
GUARD, SENTINEL = 64, -7.25


@pytest.mark.parametrize("math_mode,bricks", [(EXACT, 0), (FAST, 1)])
def test_dev_out_gets_the_same_bits_and_nothing_else_is_written(math_mode, bricks):
    import torch
    eng, origin, step, dims = _engine("B", math_mode, bricks)
    nvox = dims[0] * dims[1] * dims[2]
    base = eng.get_option("device_bytes")
    buf = torch.full((GUARD + nvox + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[GUARD:GUARD + nvox]
    assert eng.field_volume(origin, step, dims, dev_out=out.data_ptr()) is None
    eng.sync()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + nvox:] == SENTINEL), "written outside nx * ny * nz floats"
    assert eng.get_option("device_bytes") == base  # no array of the library's own
    # both outputs at once
    buf.fill_(SENTINEL)
    host = np.full(nvox, 3.5, dtype=np.float32)
    L, fp = eng._L, C.POINTER(C.c_float)
    o3, s3 = (C.c_float * 3)(*origin), (C.c_float * 3)(*step)
    d3 = (C.c_int32 * 3)(*dims)
    assert L.dsl_field_volume(eng._h, 3, o3, s3, d3, C.c_void_p(out.data_ptr()), host.ctypes.data_as(fp)) == 0
    both = buf.cpu().numpy()
    assert np.all(both[:GUARD] == SENTINEL) and np.all(both[GUARD + nvox:] == SENTINEL)
    assert np.array_equal(_bits(both[GUARD:GUARD + nvox]), _bits(got[GUARD:GUARD + nvox]))
    assert np.array_equal(_bits(host), _bits(got[GUARD:GUARD + nvox]))
    assert eng.get_option("device_bytes") == base
    # host_out alone: the same bits, out of the library's staging array, which is counted
    vol = eng.field_volume(origin, step, dims)
    assert np.array_equal(_bits(vol).reshape(-1), _bits(got[GUARD:GUARD + nvox]))
    grown = eng.get_option("device_bytes")
    assert grown >= base + 4 * nvox
    eng.field_volume(origin, step, (dims[0], dims[1], 3))  # a smaller volume fits in: nothing is allocated
    assert eng.get_option("device_bytes") == grown
    eng.close()


# ---- 5. the call leaves the simulation alone -------------------------------------------------------------------------
@pytest.mark.parametrize("math_mode,bricks", [(EXACT, 0), (FAST, 0), (FAST, 1)])
def test_volume_between_steps_leaves_the_simulation_alone(math_mode, bricks):
    res = []
    for with_volume in (True, False):
        eng, origin, step, dims = _engine("B", math_mode, bricks)
        eng.reset_forces()
        for _ in range(5):
            eng.wcsph_step(1)
            if with_volume:
                eng.field_volume(origin, step, dims)
            else:
                eng.field_interpolate(np.array([[0.3, 0.2, 0.1]], np.float32))
        res.append((eng.download("positions"), eng.download("velocities")))
        eng.close()
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and np.array_equal(_bits(res[0][1]), _bits(res[1][1]))


# ---- 6. refusals and bookkeeping -------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_change_nothing():
    eng, origin, step, dims = _engine("A", FAST, 1)
    L, fp = eng._L, C.POINTER(C.c_float)
    nvox = dims[0] * dims[1] * dims[2]
    host = np.zeros(nvox, dtype=np.float32)
    first = eng.field_volume(origin, step, dims)
    counters = eng.get_option("volume_lds_bricks"), eng.get_option("volume_fallback_bricks")
    bytes_before = eng.get_option("device_bytes")
    eng.timing_enable(True)
    eng.timing_reset()

    def call(buffer=3, o=origin, s=step, d=dims, out=True):
        rc = L.dsl_field_volume(eng._h, buffer, (C.c_float * 3)(*o), (C.c_float * 3)(*s), (C.c_int32 * 3)(*d), None,
                                host.ctypes.data_as(fp) if out else None)
        return rc, L.dsl_last_error(eng._h).decode()

    inf, nan = float("inf"), float("nan")
    refused = [
        (dict(buffer=0), "scalar_buffer"), (dict(buffer=2), "scalar_buffer"), (dict(buffer=7), "scalar_buffer"),
        (dict(d=(13, 0, 9)), "dims"), (dict(d=(-1, 11, 9)), "dims"),
        (dict(d=(1025, 1024, 1024)), "dims"), (dict(d=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), "dims"),
        (dict(s=(0.37, 0.0, 0.43)), "step"), (dict(s=(-0.37, 0.41, 0.43)), "step"), (dict(s=(0.37, 0.41, inf)), "step"),
        (dict(s=(nan, 0.41, 0.43)), "step"),
        (dict(o=(-2.3, nan, -1.9)), "origin"), (dict(o=(inf, -2.1, -1.9)), "origin"),
        (dict(out=False), "host_out"),
    ]
    for kwargs, word in refused:
        rc, text = call(**kwargs)
        assert rc == -1 and "dsl_field_volume" in text and word in text, (kwargs, rc, text)
    assert np.all(host == 0)
    assert eng.get_option("device_bytes") == bytes_before
    assert (eng.get_option("volume_lds_bricks"), eng.get_option("volume_fallback_bricks")) == counters
    assert eng.timing("volume")[1] == 0  # nothing was launched
    rc, _text = call(d=(1024, 1024, 1024), out=False)  # exactly 2^30 voxels pass the size check (and stop at the outputs)
    assert rc == -1 and "host_out" in _text
    # the next valid calls are unaffected, and every launch is timed under DSL_K_VOLUME
    assert call()[0] == 0
    assert np.array_equal(_bits(host), _bits(first).reshape(-1))
    eng.set_option("volume_bricks", 0)
    assert np.array_equal(_bits(eng.field_volume(origin, step, dims)), _bits(first))
    ms, launches = eng.timing("volume")
    assert launches == 2 and ms > 0.0
    eng.close()


def test_the_default_is_the_brick_form():
    """the form that measured faster at step = dx; DSL_MATH_EXACT handles hold the same option and sweep"""
    for math_mode in (FAST, EXACT):
        eng, origin, step, dims = _engine("B", math_mode)
        assert eng.get_option("volume_bricks") == 1
        eng.field_volume(origin, step, dims)
        assert (eng.get_option("volume_lds_bricks") > 0) == (math_mode == FAST)
        eng.close()


def test_a_slab_handle_is_refused():
    eng, origin, step, dims = _engine("A", FAST)
    eng.slab_config(0, -0.5, 0.5)
    host = np.zeros(dims[0] * dims[1] * dims[2], dtype=np.float32)
    rc = eng._L.dsl_field_volume(eng._h, 3, (C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*dims), None,
                                 host.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == -4 and "slab" in eng._L.dsl_last_error(eng._h).decode()
    assert np.all(host == 0)
    eng.close()
