"""GPU: dsl_mesh_distance_volume (include/dslsph.h; csrc/sdf.hip) against tests/sdf_ref.py, the numpy float32 restatement of
its build-defined rule.  The minimum over the triangles and the parity of the crossings depend on no order, and the rule is
the same in both math modes: every check is an equality, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import sdf_cases as sc

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = 0, 1
GUARD, SENTINEL = 256, 1234.5
INF = float("inf")
# brick edges in every axis (8 x 8 x 4 voxels), a lattice of one whole brick, rows of one voxel, a lattice thinner than a brick
ALL_DIMS = [sc.DIMS, (9, 9, 5), (8, 8, 4), (1, 9, 9), (6, 2, 1)]
# every brick lists everything; a narrow band (3 steps); a band thinner than a voxel (step / 2)
BANDS = [INF, 3 * sc.STEP, sc.STEP / 2]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _engine(math_mode=FAST, n3=12, skin=0.0):
    from dieselfluid_amd import SPHEngine, scenes
    p, pos = scenes.dambreak_scene(n3, math_mode=math_mode)
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.reset_forces()
    if skin:
        eng.set_option("skin", skin)
    return eng


def _dev_volume(eng, name, dims, band, unsigned, x0=0.0):
    """the volume through a guarded device buffer: (volume (nz, ny, nx), the device tensor)"""
    import torch
    n = dims[0] * dims[1] * dims[2]
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.mesh_distance_volume(sc.mesh(name), sc.origin(x0), sc.STEP, dims, band=band, unsigned=unsigned, dev_out=buf[GUARD:].data_ptr())
    eng.sync()
    got = buf.cpu().numpy()
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + n:] == SENTINEL), "written outside the lattice"
    return got[GUARD:GUARD + n].reshape(dims[2], dims[1], dims[0]).copy(), buf


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("name,x0", [("box", 0.0), ("box", 0.03), ("triangle", 0.0), ("ico1", 0.0), ("ico3", 0.0), ("degenerate", 0.0)])
def test_volume_equals_the_reference_bit_for_bit(name, x0, math_mode):
    """ico3: 1280 triangles, five LDS chunks of 256 in the bricks of band = +inf.  The other meshes on every lattice."""
    eng = _engine(math_mode)
    many = name in ("box", "triangle", "ico1") and x0 == 0.0
    for dims in (ALL_DIMS if many else ALL_DIMS[:1]):
        for band in BANDS:
            for unsigned in (False, True):
                want = sc.volume(name, dims, x0, band, unsigned)
                got, _buf = _dev_volume(eng, name, dims, band, unsigned, x0)
                diff = np.flatnonzero(_bits(got) != _bits(want))
                assert diff.size == 0, (name, dims, band, unsigned, diff[:8], got.reshape(-1)[diff[:8]], want.reshape(-1)[diff[:8]])
                if band != INF:  # far voxels hold exactly the band
                    assert np.any(np.abs(got) == f32(band)) or min(dims) == 1
                if dims == sc.DIMS and band == INF:  # every brick lists every triangle
                    assert eng.get_option("sdf_visits") == sc.mesh(name).shape[0] * want.size
    eng.close()


def test_host_out_dev_out_both_and_a_second_call():
    import torch
    eng = _engine()
    want = sc.volume("ico1", band=0.3)
    args = (sc.mesh("ico1"), sc.origin(), sc.STEP, sc.DIMS)
    bytes0 = eng.get_option("device_bytes")
    host = eng.mesh_distance_volume(*args, band=0.3)
    assert np.array_equal(_bits(host), _bits(want))
    grown = eng.get_option("device_bytes") - bytes0
    assert grown >= want.size * 4  # the library's own staging array (and its lists and marks) are counted
    assert np.array_equal(_bits(eng.mesh_distance_volume(*args, band=0.3)), _bits(want))  # a second call: the same bytes
    assert eng.get_option("device_bytes") - bytes0 == grown  # ... and nothing more allocated
    dev, _buf = _dev_volume(eng, "ico1", sc.DIMS, 0.3, False)
    assert np.array_equal(_bits(dev), _bits(want))
    # both outputs in one call
    v = np.ascontiguousarray(sc.mesh("ico1")).reshape(-1)
    o, s, d = eng._lattice(sc.origin(), sc.STEP, sc.DIMS)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    buf = torch.zeros(want.size, dtype=torch.float32, device="cuda")
    out = np.zeros(want.size, dtype=f32)
    rc = eng._L.dsl_mesh_distance_volume(eng._h, fp(v), v.size // 9, fp(o), fp(s), d.ctypes.data_as(C.POINTER(C.c_int32)),
                                         C.c_float(0.3), 0, C.c_void_p(buf.data_ptr()), fp(out))
    assert rc == 0
    assert np.array_equal(_bits(out), _bits(want).reshape(-1)) and np.array_equal(_bits(buf.cpu().numpy()), _bits(want).reshape(-1))
    eng.close()


def test_round_trip_the_zero_surface_of_a_sphere_is_closed():
    """dsl_surface_extract_indexed of the icosphere's signed volume at iso 0: every edge is used twice, by vertex id, and
    V - E + F = 2."""
    import torch
    eng = _engine()
    vol, buf = _dev_volume(eng, "ico2", sc.DIMS, INF, False)
    assert (vol < 0).sum() == sc.inside("ico2").sum() >= 100
    dvol = buf[GUARD:]
    V, T = eng.surface_extract_indexed(dvol.data_ptr(), sc.origin(), sc.STEP, sc.DIMS, 0.0)
    assert V > 0 and T > 0
    pos = torch.zeros(3 * V, dtype=torch.float32, device="cuda")
    nrm = torch.zeros(3 * V, dtype=torch.float32, device="cuda")
    idx = torch.zeros(3 * T, dtype=torch.int32, device="cuda")
    assert eng.surface_extract_indexed(dvol.data_ptr(), sc.origin(), sc.STEP, sc.DIMS, 0.0, dev_positions=pos.data_ptr(),
                                       dev_normals=nrm.data_ptr(), cap_vertices=V, dev_indices=idx.data_ptr(), cap_triangles=T) == (V, T)
    eng.sync()
    tri = idx.cpu().numpy().reshape(T, 3).astype(np.int64)
    edges = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    uniq, counts = np.unique(edges, axis=0, return_counts=True)
    assert np.all(counts == 2)
    assert V - uniq.shape[0] + T == 2
    # the surface lies where the mesh is: within a voxel's diagonal of the sphere of radius 0.4 around (0.85, 0.8, 0.45)
    r = np.linalg.norm(pos.cpu().numpy().reshape(V, 3).astype(np.float64) - np.array([0.85, 0.8, 0.45]), axis=1)
    assert np.all(np.abs(r - 0.4) < 0.05)
    eng.close()


def test_refusals_leave_the_output_untouched_and_timing_counts_every_launch():
    import torch
    eng = _engine()
    n = sc.DIMS[0] * sc.DIMS[1] * sc.DIMS[2]
    buf = torch.full((n,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    v = np.ascontiguousarray(sc.mesh("ico1")).reshape(-1)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def call(verts=v, T=None, origin=sc.origin(), step=(sc.STEP,) * 3, dims=sc.DIMS, band=0.3, flags=0, dev=True, host=None):
        T = v.size // 9 if T is None else T
        o = (C.c_float * 3)(*origin) if origin is not None else None
        s = (C.c_float * 3)(*step) if step is not None else None
        d = (C.c_int32 * 3)(*dims) if dims is not None else None
        return eng._L.dsl_mesh_distance_volume(eng._h, fp(verts) if verts is not None else None, T, o, s, d, C.c_float(band), flags,
                                               C.c_void_p(buf.data_ptr()) if dev else None, host)

    bad = [dict(T=0), dict(verts=None), dict(origin=None), dict(step=None), dict(dims=None), dict(dev=False),
           dict(step=(0.1, 0.0, 0.1)), dict(step=(0.1, -0.1, 0.1)), dict(step=(0.1, float("nan"), 0.1)), dict(dims=(18, 0, 10)),
           dict(dims=(2048, 1024, 1024)), dict(band=0.0), dict(band=-1.0), dict(band=float("nan")), dict(flags=2),
           dict(origin=(0.0, float("inf"), 0.0))]
    for kw in bad:
        assert call(**kw) == -1, kw  # DSL_ERR_INVALID
        assert b"dsl_mesh_distance_volume" in eng._L.dsl_last_error(eng._h), kw
    eng.sync()
    assert np.all(buf.cpu().numpy() == SENTINEL)
    assert eng.timing("sdf") == (0.0, 0)
    # a valid call: prep, brick count, scan (one entry), brick fill, distance, sweep, sign
    eng.timing_enable(1)
    assert call(band=INF) == 0
    eng.sync()
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(sc.volume("ico1")).reshape(-1))
    ms, launches = eng.timing("sdf")
    assert launches == 7 and ms > 0
    nb = 3 * 3 * 3
    assert eng.get_option("sdf_active_bricks") == nb and eng.get_option("sdf_visits") == 80 * n  # band = +inf: every pair
    assert eng.get_option("sdf_distance_ms") > 0 and eng.get_option("sdf_sign_ms") > 0
    eng.timing_reset()
    assert call(band=sc.STEP / 2, flags=1) == 0
    assert eng.timing("sdf")[1] == 5 and eng.get_option("sdf_sign_ms") == 0  # unsigned: no sweep, no sign
    assert 1 <= eng.get_option("sdf_active_bricks") <= nb and eng.get_option("sdf_visits") < 80 * n
    eng.close()


def test_steps_with_a_volume_call_in_between_are_the_steps_without_it():
    """the call reads no particle state and does not settle a live skin episode: five FAST steps with skin lists keep their
    positions bit for bit and their rebuild count"""
    a, b = _engine(FAST, 16, skin=0.07), _engine(FAST, 16, skin=0.07)
    a.wcsph_step(2)
    assert np.array_equal(_bits(a.mesh_distance_volume(sc.mesh("ico1"), sc.origin(), sc.STEP, sc.DIMS)), _bits(sc.volume("ico1")))
    a.wcsph_step(3)
    b.wcsph_step(5)
    assert np.array_equal(_bits(a.download("positions")), _bits(b.download("positions")))
    assert a.get_option("skin_steps") == b.get_option("skin_steps") > 0
    assert a.get_option("skin_rebuilds") == b.get_option("skin_rebuilds")
    a.close()
    b.close()


def test_a_slab_handle_computes_the_same_volume():
    eng = _engine()
    eng.slab_config(0, -1.0, 0.5)
    got = eng.mesh_distance_volume(sc.mesh("box"), sc.origin(), sc.STEP, sc.DIMS, band=0.3)
    assert np.array_equal(_bits(got), _bits(sc.volume("box", band=0.3)))
    eng.close()
