"""GPU: dsl_surface_extract and dsl_field_surface -- the iso-surface triangles of a volume on dsl_field_volume's lattice,
marching tetrahedra (include/dslsph.h has the rule).  The reference is tests/surface_ref.py, a numpy restatement of the rule
that derives its own windings; vertices are compared bit for bit up to a rotation of each triangle (zero-area triangles as
vertex multisets), in the product's order; normals bit for bit against the normal rule applied to the device's vertices.

Volumes: the 256 corner patterns of one cube; lattice B of test_gpu_volume.py (dambreak_scene(16), 27 x 23 x 19 at step dx,
also with jitter 0.4), whose device volume is downloaded and handed to the reference; analytic volumes for the shapes."""
import ctypes as C
import functools

import numpy as np
import pytest

import surface_ref as ref

pytestmark = pytest.mark.gpu

EXACT, FAST = 0, 1
GUARD, SENTINEL = 64, -7.25


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(tag):
    """lattice B of test_gpu_volume.py: (params, positions, origin, step, dims)"""
    from dieselfluid_amd import scenes
    f32 = np.float32
    p, pos = scenes.dambreak_scene(16, jitter=0.4 if tag == "Bj" else 0.05)
    dx = f32(1.0 / 16)
    return p, pos, (f32(-1.5) * dx,) * 3, (dx,) * 3, (27, 23, 19)


def _engine(tag="B", math_mode=FAST, density=True):
    from dieselfluid_amd import SPHEngine, _lib
    p0, pos, origin, step, dims = _case(tag)
    p = _lib.Params.from_buffer_copy(p0)
    p.math_mode = math_mode
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    if density:
        eng.density_all()
    return eng, origin, step, dims


def _iso(tag="B"):
    """rho0 / 2"""
    return np.float32(_case(tag)[0].ref_density) / np.float32(2)


def _device(vol):
    import torch
    return torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32).reshape(-1)).cuda()


def _extract(eng, dvol, origin, step, dims, iso, cap=None, normals=True):
    """(T, vertices (min(T, cap), 3, 3), normals) through guarded device buffers: nothing outside 9 * min(T, cap) and
    3 * min(T, cap) floats may change.  cap = None: a counting call first, then exactly T."""
    import torch
    if cap is None:
        cap = eng.surface_extract(dvol.data_ptr(), origin, step, dims, iso)
    vbuf = torch.full((GUARD + 9 * cap + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    nbuf = torch.full((GUARD + 3 * cap + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    T = eng.surface_extract(dvol.data_ptr(), origin, step, dims, iso, dev_vertices=vbuf[GUARD:].data_ptr(),
                            dev_normals=nbuf[GUARD:].data_ptr() if normals else None, cap=cap)
    eng.sync()
    n = min(T, cap)
    v, nr = vbuf.cpu().numpy(), nbuf.cpu().numpy()
    assert np.all(v[:GUARD] == SENTINEL) and np.all(v[GUARD + 9 * n:] == SENTINEL), "vertices written outside the first min(T, cap)"
    assert np.all(nr[:GUARD] == SENTINEL) and np.all(nr[GUARD + (3 * n if normals else 0):] == SENTINEL)
    return T, v[GUARD:GUARD + 9 * n].reshape(n, 3, 3).copy(), nr[GUARD:GUARD + 3 * n].reshape(n, 3).copy()


def _active_bricks(vol, dims, iso):
    """bricks of 8 x 8 x 4 cubes with at least one triangle, by the reference's counts"""
    nx, ny, nz = dims
    counts = ref.cube_counts(np.asarray(vol).ravel(), dims, iso).reshape(nz - 1, ny - 1, nx - 1)
    bz, by, bx = -(-(nz - 1) // 4), -(-(ny - 1) // 8), -(-(nx - 1) // 8)
    padded = np.zeros((4 * bz, 8 * by, 8 * bx), dtype=np.int64)
    padded[:nz - 1, :ny - 1, :nx - 1] = counts
    return int(np.sum(padded.reshape(bz, 4, by, 8, bx, 8).sum(axis=(1, 3, 5)) > 0))


def _check(eng, vol, origin, step, dims, iso):
    """the device against the reference on one host volume: count, vertices, order, normals, active bricks"""
    want, _wn = ref.extract(vol, origin, step, dims, iso)
    T, verts, norms = _extract(eng, _device(vol), origin, step, dims, iso)
    assert T == want.shape[0], (T, want.shape[0])
    assert ref.same_triangles(verts, want)
    assert np.array_equal(_bits(norms), _bits(ref.normals(verts)))
    assert eng.get_option("surface_triangles") == T and eng.get_option("surface_active_bricks") == _active_bricks(vol, dims, iso)
    return verts, norms


@functools.lru_cache(maxsize=None)
def _plain_engine():
    """one small handle for the tests that bring their own volume (the extraction reads no particle state)"""
    from dieselfluid_amd import SPHEngine
    from dieselfluid_amd.engine import reference_params
    return SPHEngine(reference_params(4), device=0)


# ---- 1. every corner pattern of one cube -------------------------------------------------------------------------------
def test_all_256_masks_of_one_cube_bit_for_bit():
    eng = _plain_engine()
    origin, step, dims = (0.25, -0.5, 1.0), (0.5, 0.75, 0.375), (2, 2, 2)
    total = 0
    for mask in range(256):
        vol = np.array([1.0 if (mask >> c) & 1 else -1.0 for c in range(8)], dtype=np.float32)  # corner c is voxel c
        want, wn = ref.extract(vol, origin, step, dims, 0.0)
        T, verts, norms = _extract(eng, _device(vol), origin, step, dims, 0.0, cap=12)
        assert T == want.shape[0] <= 12, mask
        assert ref.same_triangles(verts, want), mask
        assert np.array_equal(_bits(norms), _bits(ref.normals(verts))), mask
        assert np.all(np.abs(np.linalg.norm(norms.astype(np.float64), axis=1) - 1) < 1e-6), mask
        total += T
    # corners at +-1 around iso 0 cut every edge in its middle: unequal values, uneven cuts, on the same 256 patterns
    rng = np.random.default_rng(5)
    for mask in range(1, 255, 7):
        mag = rng.uniform(0.1, 3.0, 8)
        vol = np.array([mag[c] if (mask >> c) & 1 else -mag[c] for c in range(8)], dtype=np.float32)
        _check(eng, vol, origin, step, dims, 0.0)
    assert total == sum(int(ref.cube_counts(np.array([1.0 if (m >> c) & 1 else -1.0 for c in range(8)], np.float32), dims, 0.0)[0])
                        for m in range(256))


# ---- 2. the dam-break's surface ----------------------------------------------------------------------------------------
# with the oracle's volume, which the EXACT device volume equals bit for bit (test_gpu_volume.py): triangles, enclosed volume
EXACT_SURFACE = {"B": (11892, 1.021), "Bj": (11852, 1.013)}


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("tag", ["B", "Bj"])
def test_dambreak_surface_is_the_reference_closed_and_consistently_wound(tag, math_mode):
    eng, origin, step, dims = _engine(tag, math_mode)
    iso = _iso(tag)
    vol = eng.field_volume(origin, step, dims)  # the device's own volume, downloaded
    assert np.isfinite(vol).all() and int(np.sum(vol == iso)) == 0
    verts, _norms = _check(eng, vol, origin, step, dims, iso)
    V, E, F, closed, volume = ref.topology(verts)
    print(tag, "EXACT" if math_mode == EXACT else "FAST", "triangles", verts.shape[0], "degenerate", int(ref.degenerate(verts).sum()),
          "V - E + F", V - E + F, "enclosed volume", volume)
    assert not ref.degenerate(verts).any()
    assert closed and V - E + F == 2 and volume > 0
    if math_mode == EXACT:
        assert verts.shape[0] == EXACT_SURFACE[tag][0]
        assert abs(volume - EXACT_SURFACE[tag][1]) < 1e-3  # (the fluid block itself: 1.0)
    assert 0 < eng.get_option("surface_active_bricks") < 5 * 3 * 4  # (the bricks deep inside and far outside emit nothing)
    eng.close()


# ---- 3. shapes ---------------------------------------------------------------------------------------------------------
def _waves(dims, seed=0):
    """an analytic volume that crosses 0 all over the lattice, nowhere exactly: shape (nz, ny, nx)"""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.sin(0.83 * i + 0.4 * seed) + np.cos(0.57 * j) * 0.7 + np.sin(0.31 * k + 0.2 * j) * 0.9 + 0.013
    return v.astype(np.float32)


def test_an_axis_of_one_voxel_has_no_cubes():
    import torch
    eng = _plain_engine()
    for dims in [(1, 9, 9), (9, 1, 9), (9, 9, 1), (1, 1, 1), (1, 1, 40)]:
        vol = _waves(dims)
        T, verts, _n = _extract(eng, _device(vol), (0.0, 0.0, 0.0), (0.1, 0.1, 0.1), dims, 0.0, cap=4)
        assert T == 0 and verts.shape[0] == 0
        count = torch.full((1,), 77, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.surface_extract(_device(vol).data_ptr(), (0.0, 0.0, 0.0), (0.1, 0.1, 0.1), dims, 0.0, dev_count=count.data_ptr())
        eng.sync()
        assert int(count.cpu()[0]) == 0
        assert eng.get_option("surface_triangles") == 0 and eng.get_option("surface_active_bricks") == 0


@pytest.mark.parametrize("dims", [(9, 9, 5), (10, 10, 6), (9, 10, 5), (10, 9, 6), (6, 2, 2), (17, 9, 13), (8, 8, 4), (27, 23, 19)])
def test_dims_that_end_on_and_just_behind_a_brick_edge(dims):
    """a brick is 8 x 8 x 4 cubes, 9 x 9 x 5 voxels: dims of 9 (and 5 along z) fill one brick exactly, 10 (and 6) start a
    second one with a single layer of cubes"""
    eng = _plain_engine()
    vol = _waves(dims, seed=dims[0])
    verts, _ = _check(eng, vol, (-0.4, 0.3, 0.0), (0.11, 0.07, 0.13), dims, 0.0)
    assert verts.shape[0] > 0


def test_a_scan_with_more_than_one_workgroup_at_every_level_below_its_top():
    """The scan takes 256 values per workgroup and level.  A 3 x 3 x 262149 lattice has 65537 bricks (2 x 2 x 4 cubes each:
    every brick overhangs the lattice in x and y): level 0 scans 65537 counts in 257 workgroups, level 1 their 257 sums in 2,
    level 2 -- the top, one workgroup by construction -- those 2.  Triangles all along z, so every level's offsets count."""
    dims = (3, 3, 4 * 65537 + 1)
    vol = _waves(dims)
    eng = _plain_engine()
    verts, _ = _check(eng, vol, (0.0, 0.0, -3.0), (0.5, 0.5, 0.001), dims, 0.0)
    assert verts.shape[0] > 1000000 and eng.get_option("surface_active_bricks") > 30000
    # ... and with triangles only in the last brick of all, whose offset is then 0 through every level
    lone = np.full(dims[::-1], -1.0, dtype=np.float32)
    lone[-1, 1, 1] = 1.0
    verts, _ = _check(eng, lone, (0.0, 0.0, -3.0), (0.5, 0.5, 0.001), dims, 0.0)
    assert verts.shape[0] > 0 and eng.get_option("surface_active_bricks") == 1


# ---- 4. capacity -------------------------------------------------------------------------------------------------------
def test_a_short_capacity_gets_the_first_triangles_and_nothing_beyond():
    eng = _plain_engine()
    dims = (27, 23, 19)
    vol = _waves(dims, seed=3)
    origin, step = (-0.4, 0.3, 0.0), (0.11, 0.07, 0.13)
    dvol = _device(vol)
    T, full, full_n = _extract(eng, dvol, origin, step, dims, 0.0)
    assert T > 3000
    for cap in (0, 1, 2, 255, 256, 257, T // 2, T - 1, T, T + 5):
        got_T, v, n = _extract(eng, dvol, origin, step, dims, 0.0, cap=cap)  # (asserts the sentinels beyond min(T, cap))
        assert got_T == T
        m = min(T, cap)
        assert np.array_equal(_bits(v), _bits(full[:m])) and np.array_equal(_bits(n), _bits(full_n[:m])), cap
    # without normals: the same vertices, the normals' buffer untouched
    got_T, v, n = _extract(eng, dvol, origin, step, dims, 0.0, cap=T, normals=False)
    assert got_T == T and np.array_equal(_bits(v), _bits(full)) and n.size == 3 * T and np.all(n == SENTINEL)
    # the counting call: no outputs at all
    assert eng.surface_extract(dvol.data_ptr(), origin, step, dims, 0.0) == T


# ---- 5. the count stays on the device ----------------------------------------------------------------------------------
def test_dev_count_alone_needs_no_host_synchronisation():
    import torch
    eng = _plain_engine()
    dims = (17, 9, 13)
    vol = _waves(dims, seed=4)
    want, _ = ref.extract(vol, (0.0, 0.0, 0.0), (0.1, 0.1, 0.1), dims, 0.0)
    T = want.shape[0]
    eng.set_stream(torch.cuda.current_stream().cuda_stream)  # torch's own stream: what follows is ordered behind the call
    try:
        dvol = _device(vol)
        count = torch.full((3,), -5, dtype=torch.int64, device="cuda")
        verts = torch.full((9 * T,), SENTINEL, dtype=torch.float32, device="cuda")
        assert eng.surface_extract(dvol.data_ptr(), (0.0, 0.0, 0.0), (0.1, 0.1, 0.1), dims, 0.0, dev_vertices=verts.data_ptr(),
                                   cap=T, dev_count=count[1:].data_ptr(), want_count=False) is None
        doubled = count * 2  # a torch kernel behind the library's launches, on the same stream
        assert doubled.cpu().tolist() == [-10, 2 * T, -10]
        assert ref.same_triangles(verts.cpu().numpy().reshape(T, 3, 3), want)
    finally:
        eng.use_own_stream()


# ---- 6. dsl_field_surface ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", ["densities", "pressures"])
def test_field_surface_is_field_volume_plus_extract(scalar):
    eng, origin, step, dims = _engine("Bj", FAST)
    vol = eng.field_volume(origin, step, dims, scalar)
    iso = _iso("Bj") if scalar == "densities" else np.float32(np.median(vol[vol > 0]))  # (pressures: a few peaks, many zeros)
    assert np.isfinite(vol).all() and np.mean(vol >= iso) > 0.05 and np.mean(vol < iso) > 0.05
    T, want, want_n = _extract(eng, _device(vol), origin, step, dims, iso)
    assert T > 1000
    L, fp = eng._L, C.POINTER(C.c_float)
    o3, s3, d3 = (C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*dims)
    buf = 3 if scalar == "densities" else 4

    def call(cap, normals=True):
        v = np.full(9 * cap + GUARD, SENTINEL, dtype=np.float32)
        n = np.full(3 * cap + GUARD, SENTINEL, dtype=np.float32)
        cnt = C.c_int64(-1)
        assert L.dsl_field_surface(eng._h, buf, o3, s3, d3, C.c_float(iso), v.ctypes.data_as(fp),
                                   n.ctypes.data_as(fp) if normals else None, cap, C.byref(cnt)) == 0
        m = min(cap, cnt.value)
        assert np.all(v[9 * m:] == SENTINEL) and np.all(n[(3 * m if normals else 0):] == SENTINEL)
        return cnt.value, v[:9 * m].reshape(m, 3, 3), n[:3 * m].reshape(m, 3)

    short = T // 3
    n1, v1, nr1 = call(short)  # a short first call: the full count, the first triangles
    assert n1 == T and np.array_equal(_bits(v1), _bits(want[:short])) and np.array_equal(_bits(nr1), _bits(want_n[:short]))
    bytes_short = eng.get_option("device_bytes")
    n2, v2, nr2 = call(n1)     # ... completed by a second call with the capacity the first one named
    assert n2 == T and np.array_equal(_bits(v2), _bits(want)) and np.array_equal(_bits(nr2), _bits(want_n))
    assert eng.get_option("device_bytes") >= bytes_short + 48 * (T - short)  # the library's triangle array grew, and is counted
    n3, v3, _ = call(T + 7, normals=False)
    assert n3 == T and np.array_equal(_bits(v3), _bits(want))
    # the counting call
    cnt = C.c_int64(-1)
    assert L.dsl_field_surface(eng._h, buf, o3, s3, d3, C.c_float(iso), None, None, 0, C.byref(cnt)) == 0 and cnt.value == T
    # the Python wrapper: a guess that is too small costs a second call, not a wrong answer
    for guess in (0, 10):
        v, n = eng.field_surface(origin, step, dims, iso, scalar, guess=guess)
        assert v.shape == (T, 3, 3) and n.shape == (T, 3)
        assert np.array_equal(_bits(v), _bits(want)) and np.array_equal(_bits(n), _bits(want_n))
    eng.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_touch_nothing():
    import torch
    eng, origin, step, dims = _engine("B", FAST)
    iso = float(_iso())
    vol = eng.field_volume(origin, step, dims)
    dvol = _device(vol)
    T = eng.surface_extract(dvol.data_ptr(), origin, step, dims, iso)
    active = eng.get_option("surface_active_bricks")
    bytes_before = eng.get_option("device_bytes")
    verts = torch.full((9 * T,), SENTINEL, dtype=torch.float32, device="cuda")
    norms = torch.full((3 * T,), SENTINEL, dtype=torch.float32, device="cuda")
    count = torch.full((1,), -3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.timing_enable(True)
    eng.timing_reset()
    L = eng._L

    def call(volume=True, o=origin, s=step, d=dims, level=iso, out=True, cap=T):
        host = C.c_int64(-9)
        rc = L.dsl_surface_extract(eng._h, C.c_void_p(dvol.data_ptr() if volume else None), (C.c_float * 3)(*o), (C.c_float * 3)(*s),
                                   (C.c_int32 * 3)(*d), C.c_float(level), C.c_void_p(verts.data_ptr() if out else None),
                                   C.c_void_p(norms.data_ptr()), cap, C.c_void_p(count.data_ptr()), C.byref(host))
        return rc, L.dsl_last_error(eng._h).decode(), host.value

    inf, nan = float("inf"), float("nan")
    refused = [
        (dict(volume=False), "dev_volume"),
        (dict(d=(27, 0, 19)), "dims"), (dict(d=(-1, 23, 19)), "dims"),
        (dict(d=(1025, 1024, 1024)), "dims"), (dict(d=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), "dims"),
        (dict(s=(0.1, 0.0, 0.1)), "step"), (dict(s=(-0.1, 0.1, 0.1)), "step"), (dict(s=(0.1, 0.1, inf)), "step"),
        (dict(s=(nan, 0.1, 0.1)), "step"),
        (dict(o=(0.0, nan, 0.0)), "origin"), (dict(o=(-inf, 0.0, 0.0)), "origin"),
        (dict(level=nan), "iso"), (dict(level=inf), "iso"),
        (dict(out=False), "dev_vertices"),
        (dict(d=(1024, 1024, 1024), out=False), "dev_vertices"),  # exactly 2^30 voxels pass the size check
    ]
    for kwargs, word in refused:
        rc, text, host = call(**kwargs)
        assert rc == -1 and "dsl_surface_extract" in text and word in text, (kwargs, rc, text)
        assert host == -9
    eng.sync()
    assert torch.all(verts == SENTINEL) and torch.all(norms == SENTINEL) and int(count.cpu()[0]) == -3
    assert eng.get_option("device_bytes") == bytes_before
    assert eng.get_option("surface_triangles") == T and eng.get_option("surface_active_bricks") == active
    assert eng.timing("surface")[1] == 0  # nothing was launched
    # dsl_field_surface: its own two, and dsl_field_volume's
    hv = np.full(9, SENTINEL, dtype=np.float32)
    fp = C.POINTER(C.c_float)

    def field(buffer=3, d=dims, level=iso, out=True, cap=1):
        cnt = C.c_int64(-9)
        rc = L.dsl_field_surface(eng._h, buffer, (C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*d), C.c_float(level),
                                 hv.ctypes.data_as(fp) if out else None, None, cap, C.byref(cnt))
        return rc, L.dsl_last_error(eng._h).decode(), cnt.value

    for kwargs, word in [(dict(buffer=0), "scalar_buffer"), (dict(d=(27, 23, 0)), "dims"), (dict(level=nan), "iso"),
                         (dict(out=False), "host_vertices")]:
        rc, text, cnt = field(**kwargs)
        assert rc == -1 and word in text and cnt == -9, (kwargs, rc, text)
    assert np.all(hv == SENTINEL) and eng.timing("surface")[1] == 0 and eng.timing("volume")[1] == 0
    assert eng.get_option("device_bytes") == bytes_before
    # the next valid call is unaffected
    rc, _text, host = call()
    assert rc == 0 and host == T
    want, _ = ref.extract(vol, origin, step, dims, iso)
    assert ref.same_triangles(verts.cpu().numpy().reshape(T, 3, 3), want) and int(count.cpu()[0]) == T
    eng.close()


def test_a_slab_handle_extracts_but_has_no_field_surface():
    eng, origin, step, dims = _engine("B", FAST, density=False)
    eng.slab_config(0, -0.5, 0.5)
    vol = _waves(dims, seed=2)
    _check(eng, vol, origin, step, dims, 0.0)
    hv = np.full(9, SENTINEL, dtype=np.float32)
    cnt = C.c_int64(-9)
    rc = eng._L.dsl_field_surface(eng._h, 3, (C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*dims), C.c_float(0.5),
                                  hv.ctypes.data_as(C.POINTER(C.c_float)), None, 1, C.byref(cnt))
    assert rc == -4 and "slab" in eng._L.dsl_last_error(eng._h).decode()
    assert np.all(hv == SENTINEL) and cnt.value == -9
    eng.close()


# ---- 8. a live skin episode stays live ---------------------------------------------------------------------------------
def test_an_extract_between_skin_steps_leaves_the_episode_alone():
    dims = (17, 9, 13)
    dvol = _device(_waves(dims, seed=6))
    res = []
    for with_extract in (True, False):
        eng, _o, _s, _d = _engine("B", FAST, density=False)
        eng.reset_forces()
        eng.set_option("skin", 0.1)
        for _ in range(5):
            eng.wcsph_step(1)
            if with_extract:
                assert eng.surface_extract(dvol.data_ptr(), (0.0, 0.0, 0.0), (0.1, 0.1, 0.1), dims, 0.0) > 0
        steps, rebuilds = eng.get_option("skin_steps"), eng.get_option("skin_rebuilds")
        res.append((eng.download("positions"), eng.download("velocities"), steps, rebuilds))
        eng.close()
    print("skin steps", res[0][2], res[1][2], "rebuilds", res[0][3], res[1][3])
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and np.array_equal(_bits(res[0][1]), _bits(res[1][1]))
    assert res[0][2] == res[1][2] > 0 and res[0][3] == res[1][3] < res[0][2]  # (a settled episode rebuilds at its next step)


# ---- 9. determinism and timing -----------------------------------------------------------------------------------------
def test_two_extractions_give_the_same_bytes_and_are_timed():
    eng, origin, step, dims = _engine("Bj", FAST)
    iso = _iso("Bj")
    dvol = _device(eng.field_volume(origin, step, dims))
    eng.timing_enable(True)
    eng.timing_reset()
    T, a, an = _extract(eng, dvol, origin, step, dims, iso)  # a counting call, then the extraction
    ms, launches = eng.timing("surface")
    assert launches == 2 + 3 and ms > 0.0  # count and scan; count, scan and emit
    parts = [eng.get_option("surface_%s_ms" % k) for k in ("count", "scan", "emit")]
    assert all(v > 0.0 for v in parts), parts
    for _ in range(3):
        T2, b, bn = _extract(eng, dvol, origin, step, dims, iso, cap=T)
        assert T2 == T and np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(an), _bits(bn))
    eng.close()
