"""GPU: dsl_surface_extract_indexed and dsl_field_surface_indexed -- the fluid surface as an indexed mesh: every vertex once,
a normal per vertex, three int32 ids per triangle (include/dslsph.h has the rule).  The reference is tests/surface_mesh_ref.py,
a numpy restatement on top of surface_ref; positions, normals and ids are compared bit for bit, in the product's order.
Volumes are uploaded arrays, as in test_gpu_surface.py, whose small helpers (the dam-break case, the plain handle) are used."""
import ctypes as C
import functools

import numpy as np
import pytest

import surface_mesh_ref as mref
import surface_ref as ref
from test_gpu_surface import EXACT, FAST, GUARD, SENTINEL, _bits, _case, _device, _engine, _extract, _iso, _plain_engine, _waves
from test_surface_mesh_cpu import random_volume

pytestmark = pytest.mark.gpu

ISENT = -77
ORIGIN, STEP = (-0.4, 0.3, 0.05), (0.11, 0.07, 0.13)


def _mesh(eng, dvol, origin, step, dims, iso, cap_v=None, cap_t=None, normals=True):
    """(V, T, positions (min(V, cap_v), 3), normals, indices (min(T, cap_t), 3)) through guarded device buffers: nothing outside
    the first min(V, cap_v) vertices and min(T, cap_t) triples may change.  A capacity of None: a counting call first."""
    import torch
    if cap_v is None or cap_t is None:
        V0, T0 = eng.surface_extract_indexed(dvol.data_ptr(), origin, step, dims, iso)
        cap_v, cap_t = V0 if cap_v is None else cap_v, T0 if cap_t is None else cap_t
    pbuf = torch.full((GUARD + 3 * cap_v + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    nbuf = torch.full((GUARD + 3 * cap_v + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    ibuf = torch.full((GUARD + 3 * cap_t + GUARD,), ISENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    V, T = eng.surface_extract_indexed(dvol.data_ptr(), origin, step, dims, iso, dev_positions=pbuf[GUARD:].data_ptr(),
                                       dev_normals=nbuf[GUARD:].data_ptr() if normals else None, cap_vertices=cap_v,
                                       dev_indices=ibuf[GUARD:].data_ptr(), cap_triangles=cap_t)
    eng.sync()
    nv, nt = min(V, cap_v), min(T, cap_t)
    p, n, i = pbuf.cpu().numpy(), nbuf.cpu().numpy(), ibuf.cpu().numpy()
    assert np.all(p[:GUARD] == SENTINEL) and np.all(p[GUARD + 3 * nv:] == SENTINEL), "positions written outside the first min(V, cap)"
    assert np.all(n[:GUARD] == SENTINEL) and np.all(n[GUARD + (3 * nv if normals else 0):] == SENTINEL)
    assert np.all(i[:GUARD] == ISENT) and np.all(i[GUARD + 3 * nt:] == ISENT), "indices written outside the first min(T, cap)"
    return (V, T, p[GUARD:GUARD + 3 * nv].reshape(nv, 3).copy(), n[GUARD:GUARD + 3 * nv].reshape(nv, 3).copy(),
            i[GUARD:GUARD + 3 * nt].reshape(nt, 3).copy())


def _check(eng, vol, origin, step, dims, iso):
    """the device against the reference on one host volume: V, T, positions, normals, ids, the two options"""
    wp, wn, wi = mref.mesh(vol, origin, step, dims, iso)
    V, T, pos, nrm, idx = _mesh(eng, _device(vol), origin, step, dims, iso)
    assert (V, T) == (wp.shape[0], wi.shape[0]), (V, T, wp.shape[0], wi.shape[0])
    assert np.array_equal(idx, wi)
    assert np.array_equal(_bits(pos), _bits(wp))
    assert np.array_equal(_bits(nrm), _bits(wn))
    assert eng.get_option("surface_vertices") == V and eng.get_option("surface_triangles") == T
    return pos, nrm, idx


# ---- 1. every corner pattern of one cube -------------------------------------------------------------------------------
def test_all_256_masks_of_one_cube_bit_for_bit():
    eng = _plain_engine()
    origin, step, dims = (0.25, -0.5, 1.0), (0.5, 0.75, 0.375), (2, 2, 2)
    rng = np.random.default_rng(5)
    seen = 0
    for mask in range(256):
        mag = rng.uniform(0.1, 3.0, 8) if mask % 3 else np.ones(8)  # (+-1 cuts every edge in its middle; the others unevenly)
        vol = np.array([mag[c] if (mask >> c) & 1 else -mag[c] for c in range(8)], dtype=np.float32)  # corner c is voxel c
        wp, wn, wi = mref.mesh(vol, origin, step, dims, 0.0)
        V, T, pos, nrm, idx = _mesh(eng, _device(vol), origin, step, dims, 0.0, cap_v=19, cap_t=12)  # (a cube has 19 edges)
        assert (V, T) == (wp.shape[0], wi.shape[0]) and V <= 19 and T <= 12, mask
        assert np.array_equal(idx, wi), mask
        assert np.array_equal(_bits(pos), _bits(wp)) and np.array_equal(_bits(nrm), _bits(wn)), mask  # (every gradient one-sided)
        seen += V
    assert seen > 2000


# ---- 2. NaN voxels and ties, past the brick edges ----------------------------------------------------------------------
RDIMS, RISO = (18, 17, 10), 0.25


@functools.lru_cache(maxsize=None)
def _random():
    vol = random_volume(RDIMS, 21, iso=RISO)
    assert 0.01 < np.mean(np.isnan(vol)) < 0.06 and 0.03 < np.mean(vol == np.float32(RISO)) < 0.08
    return vol  # (shared: no test writes to it)


def test_a_random_volume_with_nan_and_ties_is_the_reference_and_the_soup():
    """18 x 17 x 10: x has one cube past a brick edge; y and z end exactly on an edge of the bricks of cubes, so there is one
    more brick of voxels than of cubes; z = 10 puts two voxels into a third brick of voxels"""
    vol = _random()
    res = []
    for math_mode in (FAST, EXACT):
        eng, _o, _s, _d = _engine("B", math_mode, density=False)
        pos, nrm, idx = _check(eng, vol, ORIGIN, STEP, RDIMS, RISO)
        # through the ids: the reference soup and the product's own soup on the same handle, corner by corner
        want, _ = ref.extract(vol.ravel(), ORIGIN, STEP, RDIMS, RISO)
        T, soup, _n = _extract(eng, _device(vol), ORIGIN, STEP, RDIMS, RISO)
        assert T == idx.shape[0] > 1000
        assert np.array_equal(_bits(pos[idx]), _bits(want)) and np.array_equal(_bits(pos[idx]), _bits(soup))
        assert np.array_equal(np.unique(idx), np.arange(pos.shape[0]))  # every vertex is referenced
        assert np.unique(_bits(pos), axis=0).shape[0] < pos.shape[0]    # (ties: distinct vertices with the same bits)
        # a second call gives the same bytes
        V2, T2, p2, n2, i2 = _mesh(eng, _device(vol), ORIGIN, STEP, RDIMS, RISO)
        assert np.array_equal(_bits(p2), _bits(pos)) and np.array_equal(_bits(n2), _bits(nrm)) and np.array_equal(i2, idx)
        res.append((pos, nrm, idx))
        eng.close()
    # both math modes give the same bytes
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(res[0][:2], res[1][:2])) and np.array_equal(res[0][2], res[1][2])


@pytest.mark.parametrize("dims", [(9, 9, 5), (10, 10, 6), (8, 8, 4), (17, 9, 13), (6, 2, 2), (1, 9, 9), (9, 9, 1)])
def test_dims_that_end_on_and_just_behind_a_brick_edge(dims):
    eng = _plain_engine()
    vol = random_volume(dims, dims[0] + dims[2], nan=0.02, tie=0.03, iso=0.0)
    pos, _nrm, _idx = _check(eng, vol, ORIGIN, STEP, dims, 0.0)
    assert (pos.shape[0] > 0) == (min(dims) > 1)


# ---- 3. the dam-break's surface ----------------------------------------------------------------------------------------
def test_the_dambreak_mesh_welded_by_id_is_closed():
    eng, origin, step, dims = _engine("Bj", FAST)
    iso = _iso("Bj")
    vol = eng.field_volume(origin, step, dims)
    pos, nrm, idx = _check(eng, vol, origin, step, dims, iso)
    closed, E = mref.closed_by_id(idx)  # (zero-area triangles stay in: ids keep a tie a manifold)
    V, F = pos.shape[0], idx.shape[0]
    print("dam-break Bj: V, E, F =", V, E, F, "triangle soup bytes", 48 * F, "indexed bytes", 24 * V + 12 * F)
    assert closed and V - E + F == 2 and F > 10000
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=1e-6)
    eng.close()


# ---- 4. a vertex scan of three levels ----------------------------------------------------------------------------------
def test_a_vertex_scan_of_three_levels():
    """3 x 3 x (4 * 65537 + 1) voxels: 65538 bricks of voxels (65537 of cubes), so the vertex scan has 257 workgroups at level
    0, 2 at level 1 and its top.  Sparse: a few inside voxels, at both ends, around the level boundaries -- and in the last
    brick of voxels, which holds the lattice's last layer alone."""
    nz = 4 * 65537 + 1
    dims = (3, 3, nz)
    vol = np.full((nz, 3, 3), -1.0, dtype=np.float32)
    for k in (0, 5, 4 * 256 - 1, 4 * 256, 4 * 256 * 255 + 2, 4 * 65536 - 1, 4 * 65536, 4 * 65536 + 3, nz - 2, nz - 1):
        vol[k, 1, 1] = 1.0 + 0.001 * (k % 7)
    vol[4 * 300, 0, 2] = 2.0
    vol[4 * 300 + 1, 1, 1] = np.nan
    eng = _plain_engine()
    pos, _nrm, idx = _check(eng, vol, (0.0, 0.0, -3.0), (0.5, 0.5, 0.001), dims, 0.0)
    assert pos.shape[0] > 100 and idx.max() == pos.shape[0] - 1
    u, _d = mref.vertex_order(mref.vertex_edges(vol, dims, 0.0), dims)
    assert (u // 9).max() == nz - 1  # a vertex owned by the last brick of voxels


# ---- 5. capacity -------------------------------------------------------------------------------------------------------
def test_short_capacities_get_the_first_vertices_and_triples_and_nothing_beyond():
    eng = _plain_engine()
    vol = _random()
    dvol = _device(vol)
    V, T, pos, nrm, idx = _mesh(eng, dvol, ORIGIN, STEP, RDIMS, RISO)
    assert V > 500 and T > 1000
    caps = [(0, T), (1, T), (V // 2, T), (V - 1, T + 3),                    # the vertices short
            (V, 0), (V, 1), (V + 5, 255), (V, 256), (V, 257), (V, T - 1),   # the triangles short
            (0, 0), (1, 1), (255, 256), (V // 3, T // 3), (V - 1, T - 1),   # both
            (V, T), (V + 5, T + 5)]
    for cap_v, cap_t in caps:
        gV, gT, p, n, i = _mesh(eng, dvol, ORIGIN, STEP, RDIMS, RISO, cap_v=cap_v, cap_t=cap_t)  # (asserts the guard words)
        assert (gV, gT) == (V, T), (cap_v, cap_t)
        mv, mt = min(V, cap_v), min(T, cap_t)
        assert np.array_equal(_bits(p), _bits(pos[:mv])) and np.array_equal(_bits(n), _bits(nrm[:mv])), (cap_v, cap_t)
        assert np.array_equal(i, idx[:mt]), (cap_v, cap_t)


# ---- 6. counting, count words, no normals ------------------------------------------------------------------------------
def test_counting_calls_device_counts_and_null_normals():
    import torch
    eng = _plain_engine()
    vol = _random()
    wp, wn, wi = mref.mesh(vol, ORIGIN, STEP, RDIMS, RISO)
    V, T = wp.shape[0], wi.shape[0]
    dvol = _device(vol)
    assert eng.surface_extract_indexed(dvol.data_ptr(), ORIGIN, STEP, RDIMS, RISO) == (V, T)  # NULL outputs, capacities of 0
    assert eng.get_option("surface_vertices") == V and eng.get_option("surface_triangles") == T
    # dev_normals NULL: positions and ids as ever, the normals' buffer untouched
    gV, gT, p, n, i = _mesh(eng, dvol, ORIGIN, STEP, RDIMS, RISO, cap_v=V, cap_t=T, normals=False)
    assert (gV, gT) == (V, T) and np.array_equal(_bits(p), _bits(wp)) and np.array_equal(i, wi) and np.all(n == SENTINEL)
    # dev_counts alone: no host copy, what follows on the stream sees the counts
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        counts = torch.full((4,), -5, dtype=torch.int64, device="cuda")
        assert eng.surface_extract_indexed(dvol.data_ptr(), ORIGIN, STEP, RDIMS, RISO, dev_counts=counts[1:].data_ptr(),
                                           want_counts=False) is None
        doubled = counts * 2  # a torch kernel behind the library's launches, on the same stream
        assert doubled.cpu().tolist() == [-10, 2 * V, 2 * T, -10]
        # a lattice without cubes: both words are zeroed
        flat = _device(_waves((9, 9, 1)))
        eng.surface_extract_indexed(flat.data_ptr(), ORIGIN, STEP, (9, 9, 1), 0.0, dev_counts=counts[1:].data_ptr(), want_counts=False)
        assert counts.cpu().tolist() == [-5, 0, 0, -5]
        assert eng.get_option("surface_vertices") == 0 and eng.get_option("surface_triangles") == 0
    finally:
        eng.use_own_stream()


# ---- 7. dsl_field_surface_indexed --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", ["densities", "pressures"])
def test_field_surface_indexed_is_field_volume_plus_the_indexed_extraction(scalar):
    eng, origin, step, dims = _engine("Bj", FAST)
    vol = eng.field_volume(origin, step, dims, scalar)
    iso = _iso("Bj") if scalar == "densities" else np.float32(np.median(vol[vol > 0]))
    V, T, pos, nrm, idx = _mesh(eng, _device(vol), origin, step, dims, iso)
    assert V > 500 and T > 1000
    L, fp, ip = eng._L, C.POINTER(C.c_float), C.POINTER(C.c_int32)
    o3, s3, d3 = (C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*dims)
    buf = 3 if scalar == "densities" else 4

    def call(cap_v, cap_t, normals=True):
        p = np.full(3 * cap_v + GUARD, SENTINEL, dtype=np.float32)
        n = np.full(3 * cap_v + GUARD, SENTINEL, dtype=np.float32)
        i = np.full(3 * cap_t + GUARD, ISENT, dtype=np.int32)
        cnt = (C.c_int64 * 2)(-1, -1)
        assert L.dsl_field_surface_indexed(eng._h, buf, o3, s3, d3, C.c_float(iso), p.ctypes.data_as(fp),
                                           n.ctypes.data_as(fp) if normals else None, cap_v, i.ctypes.data_as(ip), cap_t, cnt) == 0
        mv, mt = min(cap_v, cnt[0]), min(cap_t, cnt[1])
        assert np.all(p[3 * mv:] == SENTINEL) and np.all(n[(3 * mv if normals else 0):] == SENTINEL) and np.all(i[3 * mt:] == ISENT)
        return (cnt[0], cnt[1]), p[:3 * mv].reshape(mv, 3), n[:3 * mv].reshape(mv, 3), i[:3 * mt].reshape(mt, 3)

    c1, p1, n1, i1 = call(V // 3, T // 2)  # short: the full counts, the first of each
    assert c1 == (V, T) and np.array_equal(_bits(p1), _bits(pos[:V // 3])) and np.array_equal(_bits(n1), _bits(nrm[:V // 3]))
    assert np.array_equal(i1, idx[:T // 2])
    bytes_short = eng.get_option("device_bytes")
    c2, p2, n2, i2 = call(*c1)             # ... completed by a second call with the capacities the first one named
    assert c2 == (V, T) and np.array_equal(_bits(p2), _bits(pos)) and np.array_equal(_bits(n2), _bits(nrm)) and np.array_equal(i2, idx)
    assert eng.get_option("device_bytes") > bytes_short  # the library's mesh array grew, and is counted
    c3, p3, _n3, i3 = call(V + 7, T + 7, normals=False)
    assert c3 == (V, T) and np.array_equal(_bits(p3), _bits(pos)) and np.array_equal(i3, idx)
    cnt = (C.c_int64 * 2)(-1, -1)          # the counting call
    assert L.dsl_field_surface_indexed(eng._h, buf, o3, s3, d3, C.c_float(iso), None, None, 0, None, 0, cnt) == 0
    assert (cnt[0], cnt[1]) == (V, T)
    # the Python wrapper: a guess that is too small costs a second call, not a wrong answer
    for guess in ((0, 0), (10, 10), (10, 10 * T), (10 * V, 10)):
        p, n, i = eng.field_surface_indexed(origin, step, dims, iso, scalar, guess=guess)
        assert np.array_equal(_bits(p), _bits(pos)) and np.array_equal(_bits(n), _bits(nrm)) and np.array_equal(i, idx)
    eng.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_touch_nothing():
    import torch
    eng, origin, step, dims = _engine("B", FAST)
    iso = float(_iso())
    vol = eng.field_volume(origin, step, dims)
    dvol = _device(vol)
    V, T = eng.surface_extract_indexed(dvol.data_ptr(), origin, step, dims, iso)
    bytes_before = eng.get_option("device_bytes")
    pos = torch.full((3 * V,), SENTINEL, dtype=torch.float32, device="cuda")
    nrm = torch.full((3 * V,), SENTINEL, dtype=torch.float32, device="cuda")
    idx = torch.full((3 * T,), ISENT, dtype=torch.int32, device="cuda")
    counts = torch.full((2,), -3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.timing_enable(True)
    eng.timing_reset()
    L = eng._L

    def call(volume=True, o=origin, s=step, d=dims, level=iso, p=True, i=True, cap_v=V, cap_t=T):
        host = (C.c_int64 * 2)(-9, -9)
        rc = L.dsl_surface_extract_indexed(eng._h, C.c_void_p(dvol.data_ptr() if volume else None), (C.c_float * 3)(*o),
                                           (C.c_float * 3)(*s), (C.c_int32 * 3)(*d), C.c_float(level),
                                           C.c_void_p(pos.data_ptr() if p else None), C.c_void_p(nrm.data_ptr()), cap_v,
                                           C.c_void_p(idx.data_ptr() if i else None), cap_t, C.c_void_p(counts.data_ptr()), host)
        return rc, L.dsl_last_error(eng._h).decode(), (host[0], host[1])

    inf, nan = float("inf"), float("nan")
    refused = [
        (dict(volume=False), "dev_volume"),
        (dict(d=(27, 0, 19)), "dims"), (dict(d=(-1, 23, 19)), "dims"),
        (dict(d=(1025, 512, 512)), "2^28"), (dict(d=(1024, 1024, 1024)), "2^28"),  # (no allocation is needed to say so)
        (dict(d=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), "2^28"),
        (dict(s=(0.1, 0.0, 0.1)), "step"), (dict(s=(-0.1, 0.1, 0.1)), "step"), (dict(s=(0.1, 0.1, inf)), "step"),
        (dict(s=(nan, 0.1, 0.1)), "step"),
        (dict(o=(0.0, nan, 0.0)), "origin"), (dict(o=(-inf, 0.0, 0.0)), "origin"),
        (dict(level=nan), "iso"), (dict(level=inf), "iso"),
        (dict(p=False), "dev_positions"), (dict(p=False, cap_t=0), "dev_positions"),
        (dict(i=False), "dev_indices"), (dict(i=False, cap_v=0), "dev_indices"),
        (dict(d=(1024, 512, 512), p=False), "dev_positions"),  # exactly 2^28 voxels pass the size check
    ]
    for kwargs, word in refused:
        rc, text, host = call(**kwargs)
        assert rc == -1 and "dsl_surface_extract_indexed" in text and word in text, (kwargs, rc, text)
        assert host == (-9, -9)
    eng.sync()
    assert torch.all(pos == SENTINEL) and torch.all(nrm == SENTINEL) and torch.all(idx == ISENT) and counts.cpu().tolist() == [-3, -3]
    assert eng.get_option("device_bytes") == bytes_before
    assert eng.get_option("surface_vertices") == V and eng.get_option("surface_triangles") == T
    assert eng.timing("surface_mesh")[1] == 0 and eng.timing("surface")[1] == 0  # nothing was launched
    # dsl_field_surface_indexed: its own, and dsl_field_volume's
    hp, hi = np.full(3, SENTINEL, dtype=np.float32), np.full(3, ISENT, dtype=np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def field(buffer=3, d=dims, level=iso, p=True, i=True):
        cnt = (C.c_int64 * 2)(-9, -9)
        rc = L.dsl_field_surface_indexed(eng._h, buffer, (C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*d),
                                         C.c_float(level), hp.ctypes.data_as(fp) if p else None, None, 1,
                                         hi.ctypes.data_as(ip) if i else None, 1, cnt)
        return rc, L.dsl_last_error(eng._h).decode(), (cnt[0], cnt[1])

    for kwargs, word in [(dict(buffer=0), "scalar_buffer"), (dict(d=(27, 23, 0)), "dims"), (dict(d=(1024, 1024, 257)), "2^28"),
                         (dict(level=nan), "iso"), (dict(p=False), "host_positions"), (dict(i=False), "host_indices")]:
        rc, text, cnt = field(**kwargs)
        assert rc == -1 and word in text and cnt == (-9, -9), (kwargs, rc, text)
    assert np.all(hp == SENTINEL) and np.all(hi == ISENT)
    assert eng.timing("surface_mesh")[1] == 0 and eng.timing("surface")[1] == 0 and eng.timing("volume")[1] == 0
    assert eng.get_option("device_bytes") == bytes_before
    # the next valid call is unaffected
    rc, _text, host = call()
    assert rc == 0 and host == (V, T)
    wp, _wn, wi = mref.mesh(vol, origin, step, dims, iso)
    assert np.array_equal(_bits(pos.cpu().numpy().reshape(V, 3)), _bits(wp)) and np.array_equal(idx.cpu().numpy().reshape(T, 3), wi)
    assert counts.cpu().tolist() == [V, T]
    eng.close()


# ---- 9. slab handles and skin episodes ---------------------------------------------------------------------------------
def test_a_slab_handle_extracts_but_has_no_field_surface_indexed():
    eng, origin, step, dims = _engine("B", FAST, density=False)
    eng.slab_config(0, -0.5, 0.5)
    _check(eng, random_volume(dims, 2, iso=0.0), origin, step, dims, 0.0)
    hp, hi = np.full(3, SENTINEL, dtype=np.float32), np.full(3, ISENT, dtype=np.int32)
    cnt = (C.c_int64 * 2)(-9, -9)
    rc = eng._L.dsl_field_surface_indexed(eng._h, 3, (C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*dims),
                                          C.c_float(0.5), hp.ctypes.data_as(C.POINTER(C.c_float)), None, 1,
                                          hi.ctypes.data_as(C.POINTER(C.c_int32)), 1, cnt)
    assert rc == -4 and "slab" in eng._L.dsl_last_error(eng._h).decode()
    assert np.all(hp == SENTINEL) and np.all(hi == ISENT) and (cnt[0], cnt[1]) == (-9, -9)
    eng.close()


def test_an_extraction_between_skin_steps_leaves_the_episode_alone():
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
                V, T = eng.surface_extract_indexed(dvol.data_ptr(), (0.0, 0.0, 0.0), (0.1, 0.1, 0.1), dims, 0.0)
                assert V > 0 and T > 0
        steps, rebuilds = eng.get_option("skin_steps"), eng.get_option("skin_rebuilds")
        res.append((eng.download("positions"), eng.download("velocities"), steps, rebuilds))
        eng.close()
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])) and np.array_equal(_bits(res[0][1]), _bits(res[1][1]))
    assert res[0][2] == res[1][2] > 0 and res[0][3] == res[1][3] < res[0][2]


# ---- 10. timing --------------------------------------------------------------------------------------------------------
def test_the_launches_are_counted_under_surface_mesh():
    eng, origin, step, dims = _engine("Bj", FAST)
    iso = _iso("Bj")
    dvol = _device(eng.field_volume(origin, step, dims))
    eng.timing_enable(True)
    eng.timing_reset()
    _mesh(eng, dvol, origin, step, dims, iso)  # a counting call, then the extraction
    ms, launches = eng.timing("surface_mesh")
    assert launches == 2 + 4 and ms > 0.0     # vertex count and scan; vertex count, scan, vertex emit and index emit
    assert eng.timing("surface")[1] == 2 + 2  # the triangle count and its scan, twice: they stay under DSL_K_SURFACE
    parts = [eng.get_option("surface_mesh_%s_ms" % k) for k in ("vcount", "vscan", "vemit", "iemit")]
    assert all(v > 0.0 for v in parts), parts
    eng.surface_extract_indexed(dvol.data_ptr(), origin, step, dims, iso)  # a counting call emits nothing
    assert eng.get_option("surface_mesh_vemit_ms") == 0.0 and eng.get_option("surface_mesh_iemit_ms") == 0.0
    assert eng.get_option("surface_mesh_vcount_ms") > 0.0
    eng.close()
