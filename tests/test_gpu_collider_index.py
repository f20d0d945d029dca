"""GPU: the cell index over the collider's triangles (DSL_OPT_COLLIDE_INDEX; csrc/kernels_collide_index.hpp).  With the
index on, query and response are the list walk's, and the list walk's are tests/collider_ref.py's: every check of a result
here is an equality on bits against that numpy reference (or, for the step drivers, against the same handle with the
index off), on the inputs of tests/test_gpu_collider.py -- irregular triangles that win, slow lanes, one-lane waves -- a
curved mesh, and the corners of the index itself; the counters (DSL_OPT_COLLIDE_VISITS, _FULL_WAVES) show that it is the
indexed kernel that ran and that it visits what a model computed here allows, no more."""
import ctypes as C
import functools

import numpy as np
import pytest

import collider_ref as cr
import helpers
import test_gpu_collider as tc
from test_gpu_collider import DT, EXACT, FAST, R, R2, REST, _bits, _engine, _same

pytestmark = pytest.mark.gpu

f32 = np.float32
EDGES = (0.0, 0.125, 0.25, 100.0)  # the library's choice, two set ones, and one cell for everything


def _indexed(pos, vel, verts, normals, r, math_mode, *, edge=0.0, cell_order=False, option_first=True):
    """an engine with the particles uploaded, the mesh set and the index on"""
    eng, _p = _engine(pos.shape[0], math_mode)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    if cell_order:
        eng.nn()
    if option_first:
        eng.set_option("collide_index_edge", edge)
        eng.set_option("collide_index", 1)
    eng.set_collider_mesh(verts, normals, r, REST)
    if not option_first:
        eng.set_option("collide_index", 1)
        eng.set_option("collide_index_edge", edge)
    assert eng.get_option("collide_index") == 1 and eng.get_option("collide_index_cells") > 0
    if edge:
        assert eng.get_option("collide_index_edge") == f32(edge)
    return eng


def _check_query_and_pass(eng, ref_query, ref_pass, what):
    """query, then response, against the numpy reference; both ran the indexed kernel.  -> (visits, full waves) of the pass"""
    tri, normal, coord, point = ref_query
    want_x, want_v, moved = ref_pass
    gtri, gnormal, gcoord, gpoint = eng.collider_query()
    assert eng.get_option("collide_visits") >= 0, what
    assert np.array_equal(gtri, tri), (what, np.flatnonzero(gtri != tri)[:8], gtri[gtri != tri][:8], tri[gtri != tri][:8])
    assert _same(gnormal, normal) and _same(gcoord, coord) and _same(gpoint, point), what
    eng.collide()
    visits, full = eng.get_option("collide_visits"), eng.get_option("collide_full_waves")
    assert visits >= 0 and full >= 0, what
    assert _same(eng.download("positions"), want_x) and _same(eng.download("velocities"), want_v), what
    assert eng.get_option("collide_hits") == int(moved.sum()), what
    return visits, full


# ---- 1. query and pass equal collider_ref, index on ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _response(T, lo, hi):
    pos, vel = tc._particles()
    out = cr.respond(pos[lo:hi], vel[lo:hi], *tc._mesh(T), DT, R, REST)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("T,lo,hi", [(12, 0, 1000), (300, 0, 1000), (300, 200, 264), (300, 225, 226)])
def test_query_and_pass_equal_the_reference_with_the_index_on(T, lo, hi, math_mode):
    """test_gpu_collider's particles and meshes (in _mesh(300) the zero-normal triangle 299 and the irregular 200..219 are
    among the winners: the always-list decides results), host order and cell order, four cell edges"""
    pos, vel = tc._particles()
    pos, vel = pos[lo:hi], vel[lo:hi]
    v, nr = tc._mesh(T)
    ref = tc._reference(T, lo, hi)
    if T == 300 and hi - lo == 1000:
        assert np.any(ref[0] == 299) and np.any((ref[0] >= 200) & (ref[0] < 220))
    for cell_order in (False, True):
        for k, edge in enumerate(EDGES):
            eng = _indexed(pos, vel, v, nr, R, math_mode, edge=edge, cell_order=cell_order, option_first=bool(k % 2))
            if T == 300:  # the 22 irregular triangles (test_collide_index_cpu restates which) are on the always-list
                assert eng.get_option("collide_index_entries") >= 300
            if edge == 100.0:
                assert eng.get_option("collide_index_cells") == 1
                assert eng.get_option("collide_index_entries") == T
            visits, full = _check_query_and_pass(eng, ref[:4], _response(T, lo, hi), (T, lo, hi, cell_order, edge))
            if hi - lo == 1000 and not cell_order:
                # the 20 slow particles sit in four of the sixteen waves (test_gpu_collider checks that on the CPU)
                assert full == 4
            elif hi - lo < 1000:
                assert full == 0
            eng.close()


# ---- 2. the index is at work -----------------------------------------------------------------------------------------

def _visit_model(order, pos, vel, verts, r, edge):
    """Per wave of 64 slots in slot order `order`: the triangles whose box, taken loosely as tc._skipped_chunks does
    (2.2 r + 2 % of its extents + 2e-5 of its largest coordinate: more than the kernel's pad) and grown by one cell edge,
    holds some moving lane of the wave.  A triangle in a lane's cell list overlaps the lane's cell, so the lane lies
    within one edge of the triangle's box: the kernel visits no more than this."""
    x = pos[order].astype(np.float64)
    moving = cr._dot(vel, vel)[order] != 0
    q = verts.reshape(-1, 3, 3).astype(np.float64)
    lo, hi = q.min(axis=1), q.max(axis=1)
    pad = (2.2 * r + 0.02 * (hi - lo).sum(axis=1) + 2e-5 * np.abs(q).max(axis=(1, 2)) + edge)[:, None]
    lo, hi = lo - pad, hi + pad
    total = 0
    for w in range(0, x.shape[0], 64):
        xs = x[w:w + 64][moving[w:w + 64]]
        inside = np.all((xs[:, None, :] >= lo[None]) & (xs[:, None, :] <= hi[None]), axis=2)  # (lanes, triangles)
        total += int(inside.any(axis=0).sum())
    return total


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("cell_order", [True, False])
def test_the_index_visits_no_more_than_the_model_allows(cell_order, math_mode):
    """1536 regular triangles, no slow lane: every wave walks its lanes' cell lists only.  (Checked on the CPU: the model is
    0.21-0.23 of waves * T in cell order and 0.34 in host order at edge 0.125.)"""
    pos, vel = tc._fast_particles()
    v, nr = tc._two_boxes()
    tri, normal, coord, point, _k, want_x, want_v, moved = tc._two_boxes_reference()
    edge = 0.125
    eng = _indexed(pos, vel, v, nr, R2, math_mode, edge=edge, cell_order=cell_order)
    assert eng.get_option("collide_index_entries") >= 1536
    order = eng.download_ids()
    assert np.array_equal(order, np.arange(1000)) != cell_order
    model, waves, T = _visit_model(order, pos, vel, v, R2, edge), 16, 1536
    for what in ("query", "pass"):
        if what == "query":
            gtri, gnormal, gcoord, gpoint = eng.collider_query()
            assert np.array_equal(gtri, tri) and _same(gnormal, normal) and _same(gcoord, coord) and _same(gpoint, point)
        else:
            eng.collide()
            assert _same(eng.download("positions"), want_x) and _same(eng.download("velocities"), want_v)
            assert eng.get_option("collide_hits") == int(moved.sum())
        visits, full = eng.get_option("collide_visits"), eng.get_option("collide_full_waves")
        print(f"{what}, cell order {cell_order}: visits {visits:.0f} = {visits / (waves * T):.3f} of waves * T, "
              f"model {model} = {model / (waves * T):.3f}")
        assert 0 <= visits <= model
        assert full == 0
        assert model <= waves * T / 2
    eng.close()


# ---- 3. a curved mesh ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sphere():
    from dieselfluid_amd import scenes
    v, n = scenes.icosphere_mesh((0.05, -0.1, 0.0), 0.7, 3)
    v.setflags(write=False)
    n.setflags(write=False)
    return v, n


@functools.lru_cache(maxsize=None)
def _sphere_reference():
    pos, vel = tc._particles()
    v, nr = _sphere()
    out = cr.collide(pos, vel, v, nr, DT, 0.1) + cr.respond(pos, vel, v, nr, DT, 0.1, REST)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("cell_order", [False, True])
def test_an_icosphere_of_five_chunks(cell_order, math_mode):
    """1280 triangles, none axis-aligned, every one regular (test_collide_index_cpu): the particles of test_gpu_collider,
    slow lanes included, r = 0.1"""
    pos, vel = tc._particles()
    v, nr = _sphere()
    assert v.shape[0] == 1280
    tri, normal, coord, point, k, want_x, want_v, moved = _sphere_reference()
    per_chunk = np.bincount(tri[tri >= 0] // 256, minlength=5)
    receding = (tri >= 0) & (k < 0)
    print(f"collide {int(np.sum(tri >= 0))} of 1000, per chunk {per_chunk}, moved {int(moved.sum())}, receding {int(receding.sum())}")
    assert 0.05 <= np.mean(tri >= 0) <= 0.95 and np.all(per_chunk >= 1)
    assert moved.sum() >= 1 and receding.sum() >= 1
    for edge in (0.0, 0.125):
        eng = _indexed(pos, vel, v, nr, 0.1, math_mode, edge=edge, cell_order=cell_order)
        assert eng.get_option("collide_index_entries") >= 1280
        _check_query_and_pass(eng, (tri, normal, coord, point), (want_x, want_v, moved), (cell_order, edge))
        eng.close()


# ---- 4. corners ------------------------------------------------------------------------------------------------------

def _against_numpy(pos, vel, verts, normals, r, math_mode, **kw):
    ref = cr.collide(pos, vel, verts, normals, DT, r)
    eng = _indexed(pos, vel, verts, normals, r, math_mode, **kw)
    out = _check_query_and_pass(eng, ref[:4], cr.respond(pos, vel, verts, normals, DT, r, REST), kw)
    return eng, ref, out


@pytest.mark.parametrize("T", [300, 12])
def test_a_moving_particle_far_outside_the_index_grid(T):
    """at (3, 3, 3), alone in its wave's corner of space: no regular candidates; against a mesh with irregular triangles
    (it still meets the always-list, as the reference does) and against one without"""
    pos, vel = (a.copy() for a in tc._fast_particles())
    pos[5], vel[5] = (3.0, 3.0, 3.0), (0.3, -0.2, 0.1)
    pos[70], vel[70] = (-3.5, 3.0, 0.0), (0.0, -0.4, 0.0)
    for cell_order in (False, True):
        eng, ref, _ = _against_numpy(pos, vel, *tc._mesh(T), R, EXACT, cell_order=cell_order)
        assert np.any(ref[0] >= 0)
        eng.close()
    # alone: a handle of one particle, outside the grid
    eng, ref, (visits, _full) = _against_numpy(pos[5:6], vel[5:6], *tc._mesh(T), R, EXACT)
    print(f"T = {T}: the lone particle's wave loaded {visits:.0f} records, hit {ref[0][0]}")
    assert (1 <= visits <= 22) if T == 300 else visits == 0, visits  # the always-list (22 irregular triangles) and nothing else
    eng.close()


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_a_mesh_of_irregular_triangles_only(math_mode):
    """normals zeroed: every triangle is on the always-list and collides anywhere in its prism"""
    pos, vel = tc._particles()
    v, nr = tc._mesh(12)
    eng, ref, _ = _against_numpy(pos, vel, v, np.zeros_like(nr), R, math_mode)
    assert eng.get_option("collide_index_entries") == 12 and np.any(ref[0] >= 0)
    eng.close()


def test_one_triangle():
    pos, vel = tc._particles()
    v, nr = tc._mesh(12)
    for t in (0, 11):
        eng, ref, _ = _against_numpy(pos, vel, v[t:t + 1], nr[t:t + 1], R, EXACT)
        assert eng.get_option("collider_triangles") == 1 and np.any(ref[0] == 0)
        eng.close()


def test_free_fall_onto_a_floor_of_two_large_triangles_with_the_index_on():
    """test_gpu_collider's free fall, 200 steps: two triangles four units wide get a handful of cells from the library's
    choice of edge, and the steps equal the numpy loop bit for bit"""
    from dieselfluid_amd import SPHEngine, scenes
    rng = np.random.default_rng(2024)
    g = np.linspace(-0.5, 0.4, 10).astype(f32)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(f32)
    pos = (pos + rng.uniform(-0.01, 0.01, pos.shape).astype(f32)).astype(f32)
    vel = np.tile(np.array([0.3, 0, 0], dtype=f32), (1000, 1))
    verts, normals = scenes.quad_mesh((-2, -1.5, -2), (2, -1.5, -2), (2, -1.5, 2), (-2, -1.5, 2), (0, 1, 0))
    want = tc._free_fall_numpy(pos, vel, verts, normals, 200, (200,))
    p, _ = scenes.reference_scene(10)
    p.math_mode = EXACT
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.upload("forces", np.tile(np.array([0, -9.81, 0], dtype=f32), (1000, 1)))
    eng.set_option("collide_index", 1)
    eng.set_collider_mesh(verts, normals, 0.1, 0.5)
    cells, entries = eng.get_option("collide_index_cells"), eng.get_option("collide_index_entries")
    print(f"floor: {cells:.0f} cells of edge {eng.get_option('collide_index_edge'):.4f}, {entries:.0f} entries")
    assert 0 < cells <= 64 and 2 <= entries <= 2 * cells
    eng.wcsph_step(200)
    assert eng.get_option("collide_visits") >= 0
    gx, gv = eng.download("positions"), eng.download("velocities")
    assert _same(gx, want[200][0]) and _same(gv, want[200][1])
    assert int(np.sum(gx[:, 1] < -1.5)) == 0
    eng.close()


# ---- 5. life cycle ---------------------------------------------------------------------------------------------------

def _started(math_mode=EXACT):
    pos, vel = tc._fast_particles()
    eng, _p = _engine(1000, math_mode)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    return eng


def _index_shape(eng):
    return tuple(eng.get_option(k) for k in ("collide_index_cells", "collide_index_entries", "collide_index_edge"))


def test_the_index_follows_option_mesh_and_edge():
    a, b = _started(), _started()
    base = a.get_option("device_bytes")
    # a handle that never touches the new options
    assert a.get_option("collide_index") == 0 and _index_shape(a) == (0, 0, 0) and a.get_option("collide_visits") == -1
    b.set_collider_mesh(*tc._two_boxes(), R2, REST)
    b.collide()
    assert b.get_option("collide_index") == 0 and _index_shape(b) == (0, 0, 0) and b.get_option("collide_visits") == -1
    b.close()
    b = _started()
    # the option before the mesh, and after it: the same index
    a.set_option("collide_index", 1)
    assert _index_shape(a) == (0, 0, 0)  # nothing to index yet
    a.set_collider_mesh(*tc._two_boxes(), R2, REST)
    b.set_collider_mesh(*tc._two_boxes(), R2, REST)
    with_mesh = b.get_option("device_bytes")
    b.set_option("collide_index", 1)
    big = _index_shape(a)
    assert big == _index_shape(b) and big[0] > 1 and big[1] >= 1536 and big[2] > 0
    assert a.get_option("device_bytes") > with_mesh  # the index is counted
    # the edge after the mesh: rebuilt
    b.set_option("collide_index_edge", 0.25)
    assert _index_shape(b)[2] == 0.25 and _index_shape(b)[0] != big[0]
    b.set_option("collide_index_edge", 0)
    assert _index_shape(b) == big
    # mesh replaced: cells and entries follow
    a.set_collider_mesh(*tc._mesh(300), R, REST)
    small = _index_shape(a)
    assert small != big and small[1] >= 300
    b.set_collider_mesh(*tc._mesh(300), R, REST)
    assert _index_shape(b) == small
    # the option off: the index goes, the list walk runs
    b.set_option("collide_index", 0)
    assert _index_shape(b) == (0, 0, 0)
    b.collide()
    assert b.get_option("collide_visits") == -1 and b.get_option("collide_full_waves") == -1
    # mesh removed
    a.collide()
    assert a.get_option("collide_visits") >= 0
    a.set_collider_mesh(None)
    assert _index_shape(a) == (0, 0, 0) and a.get_option("collide_visits") == -1
    assert a.get_option("collide_index") == 1  # the option stays for the next mesh
    assert base < a.get_option("device_bytes") == with_mesh  # the index's bytes are gone (the mesh's arrays and `hits` stay)
    a.close()
    b.close()


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_a_removed_mesh_leaves_no_trace_with_the_index_on(math_mode):
    pos, vel = tc._particles()
    a, c = (tc._started(math_mode, with_mesh=False) for _ in range(2))
    a.set_option("collide_index", 1)
    a.set_collider_mesh(*tc._mesh(300), R, REST)
    assert a.get_option("collide_index_cells") > 0
    a.set_collider_mesh(None)
    assert a.get_option("collide_index_cells") == 0 and a.get_option("collide_visits") == -1
    a.wcsph_step(10)
    c.wcsph_step(10)
    assert all(_same(x, y) for x, y in zip(tc._state(a), tc._state(c)))
    a.close()
    c.close()


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_cull_off_means_the_list_walk(math_mode):
    """DSL_OPT_COLLIDE_CULL = 0 keeps meaning "every pair is tested": the index is not used, the bits are the same"""
    pos, vel = tc._fast_particles()
    tri, normal, coord, point, _k, want_x, want_v, moved = tc._two_boxes_reference()
    eng = _indexed(pos, vel, *tc._two_boxes(), R2, math_mode, cell_order=True)
    eng.set_option("collide_cull", 0)
    gtri, gnormal, gcoord, gpoint = eng.collider_query()
    assert eng.get_option("collide_visits") == -1
    assert np.array_equal(gtri, tri) and _same(gnormal, normal) and _same(gcoord, coord) and _same(gpoint, point)
    eng.collide()
    assert eng.get_option("collide_visits") == -1 and eng.get_option("collide_index_cells") > 0
    assert _same(eng.download("positions"), want_x) and _same(eng.download("velocities"), want_v)
    assert eng.get_option("collide_hits") == int(moved.sum())
    eng.close()


def test_an_edge_outside_the_budget_is_refused_and_changes_nothing():
    from dieselfluid_amd import DslError
    from dieselfluid_amd._lib import load_library
    L = load_library()
    eng = _started()
    eng.set_option("collide_index", 1)
    eng.set_option("collide_index_edge", 0.125)
    eng.set_collider_mesh(*tc._two_boxes(), R2, REST)
    before = _index_shape(eng)
    assert before[0] > 0 and before[2] == 0.125
    opt = eng.OPTIONS["collide_index_edge"]
    for bad, word in ((1e-4, b"budget"), (1e-3, b"budget"), (-1.0, b"budget"), (float("nan"), b"budget"), (float("inf"), b"budget")):
        assert L.dsl_set_option(eng._h, opt, C.c_double(bad)) == -1, bad  # DSL_ERR_INVALID
        text = L.dsl_last_error(eng._h)
        assert word in text and b"2^22" in text, (bad, text)
        assert _index_shape(eng) == before and eng.get_option("collide_index") == 1, bad
    with pytest.raises(DslError, match="budget"):
        eng.set_option("collide_index_edge", 1e-4)
    # ... and the index that stayed is whole
    tri, normal, coord, point, _k, want_x, want_v, moved = tc._two_boxes_reference()
    _check_query_and_pass(eng, (tri, normal, coord, point), (want_x, want_v, moved), "after the refusals")
    eng.close()


# ---- 6. the step drivers ---------------------------------------------------------------------------------------------

def _dam(math_mode, index):
    from dieselfluid_amd import SPHEngine, scenes
    p, pos = scenes.dambreak_scene(16, math_mode=math_mode)
    vel = (np.array([1, 0, 0], dtype=f32)[None, :] + helpers.seeded_velocities(4096, 0.05, seed=5)).astype(f32)
    verts, normals = scenes.box_mesh((0.5, 0.6, 0.5), (0.25, 1.2, 0.25), 8)
    assert verts.shape[0] == 768
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.reset_forces()
    eng.set_option("collide_index", index)
    eng.set_collider_mesh(verts, normals, 0.5 * float(p.h), 0.0)
    assert (eng.get_option("collide_index_cells") > 0) == bool(index)
    return eng


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("driver,steps,every", [("wcsph", 30, 5), ("pcisph", 5, 1)])
def test_the_step_drivers_with_the_index_equal_those_without(driver, steps, every, math_mode):
    """a pillar of 768 triangles in the 4096-particle dam break, the block moving into it at (1, 0, 0) plus noise (the
    first pass alone moves 128 particles, by collider_ref on the CPU): single steps, index on = index off, bit for bit"""
    a, b = _dam(math_mode, 1), _dam(math_mode, 0)
    hits = [0, 0]
    for s in range(1, steps + 1):
        for k, e in enumerate((a, b)):
            getattr(e, driver + "_step")(1)
            hits[k] += int(e.get_option("collide_hits"))
        if s % every == 0:
            assert all(_same(x, y) for x, y in zip(tc._state(a), tc._state(b))), s
    print(f"{driver}: {hits[0]} particles moved by the collider in {steps} steps")
    assert hits[0] == hits[1] and hits[0] > 0
    assert a.get_option("collide_visits") >= 0 and b.get_option("collide_visits") == -1
    a.close()
    b.close()
