"""GPU: the triangle-mesh collider (include/dslsph.h: dsl_collider_set_mesh, dsl_collide_pass, dsl_collider_query;
csrc/kernels_collide.hpp) against tests/collider_ref.py, the numpy float32 restatement of Mesh.Collision
(geom/mesh/mesh.go:41-57, geom/triangle/tri.go:37-101) that tests/test_collider_cpu.py checks by hand.

A collision is a classification, so the collider has ONE arithmetic in both math modes and every check here is an
equality, bit for bit."""
import functools

import numpy as np
import pytest

import collider_ref as cr
import helpers

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = 0, 1
DT, R, REST = 0.01, 0.15, 0.5


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _engine(n, math_mode, n3=10):
    from dieselfluid_amd import SPHEngine, scenes
    p, _ = scenes.reference_scene(n3)  # h = 1, m = 1, dt = 0.01, grid box [-4, 4]^3
    p.n_particles = n
    p.math_mode = math_mode
    return SPHEngine(p, device=0), p


@functools.lru_cache(maxsize=None)
def _particles():
    """1000 particles = 15 waves and a 40-lane tail: the jittered [-1,1)^3 lattice with seeded velocities; every tenth
    particle stands still (Mag(V) == 0), every tenth moves exactly horizontally (n.V == 0 against the horizontal faces:
    the 0.0001 substitute).  Twenty particles (402, 412 .. 592) move slower than 1e-4: the broad phase stands down in
    THEIR waves -- four of the sixteen in host order -- and works in the others."""
    pos = helpers.jittered_lattice(10, 0.3, seed=4321)
    vel = helpers.seeded_velocities(1000, 0.5, seed=77).copy()
    vel[::10] = 0
    vel[1::10, 1] = 0
    vel[402:600:10] *= f32(1e-4)
    pos.setflags(write=False)
    vel.setflags(write=False)
    return pos, vel


@functools.lru_cache(maxsize=None)
def _mesh(T):
    """T = 12: a box.  T = 300 (two chunks of 256, the second partial): the same box, 50 triangles per face, with
    overlapping duplicates (100..119 repeat 0..19 and must never win), a degenerate triangle (150: b == a), normals that
    are not unit (200..209), normals in the triangle's own plane (210..219) and InitMesh's zero normal on the last one."""
    from dieselfluid_amd import scenes
    v, n = scenes.box_mesh((0.05, -0.1, 0.0), (1.3, 1.1, 1.2), 1 if T == 12 else 5)
    v, n = v.copy(), n.copy()
    assert v.shape[0] == T
    if T == 300:
        v[100:120], n[100:120] = v[0:20], n[0:20]
        v[150, 1] = v[150, 0]
        n[200:210] *= f32(3.0)
        n[210:220] = n[210:220][:, [1, 2, 0]]
        n[299] = 0
    v.setflags(write=False)
    n.setflags(write=False)
    return v, n


def _slow(vel):
    """the lanes that switch the broad phase off in their wave: 0 < Mag(V) < 1e-4, on the float32 sum of squares"""
    mv2 = cr._dot(vel, vel)
    return (mv2 != 0) & ~(mv2 >= f32(1.0001e-8))


def _waves_with(flag, order=None):
    """per wave of 64 slots: does it hold a particle with `flag`?  `order`: slot -> particle (None: host order)"""
    f = flag if order is None else flag[order]
    return np.array([f[w:w + 64].any() for w in range(0, f.size, 64)])


@functools.lru_cache(maxsize=None)
def _reference(T, lo, hi):
    """(tri, normal, coord, point, k) of particles lo..hi-1 against mesh T: computed once, shared, read-only"""
    pos, vel = _particles()
    v, nr = _mesh(T)
    out = cr.collide(pos[lo:hi], vel[lo:hi], v, nr, DT, R)
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1. the query, bit for bit ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("T,lo,hi", [(12, 0, 1000), (300, 0, 1000), (300, 200, 264), (300, 225, 226)])
def test_query_equals_the_reference_bit_for_bit(T, lo, hi, math_mode):
    """all 1000 particles; one wave (200..263: no slow lane, so the broad phase works; 21 of the 64 collide); one
    particle (225: it moves and collides, the single-lane wave has work to do)"""
    pos, vel = _particles()
    pos, vel, n = pos[lo:hi], vel[lo:hi], hi - lo
    v, nr = _mesh(T)
    tri, normal, coord, point, _k = _reference(T, lo, hi)
    slow = _slow(vel)
    if n == 1000:
        # the broad phase works in twelve waves and stands down in four
        assert _waves_with(slow).sum() == 4 and slow.sum() == 20
    else:
        assert not slow.any() and np.any(tri >= 0) and (n == 64 or vel.any())
    if T == 300 and n == 1000:
        # between 5 % and 95 % of the particles collide (180 of 1000 with these seeds, chosen against collider_ref on the
        # CPU), every kind of triangle is among the winners except the duplicates, and every kind of particle is hit
        frac = float(np.mean(tri >= 0))
        print(f"colliding fraction {frac:.3f}")
        assert 0.05 <= frac <= 0.95
        assert not np.any((tri >= 100) & (tri < 120)) and np.any(tri < 20)
        assert np.any(tri == 299) and np.any((tri >= 200) & (tri < 220)) and not np.any(tri == 150)
        assert np.all(tri[::10] == -1) and np.any(tri[1::10] >= 0) and np.any(tri[slow] >= 0)
    eng, _p = _engine(n, math_mode)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.set_collider_mesh(v, nr, R, REST)
    assert eng.get_option("collider_triangles") == T and eng.get_option("collide_cull") == 1
    for cull in (1, 0):
        eng.set_option("collide_cull", cull)
        gtri, gnormal, gcoord, gpoint = eng.collider_query()
        assert np.array_equal(gtri, tri), (cull, np.flatnonzero(gtri != tri)[:8])
        assert _same(gnormal, normal) and _same(gcoord, coord) and _same(gpoint, point), cull
    # the query answers, it does not respond
    assert _same(eng.download("positions"), pos) and _same(eng.download("velocities"), vel)
    eng.close()


def test_query_after_a_neighbour_build_is_in_host_order():
    """the kernel walks the cell-sorted slots; the four returns come back in the order of the upload"""
    pos, vel = _particles()
    v, nr = _mesh(300)
    tri, normal, coord, point, _k = _reference(300, 0, 1000)
    eng, _p = _engine(1000, EXACT)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.nn()
    order = eng.download_ids()
    assert not np.array_equal(order, np.arange(1000))
    with_slow = _waves_with(_slow(vel), order)
    assert 0 < with_slow.sum() < with_slow.size  # the broad phase works in some waves of this order, not in all
    eng.set_collider_mesh(v, nr, R, REST)
    gtri, gnormal, gcoord, gpoint = eng.collider_query()
    assert np.array_equal(gtri, tri) and _same(gnormal, normal) and _same(gcoord, coord) and _same(gpoint, point)
    eng.close()


# ---- 1b. the broad phase at work: a regular mesh of six chunks, cell-sorted waves, no slow lane -----------------------

R2 = 0.1


@functools.lru_cache(maxsize=None)
def _two_boxes():
    """1536 triangles = six chunks of 256, every one regular (unit normal, perpendicular to its triangle): two small
    boxes (scenes.box_mesh, subdiv 8: 768 triangles, a pair of opposite faces per chunk) in opposite corners of the
    particle block.  A wave near the second box skips chunks 0..2 by their box and collides with triangles >= 768."""
    from dieselfluid_amd import scenes
    va, na = scenes.box_mesh((0.55, 0.55, 0.55), (0.5, 0.5, 0.5), 8)
    vb, nb = scenes.box_mesh((-0.55, -0.55, -0.55), (0.5, 0.5, 0.5), 8)
    v, n = np.concatenate([va, vb]), np.concatenate([na, nb])
    assert v.shape == (1536, 3, 3)
    v.setflags(write=False)
    n.setflags(write=False)
    return v, n


@functools.lru_cache(maxsize=None)
def _fast_particles():
    """_particles() without the slow lanes: standing still or faster than 1e-4, so the broad phase works in every wave"""
    pos, vel = _particles()
    vel = helpers.seeded_velocities(1000, 0.5, seed=77).copy()
    vel[::10] = 0
    vel[1::10, 1] = 0
    assert not _slow(vel).any()
    vel.setflags(write=False)
    return pos, vel


@functools.lru_cache(maxsize=None)
def _two_boxes_reference():
    pos, vel = _fast_particles()
    v, nr = _two_boxes()
    out = cr.collide(pos, vel, v, nr, DT, R2) + cr.respond(pos, vel, v, nr, DT, R2, REST)
    for a in out:
        a.setflags(write=False)
    return out


def _skipped_chunks(order, pos, vel, verts, r):
    """(waves, chunks) bool: the wave's box -- over its lanes that move, in slot order `order` -- lies outside the
    chunk's box.  The chunk's box here is its vertices' box inflated by 2.2 r + 2 % of its extents + 2e-5 of its largest
    coordinate: more than the kernel's pad on any of its triangles (2.1 r + 1 % + 1e-5), so what lies outside this box
    lies outside the kernel's, and the kernel skips it (all triangles are regular)."""
    x = pos[order]
    moving = cr._dot(vel, vel)[order] != 0
    q = verts.reshape(-1, 256, 9).reshape(-1, 768, 3)
    lo, hi = q.min(axis=1), q.max(axis=1)
    pad = (2.2 * r + 0.02 * (hi - lo).sum(axis=1) + 2e-5 * np.abs(q).max(axis=(1, 2)))[:, None]
    lo, hi = lo - pad, hi + pad
    out = []
    for w in range(0, x.shape[0], 64):
        xs = x[w:w + 64][moving[w:w + 64]]
        wlo, whi = xs.min(axis=0), xs.max(axis=0)
        out.append(np.any((whi[None, :] < lo) | (wlo[None, :] > hi), axis=1))
    return np.array(out)


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_cull_on_equals_cull_off_on_a_regular_mesh_of_six_chunks(math_mode):
    """DSL_OPT_COLLIDE_CULL 1 = 0 = collider_ref, query and response, where the broad phase does all it can: every
    triangle regular, no slow lane in any wave, slots in cell order.  Checked on the CPU first: waves lie outside chunk
    boxes (chunks past the first among them), a wave that skips chunks collides in a later one, and particles collide
    with triangles of every chunk."""
    pos, vel = _fast_particles()
    v, nr = _two_boxes()
    tri, normal, coord, point, k, want_x, want_v, moved = _two_boxes_reference()
    # regular: |n| = 1 and n perpendicular to both edges, exactly, on every triangle
    assert np.all(cr._dot(nr, nr) == 1) and np.all(cr._dot(nr, v[:, 1] - v[:, 0]) == 0) and np.all(cr._dot(nr, v[:, 2] - v[:, 0]) == 0)
    print(f"collide {int(np.sum(tri >= 0))} of 1000, per chunk {np.bincount(tri[tri >= 0] // 256, minlength=6)}, moved {int(moved.sum())}")
    assert np.all(np.bincount(tri[tri >= 0] // 256, minlength=6) >= 1)  # (37 collide: 6 6 7 7 5 6 per chunk)
    assert moved.sum() >= 1 and np.sum((tri >= 0) & (k < 0)) >= 1       # (19 moved, 18 receding)
    got = {}
    for cull in (1, 0):
        eng, _p = _engine(1000, math_mode)
        eng.upload("positions", pos)
        eng.upload("velocities", vel)
        eng.nn()  # slots in cell order, as the step drivers have them: a wave is spatially compact
        if cull:
            order = eng.download_ids()
            skip = _skipped_chunks(order, pos, vel, v, R2)
            print(f"(wave, chunk) pairs skipped by the chunk's box: {int(skip.sum())} of {skip.size}; per chunk {skip.sum(axis=0)}")
            assert skip[:, 1:].any() and not skip.all(axis=0).any()  # every chunk: skipped by some waves, walked by others
            late = np.array([np.any(tri[order[w:w + 64]] >= 768) for w in range(0, 1000, 64)])
            assert np.any(skip[:, :3].all(axis=1) & late)  # skips the first box's three chunks, collides with the second
        eng.set_collider_mesh(v, nr, R2, REST)
        eng.set_option("collide_cull", cull)
        gtri, gnormal, gcoord, gpoint = eng.collider_query()
        assert np.array_equal(gtri, tri), (cull, np.flatnonzero(gtri != tri)[:8])
        assert _same(gnormal, normal) and _same(gcoord, coord) and _same(gpoint, point), cull
        eng.collide()
        got[cull] = (eng.download("positions"), eng.download("velocities"), eng.get_option("collide_hits"))
        eng.close()
    for cull in (1, 0):
        assert _same(got[cull][0], want_x) and _same(got[cull][1], want_v) and got[cull][2] == int(moved.sum()), cull


# ---- 2. the response -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("cull", [1, 0])
def test_collide_pass_equals_the_numpy_response(math_mode, cull):
    pos, vel = _particles()
    v, nr = _mesh(300)
    tri, _n, _c, _pt, k = _reference(300, 0, 1000)
    want_x, want_v, moved = cr.respond(pos, vel, v, nr, DT, R, REST)
    receding = (tri >= 0) & (k < 0)
    assert receding.sum() >= 1 and moved.sum() >= 1  # (80 and 100 with these seeds)
    eng, _p = _engine(1000, math_mode)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.nn()  # slots in cell order, as the step drivers have them
    eng.set_collider_mesh(v, nr, R, REST)
    eng.set_option("collide_cull", cull)
    eng.collide()
    gx, gv = eng.download("positions"), eng.download("velocities")
    assert _same(gx, want_x) and _same(gv, want_v)
    # a receding hit is left exactly as it was; an approaching one has moved
    assert _same(gx[receding], pos[receding]) and _same(gv[receding], vel[receding])
    assert not np.any(np.all(gx[moved] == pos[moved], axis=1))
    assert eng.get_option("collide_hits") == int(moved.sum())
    eng.close()


# ---- 3. the step drivers ---------------------------------------------------------------------------------------------

def _started(math_mode, with_mesh=True):
    pos, vel = _particles()
    eng, p = _engine(1000, math_mode)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    if with_mesh:
        eng.set_collider_mesh(*_mesh(300), R, REST)
    return eng


def _state(eng):
    return [eng.download(k) for k in ("positions", "velocities")]


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_wcsph_step_runs_the_collide_pass_after_update(math_mode):
    """dsl_wcsph_step(1) with a mesh = build_neighbours, density_pass, force_pass, collide_pass.  (The step and the pass
    sequence launch the same kernels on the same slot order in both math modes, so FAST is held to bits as well.)"""
    a, b, c = _started(math_mode), _started(math_mode), _started(math_mode, with_mesh=False)
    a.wcsph_step(1)
    for e in (b, c):
        e.nn()
        e.density_all()
        e.force_pass()
    after_update = _state(c)
    assert not _same(_state(b)[0], _state(a)[0])  # dsl_force_pass stays one to one: no collide pass yet
    assert all(_same(x, y) for x, y in zip(_state(b), after_update))
    b.collide()
    assert all(_same(x, y) for x, y in zip(_state(a), _state(b)))
    # ... and it is the numpy response to the state Update left
    want_x, want_v, moved = cr.respond(*after_update, *_mesh(300), DT, R, REST)
    assert moved.sum() >= 1
    assert _same(_state(a)[0], want_x) and _same(_state(a)[1], want_v)
    assert a.get_option("collide_hits") == int(moved.sum())
    # dsl_stats stay what Update saw
    assert a.stats().max_vel == c.stats().max_vel and a.stats().max_f == c.stats().max_f
    assert a.timing("collide")[1] == 0  # (timing off: nothing recorded)
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_pcisph_step_runs_the_collide_pass_after_update(math_mode):
    """dsl_pcisph_step(1) with a mesh = the four phases, DSL_PCI_END_STEP running the collide pass after Update = the four
    phases of a handle without a mesh plus a collide pass."""
    a, b, c = _started(math_mode), _started(math_mode), _started(math_mode, with_mesh=False)
    iters = int(a.params.pci_max_iters)
    a.pcisph_step(1)
    for e in (b, c):
        e.pcisph_begin()
        e.pcisph_phase(0)
        for _ in range(iters):
            e.pcisph_phase(1)
            e.pcisph_phase(2)
        e.pcisph_phase(3)
    assert all(_same(x, y) for x, y in zip(_state(a), _state(b)))
    assert not _same(_state(c)[0], _state(a)[0])
    c.set_collider_mesh(*_mesh(300), R, REST)
    c.collide()
    assert all(_same(x, y) for x, y in zip(_state(a), _state(c)))
    # the predictor state is not touched
    for k in ("pci_positions", "pci_velocities"):
        assert _same(a.download(k), c.download(k))
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_a_removed_mesh_leaves_no_trace(math_mode):
    """after dsl_collider_set_mesh(T = 0) ten steps equal those of a handle that never had a mesh, bit for bit"""
    a, c = _started(math_mode), _started(math_mode, with_mesh=False)
    a.set_collider_mesh(None)
    assert a.get_option("collider_triangles") == 0
    tri, *_ = a.collider_query()
    assert np.all(tri == -1)
    a.timing_enable(1)
    a.wcsph_step(10)
    c.wcsph_step(10)
    assert all(_same(x, y) for x, y in zip(_state(a), _state(c)))
    assert a.timing("collide")[1] == 0 and a.timing("density")[1] == 10  # no collide kernel without a mesh
    a.collide()  # nothing to do
    assert all(_same(x, y) for x, y in zip(_state(a), _state(c)))
    a.close()
    c.close()


# ---- 4. free fall onto a floor ---------------------------------------------------------------------------------------

def _free_fall_numpy(pos, vel, verts, normals, steps, checkpoints):
    """The reference WCSPH loop (wcsph.go:14-26) in numpy float32: no pressure force, double gravity -- Update's force is
    force_reset + external = (0, -9.81, 0) + (0, -9.81, 0) -- with Update as in test_wcsph_free_fall_known_answer
    (a = F * (1/m), v += a dt, x += v dt; m = 1), then the collider's response."""
    x, v = pos.copy(), vel.copy()
    F = np.array([0, f32(-9.81) + f32(-9.81), 0], dtype=f32)
    dt = f32(DT)
    out = {}
    for s in range(1, steps + 1):
        a = F * f32(1.0)
        v = v + (a * dt)[None, :]
        x = x + v * dt
        x, v, _ = cr.respond(x, v, verts, normals, DT, 0.1, 0.5)
        if s in checkpoints:
            out[s] = (x.copy(), v.copy())
    return out


def test_free_fall_onto_a_floor_against_numpy():
    """1000 particles fall, drifting along x, onto a floor of two triangles at y = -1.5 (r = 0.1, e = 0.5).  After 200 and
    400 steps EXACT positions and velocities equal the numpy loop bit for bit and nobody is below the floor (the numpy
    loop alone: 0 of 1000 below at both points, lowest particle at y = -1.46379 / -1.47870)."""
    from dieselfluid_amd import SPHEngine, scenes
    rng = np.random.default_rng(2024)
    g = np.linspace(-0.5, 0.4, 10).astype(f32)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(f32)
    pos = (pos + rng.uniform(-0.01, 0.01, pos.shape).astype(f32)).astype(f32)
    vel = np.tile(np.array([0.3, 0, 0], dtype=f32), (1000, 1))
    verts, normals = scenes.quad_mesh((-2, -1.5, -2), (2, -1.5, -2), (2, -1.5, 2), (-2, -1.5, 2), (0, 1, 0))
    assert verts.shape == (2, 3, 3)
    want = _free_fall_numpy(pos, vel, verts, normals, 400, (200, 400))
    p, _ = scenes.reference_scene(10)  # grid box [-4, 4]^3 covers the scene: x drifts to 1.6, y stops at the floor
    p.math_mode = EXACT
    assert p.dt == f32(DT) and p.mass == 1 and not p.wcsph_pressure_force and not p.wcsph_viscosity and not p.walls
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.upload("forces", np.tile(np.array([0, -9.81, 0], dtype=f32), (1000, 1)))  # the state after sph.Init
    eng.set_collider_mesh(verts, normals, 0.1, 0.5)
    for steps in (200, 400):
        eng.wcsph_step(200)
        gx, gv = eng.download("positions"), eng.download("velocities")
        wx, wv = want[steps]
        below = int(np.sum(gx[:, 1] < -1.5))
        print(f"step {steps}: min y {gx[:, 1].min():.4f} (numpy {wx[:, 1].min():.4f}), below the floor {below}")
        assert _same(gx, wx) and _same(gv, wv)
        assert below == 0 and int(np.sum(wx[:, 1] < -1.5)) == 0
    eng.close()


# ---- 5. restrictions -------------------------------------------------------------------------------------------------

def test_no_skin_step_while_a_mesh_is_set():
    from dieselfluid_amd import SPHEngine, scenes
    p, pos = scenes.dambreak_scene(16, math_mode=FAST)
    verts, normals = scenes.box_mesh((2.0, 0.25, 0.5), (0.5, 0.5, 0.5))
    counts = {}
    for with_mesh in (True, False):
        eng = SPHEngine(p, device=0)
        eng.upload("positions", pos)
        eng.reset_forces()
        eng.set_option("skin", 0.07)
        if with_mesh:
            eng.set_collider_mesh(verts, normals, 0.5 * p.h, 0.0)
        eng.wcsph_step(4)
        counts[with_mesh] = eng.get_option("skin_steps")
        eng.close()
    assert counts[True] == 0
    assert counts[False] > 0  # (the same handle without a mesh does take them: the mesh is what holds them back)


def test_slab_handles_and_bad_arguments_are_refused():
    from dieselfluid_amd import DslError
    from dieselfluid_amd._lib import load_library
    import ctypes as C
    L = load_library()
    pos, vel = _particles()
    v, nr = _mesh(12)
    eng, _p = _engine(1000, FAST)
    eng.upload("positions", pos)
    eng.slab_config(0, -0.5, 0.5)
    with pytest.raises(DslError, match="slab"):
        eng.set_collider_mesh(v, nr, R, REST)
    vv, nn = np.ascontiguousarray(v).reshape(-1), np.ascontiguousarray(nr).reshape(-1)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.dsl_collider_set_mesh(eng._h, fp(vv), fp(nn), 12, C.c_float(R), C.c_float(REST)) == -4  # DSL_ERR_UNSUPPORTED
    assert b"slab" in L.dsl_last_error(eng._h)
    eng.close()
    eng, _p = _engine(1000, FAST)
    eng.upload("positions", pos)
    eng.set_collider_mesh(v, nr, R, REST)
    assert L.dsl_slab_config(eng._h, 0, C.c_float(-0.5), C.c_float(0.5)) == -4
    assert b"collider" in L.dsl_last_error(eng._h)
    assert L.dsl_collider_set_mesh(eng._h, None, fp(nn), 12, C.c_float(R), C.c_float(REST)) == -1  # DSL_ERR_INVALID
    assert L.dsl_collider_set_mesh(eng._h, fp(vv), None, 12, C.c_float(R), C.c_float(REST)) == -1
    assert eng.get_option("collider_triangles") == 12  # a refused call leaves the mesh that was set
    eng.close()
