"""GPU: the volume collider (include/dslsph.h: dsl_collider_set_volume, the volume branch of dsl_collide_pass,
dsl_collider_volume_query; csrc/sdf.hip: k_collide_volume) against tests/sdf_ref.py, the numpy float32 restatement of its
build-defined rule.  One arithmetic in both math modes: every check is an equality, bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers
import sdf_cases as sc
import sdf_ref
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = 0, 1
ORIGIN, STEP, DIMS = (-0.6, -0.55, -0.45), (0.1, 0.1, 0.1), (12, 11, 9)
CENTER, SPHERE_R = np.array([-0.05, -0.05, -0.05]), 0.3
RADIUS = 0.05
N = 1000


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _sphere_volume(origin, step, dims, center, r):
    x, y, z = (a.astype(np.float64) for a in sdf_ref.axes(origin, step, dims))
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return (np.sqrt((xx - center[0]) ** 2 + (yy - center[1]) ** 2 + (zz - center[2]) ** 2) - r).astype(f32)


@functools.lru_cache(maxsize=None)
def _volume():
    """an analytic sphere computed on the host, one voxel NaN (next to the surface: its eight cells hold particles)"""
    vol = _sphere_volume(ORIGIN, STEP, DIMS, CENTER, SPHERE_R)
    vol[4, 5, 8] = np.nan
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def _particles():
    """1000 particles = 15 waves and a 40-lane tail: a seeded cloud over the lattice and a margin around it (inside the sphere,
    within RADIUS of it, outside, outside the lattice); the first 64 sit on cell faces (a lattice coordinate in one, two or all
    three axes, the lattice's first and last planes among them), the next 32 in the cells of the last index."""
    rng = np.random.default_rng(99)
    ax = sdf_ref.axes(ORIGIN, STEP, DIMS)
    lo = np.array([a[0] for a in ax]) - 0.08
    hi = np.array([a[-1] for a in ax]) + 0.08
    pos = rng.uniform(lo, hi, (N, 3)).astype(f32)
    for k in range(64):
        for a in range(3):
            if (k >> a) & 1 or k % 8 == 0:
                pos[k, a] = ax[a][rng.integers(0, DIMS[a])]
    pos[0] = [ax[0][0], ax[1][0], ax[2][0]]
    pos[1] = [ax[0][-1], ax[1][-1], ax[2][-1]]
    pos[2] = [ax[0][-2], ax[1][-2], ax[2][-2]]
    for k in range(64, 96):
        for a in range(3):
            pos[k, a] = ax[a][-2] + f32(rng.uniform(0.0, 0.0999))
    vel = helpers.seeded_velocities(N, 0.5, seed=7).copy()
    vel[::10] = 0  # (a particle at rest collides too: the rule needs no ray)
    pos.setflags(write=False)
    vel.setflags(write=False)
    return pos, vel


def _engine(n, math_mode):
    from dieselfluid_amd import SPHEngine, scenes
    p, _ = scenes.reference_scene(10)  # h = 1, m = 1, dt = 0.01, grid box [-4, 4]^3
    p.n_particles = n
    p.math_mode = math_mode
    return SPHEngine(p, device=0)


def _check_query_and_pass(eng, vol, origin, step, rest, dev_volume=None, unsigned=False):
    pos, vel = _particles()
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.nn()  # slots in cell order, as the step drivers have them
    if dev_volume is None:
        eng.set_collider_volume(vol, origin, step, radius=RADIUS, restitution=rest, unsigned=unsigned)
    else:
        eng.set_collider_volume(None, origin, step, dims=vol.shape[::-1], radius=RADIUS, restitution=rest, unsigned=unsigned,
                                dev_volume=dev_volume)
    assert eng.get_option("collider_volume") == vol.size
    want_d, want_n = sdf_ref.collider_query(vol, origin, step, pos)
    got_d, got_n = eng.collider_volume_query()
    assert _same(got_d, want_d) and _same(got_n, want_n)
    assert _same(eng.download("positions"), pos) and _same(eng.download("velocities"), vel)  # the query does not respond
    want_x, want_v, hit = sdf_ref.collider_pass(vol, origin, step, pos, vel, RADIUS, rest)
    eng.collide()
    assert _same(eng.download("positions"), want_x) and _same(eng.download("velocities"), want_v)
    assert eng.get_option("collide_hits") == int(hit.sum())
    return hit


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("rest", [0.0, 0.5])
@pytest.mark.parametrize("unsigned", [False, True])
def test_query_and_pass_equal_the_reference_bit_for_bit(math_mode, rest, unsigned):
    vol = _volume() if not unsigned else np.abs(_volume())
    pos, vel = _particles()
    cell, d, g, mag = sdf_ref.collider_eval(vol, ORIGIN, STEP, pos)
    # the cloud covers the cases: no cell (outside, or the NaN corner), inside the sphere, within RADIUS, outside it
    assert 50 < (~cell).sum() and np.isnan(d[~cell]).any() and not cell[1] and cell[0] and cell[2] and cell[64:96].all()
    if not unsigned:
        assert (d[cell] < 0).sum() > 20 and ((d[cell] >= 0) & (d[cell] < f32(RADIUS))).sum() > 20 and (d[cell] >= f32(RADIUS)).sum() > 100
    eng = _engine(N, math_mode)
    hit = _check_query_and_pass(eng, vol, ORIGIN, STEP, rest, unsigned=unsigned)
    assert 40 < hit.sum() < cell.sum()
    eng.close()


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_a_volume_made_on_the_device_is_a_collider(math_mode):
    """dsl_mesh_distance_volume of the icosphere into device memory, handed over as dev_volume: the library's copy is what the
    reference computes from the same mesh"""
    import torch
    eng = _engine(N, math_mode)
    origin, dims = (-0.9, -0.85, -0.5), sc.DIMS  # the shared lattice, moved so that the sphere sits in the cloud
    shift = np.array(origin, dtype=f32) - np.array(sc.origin(), dtype=f32)
    verts = (sc.mesh("ico1") + shift[None, None, :]).astype(f32)
    vol = sdf_ref.volume(verts, origin, sc.STEP, dims, band=0.25)
    buf = torch.zeros(vol.size, dtype=torch.float32, device="cuda")
    eng.mesh_distance_volume(verts, origin, sc.STEP, dims, band=0.25, dev_out=buf.data_ptr())
    hit = _check_query_and_pass(eng, vol, origin, sc.STEP, 0.5, dev_volume=buf.data_ptr())
    assert hit.sum() > 20
    buf.zero_()  # the library owns a copy: the caller's array may go
    torch.cuda.synchronize()
    assert _same(eng.collider_volume_query()[0], sdf_ref.collider_query(vol, origin, sc.STEP, eng.download("positions"))[0])
    eng.close()


# ---- the step drivers ----
DAM_C, DAM_R = np.array([1.0, 0.2, 0.5]), 0.25  # a sphere at the foot of the dam-break block [0, 1]^3, half in it
DAM_O, DAM_S, DAM_D = (0.6, -0.2, 0.1), (0.05, 0.05, 0.05), (17, 17, 17)


def _dam(math_mode):
    from dieselfluid_amd import SPHEngine, scenes
    p, pos = scenes.dambreak_scene(12, math_mode=math_mode)
    frc = np.tile(np.array(p.force_reset[:], dtype=f32), (pos.shape[0], 1))
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.upload("forces", frc)
    return eng, p, pos, frc


def test_wcsph_steps_are_the_oracle_step_followed_by_the_reference_pass():
    vol = _sphere_volume(DAM_O, DAM_S, DAM_D, DAM_C, DAM_R)
    eng, p, pos, frc = _dam(EXACT)
    radius, rest = 0.5 * float(p.h), 0.3
    eng.set_collider_volume(vol, DAM_O, DAM_S, radius=radius, restitution=rest)
    plain, _p, _pos, _frc = _dam(EXACT)
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, force=frc)
    total = 0
    for step in range(5):
        eng.wcsph_step(1)
        plain.wcsph_step(1)
        ora.wcsph_step(1)
        x, v, hit = sdf_ref.collider_pass(vol, DAM_O, DAM_S, ora.positions(), ora.velocities(), radius, rest)
        ora.set_positions(x)
        ora.set_velocities(v)
        assert _same(eng.download("positions"), x) and _same(eng.download("velocities"), v), step
        assert eng.get_option("collide_hits") == int(hit.sum())
        total += int(hit.sum())
        if step == 0:  # dsl_stats stay what Update saw
            assert eng.stats().max_vel == plain.stats().max_vel and eng.stats().max_f == plain.stats().max_f
    assert total > 20
    assert not _same(eng.download("positions"), plain.download("positions"))
    eng.close()
    plain.close()


def test_one_pcisph_step_is_the_oracle_step_followed_by_the_reference_pass():
    vol = _sphere_volume(DAM_O, DAM_S, DAM_D, DAM_C, DAM_R)
    eng, p, pos, frc = _dam(EXACT)
    radius, rest = 0.5 * float(p.h), 0.3
    eng.set_collider_volume(vol, DAM_O, DAM_S, radius=radius, restitution=rest)
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, force=frc)
    ora.delta = p.delta
    eng.pcisph_begin()
    ora.pcisph_begin()
    eng.pcisph_step(1)
    ora.pcisph_step(1)
    x, v, hit = sdf_ref.collider_pass(vol, DAM_O, DAM_S, ora.positions(), ora.velocities(), radius, rest)
    assert hit.sum() > 5
    assert _same(eng.download("positions"), x) and _same(eng.download("velocities"), v)
    # the predictor state is not touched
    assert _same(eng.download("pci_positions"), ora.pci_positions()) and _same(eng.download("pci_velocities"), ora.pci_velocities())
    assert eng.get_option("collide_hits") == int(hit.sum())
    eng.close()


def test_no_skin_step_while_a_volume_is_set():
    from dieselfluid_amd import SPHEngine, scenes
    p, pos = scenes.dambreak_scene(16, math_mode=FAST)
    vol = _sphere_volume(DAM_O, DAM_S, DAM_D, DAM_C, DAM_R)
    counts = {}
    for with_volume in (True, False):
        eng = SPHEngine(p, device=0)
        eng.upload("positions", pos)
        eng.reset_forces()
        eng.set_option("skin", 0.07)
        if with_volume:
            eng.set_collider_volume(vol, DAM_O, DAM_S, radius=0.5 * p.h)
        eng.wcsph_step(4)
        counts[with_volume] = eng.get_option("skin_steps")
        eng.close()
    assert counts[True] == 0 and counts[False] > 0


# ---- exclusion, removal, refusals ----
def test_a_mesh_and_a_volume_exclude_each_other_and_a_removed_volume_leaves_no_trace():
    from dieselfluid_amd import DslError, scenes
    pos, vel = _particles()
    verts, normals = scenes.box_mesh((0.05, -0.1, 0.0), (1.3, 1.1, 1.2))
    eng, ref = _engine(N, FAST), _engine(N, FAST)
    for e in (eng, ref):
        e.upload("positions", pos)
        e.upload("velocities", vel)
    # a volume, then a mesh
    eng.set_collider_volume(_volume(), ORIGIN, STEP, radius=RADIUS)
    with pytest.raises(DslError, match="exclude each other"):
        eng.set_collider_mesh(verts, normals, 0.1, 0.0)
    assert eng.get_option("collider_volume") == _volume().size and eng.get_option("collider_triangles") == 0
    eng.set_collider_mesh(None)  # removing a mesh that is not there is no conflict
    # removal by dims = NULL; then the mesh is accepted, and the volume refused
    eng.set_collider_volume(None)
    assert eng.get_option("collider_volume") == 0
    eng.set_collider_mesh(verts, normals, 0.1, 0.0)
    with pytest.raises(DslError, match="exclude each other"):
        eng.set_collider_volume(_volume(), ORIGIN, STEP, radius=RADIUS)
    assert eng.get_option("collider_triangles") == 12 and eng.get_option("collider_volume") == 0
    eng.set_collider_mesh(None)
    # nothing is set: ten steps are those of a handle that never had a collider, and nothing runs under DSL_K_COLLIDE
    eng.timing_enable(1)
    eng.wcsph_step(10)
    ref.wcsph_step(10)
    eng.collide()
    assert _same(eng.download("positions"), ref.download("positions")) and _same(eng.download("velocities"), ref.download("velocities"))
    assert eng.timing("collide")[1] == 0 and eng.timing("density")[1] == 10
    d, n = eng.collider_volume_query()
    assert not d.any() and not n.any()
    # ... and with a volume every step launches one
    eng.set_collider_volume(_volume(), ORIGIN, STEP, radius=RADIUS)
    eng.wcsph_step(2)
    assert eng.timing("collide")[1] == 2
    eng.close()
    ref.close()


def test_slab_handles_and_bad_arguments_are_refused():
    pos, vel = _particles()
    vol = np.ascontiguousarray(_volume())
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def call(eng, dev=None, host=vol, origin=ORIGIN, step=STEP, dims=DIMS, flags=0):
        o = (C.c_float * 3)(*origin) if origin is not None else None
        s = (C.c_float * 3)(*step) if step is not None else None
        d = (C.c_int32 * 3)(*dims) if dims is not None else None
        return eng._L.dsl_collider_set_volume(eng._h, C.c_void_p(dev), fp(host) if host is not None else None, o, s, d,
                                              C.c_float(RADIUS), C.c_float(0.0), flags)

    eng = _engine(N, FAST)
    eng.upload("positions", pos)
    eng.slab_config(0, -0.5, 0.5)
    assert call(eng) == -4 and b"slab" in eng._L.dsl_last_error(eng._h)  # DSL_ERR_UNSUPPORTED
    assert call(eng, dims=None) == -4
    eng.close()
    eng = _engine(N, FAST)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    bad = [dict(host=None), dict(dev=vol.ctypes.data), dict(origin=None), dict(step=None), dict(dims=(1, 11, 9)), dict(dims=(12, 11, 1)),
           dict(dims=(2048, 1024, 1024)), dict(step=(0.1, 0.0, 0.1)), dict(step=(0.1, float("nan"), 0.1)),
           dict(origin=(float("inf"), 0.0, 0.0)), dict(flags=4)]
    for kw in bad:
        assert call(eng, **kw) == -1 and b"dsl_collider_set_volume" in eng._L.dsl_last_error(eng._h), kw
    assert eng.get_option("collider_volume") == 0
    assert call(eng) == 0
    for kw in bad:  # a refused call leaves the volume that was set
        assert call(eng, **kw) == -1, kw
    assert eng.get_option("collider_volume") == vol.size
    assert eng._L.dsl_slab_config(eng._h, 0, C.c_float(-0.5), C.c_float(0.5)) == -4
    assert b"volume collider" in eng._L.dsl_last_error(eng._h)
    hit = sdf_ref.collider_pass(vol, ORIGIN, STEP, pos, vel, RADIUS, 0.0)[2]
    eng.collide()
    assert eng.get_option("collide_hits") == int(hit.sum())
    eng.close()
