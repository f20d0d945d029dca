"""Parameter sets the dam-break and reference parity tests never reach, against the CPU oracle: one WCSPH force term
without the other, the running-mass viscosity in the fused step, an attracting pressure sign, wall restitution,
per-particle forces (the first step after an upload reads them per slot and the sort carries them), and the unordered
counting sort (dsl_params.sort_unordered).

Yardsticks, as in tests/test_gpu_parity.py: DSL_MATH_EXACT bit for bit against the oracle's DSLO_ORDER_CELL sums;
DSL_MATH_FAST to test_wcsph_dambreak_10_steps' tolerances (positions 2e-6 relative, velocities
helpers.fast_velocity_tolerance, densities 2e-5); one FAST step against helpers.brute_force_step_f64 to
test_full_size_16m_properties' float64 tolerances (a).  Every test first shows, with the oracle alone, that the switch it
covers moves the result by more than the tolerance it is checked to."""
import numpy as np
import pytest

import helpers
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

EXACT, FAST = 0, 1
N3 = 16
TOL_X, TOL_RHO = 2e-6, 2e-5


def _scene(math_mode, G=1, V=1, **kw):
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(N3, math_mode=math_mode, **kw)
    p.wcsph_pressure_force, p.wcsph_viscosity = G, V
    return p, pos


def _seeded_vel(p, n=N3 ** 3, frac=0.03):
    """test_skin_steps_match_the_oracle_over_reuse_and_rebuild's velocities: |v| dt up to ~0.012 h per step, so that a
    skin of 0.1 rebuilds at least twice in 10 steps"""
    return helpers.seeded_velocities(n, scale=frac * float(np.sqrt(p.eos_w / p.mass)))


def _reset_field(p, n=N3 ** 3):
    return np.tile(np.array(p.force_reset[:], dtype=np.float32), (n, 1))


def _force_field(p, n=N3 ** 3, seed=17):
    """force_reset + m g U(-1,1)^3, a different vector on every particle"""
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))
    return (_reset_field(p, n).astype(np.float64) + float(p.mass) * 9.81 * u).astype(np.float32)


def _engine(p, pos, vel=None, skin=0.0, force=None):
    from dieselfluid_amd import SPHEngine
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    if vel is not None:
        eng.upload("velocities", vel)
    if force is None:
        eng.reset_forces()
    else:
        eng.upload("forces", force)
    eng.set_option("skin", skin)
    return eng


def _oracle(p, pos, vel=None, steps=0, force=None):
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, vel=vel,
                                  force=_reset_field(p, pos.shape[0]) if force is None else force)
    if steps:
        ora.wcsph_step(steps)
    return ora


def _stat_tols(p, steps):
    """Absolute bounds on |stats().max_vel - oracle| and |stats().max_f - oracle| in DSL_MATH_FAST.  Both are running
    maxima of per-particle magnitudes, and |max_i |a_i| - max_i |b_i|| <= max_i |a_i - b_i|, so they inherit the
    per-particle bounds: max_vel the velocity bound of the step it was taken at (helpers.fast_velocity_tolerance, at
    most `steps` steps); max_f the force behind one step's velocity error, m / dt times the model's full one-step
    velocity bound (2 x fast_velocity_tolerance(p, 1), the helper asserts half its model).  On the 16^3 dam-break
    these are 7.9e-4 m/s (3e-4 to 4e-4 of max_vel) and 0.055 N (1e-4 to 4e-4 of max_f).  Without the pressure force the model
    has nothing to amplify and max_f gets 2e-5 relative, the densities' bar: every other term is a float32 sum of the
    density's kind (same pairs, one more rcp)."""
    tol_v = helpers.fast_velocity_tolerance(p, steps)
    tol_f = 2.0 * float(p.mass) * helpers.fast_velocity_tolerance(p, 1) / float(p.dt)
    return tol_v, tol_f


def _fast_errs(x, v, rho, ora):
    return (helpers.rel_err(x, ora.positions()), float(np.abs(v.astype(np.float64) - ora.velocities()).max()),
            helpers.rel_err(rho, ora.densities()))


def _check(eng, ora, p, steps):
    """positions, velocities, densities and the maxVel / maxF statistics against the oracle"""
    x, v, rho = eng.download("positions"), eng.download("velocities"), eng.download("densities")
    st = eng.stats()
    if p.math_mode == EXACT:
        for got, want in ((x, ora.positions()), (v, ora.velocities()), (rho, ora.densities())):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert st.max_vel == np.float32(ora.max_vel) and st.max_f == np.float32(ora.max_f), \
            (st.max_vel, ora.max_vel, st.max_f, ora.max_f)
        return
    ex, ev, er = _fast_errs(x, v, rho, ora)
    assert ex < TOL_X and ev < helpers.fast_velocity_tolerance(p, steps) and er < TOL_RHO, (ex, ev, er)
    tol_v, tol_f = _stat_tols(p, steps)
    if not p.wcsph_pressure_force:
        tol_f = TOL_RHO * float(ora.max_f)
    assert abs(st.max_vel - ora.max_vel) <= tol_v, (st.max_vel, ora.max_vel, tol_v)
    assert abs(st.max_f - ora.max_f) <= tol_f, (st.max_f, ora.max_f, tol_f)


def _guard(p, ora, ora_flipped, steps):
    """the flipped switch moves the oracle's result by more than the tolerance the run is checked to"""
    dx = helpers.rel_err(ora_flipped.positions(), ora.positions())
    dv = float(np.abs(ora_flipped.velocities().astype(np.float64) - ora.velocities()).max())
    assert dx > TOL_X or dv > helpers.fast_velocity_tolerance(p, steps), (dx, dv)


def _check_brute_force(p, x, v, x1, v1, force=None):
    """one step of every particle against helpers.brute_force_step_f64, tolerances (a) of test_full_size_16m_properties"""
    n = x.shape[0]
    allp = np.arange(n)
    want_rho, want_x, want_v = helpers.brute_force_step_f64(p, x, v, allp, allp, force=force)
    assert np.isfinite(want_x).all() and np.isfinite(want_v).all()
    x64, v64 = x.astype(np.float64), v.astype(np.float64)
    dx_want, dx_got = want_x - x64, x1.astype(np.float64) - x64
    assert np.abs(dx_got - dx_want).max() < 1e-3 * np.abs(dx_want).max() + 2e-7 * np.abs(want_x).max()
    dv_want, dv_got = want_v - v64, v1.astype(np.float64) - v64
    assert np.abs(dv_got - dv_want).max() < 1e-3 * np.abs(dv_want).max()


def _flipped(p, **kw):
    q = type(p).from_buffer_copy(p)
    for k, val in kw.items():
        setattr(q, k, val)
    return q


# ---- A: one force term without the other -----------------------------------------------------------------------------

TERMS = [(1, 0), (0, 1)]
PATHS = ["fast", "fast_skin", "exact", "fast_xsph", "exact_xsph", "fast_queue", "fast_skin_queue"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("G,V", TERMS)
def test_one_force_term_without_the_other(G, V, path):
    """(pressure, viscosity) = (1, 0) and (0, 1) take instantiations of their own at every launch site: the FAST
    tiled kernel (with and without the XSPH / cohesion variant), the skin step's list kernel, the EXACT tiled kernel --
    and the mask walk and the list walk once more with their tiles drawn from the tile queue (tile_queue = 2: the queue
    is a template argument of both).  10 steps of the 16^3 dam-break with seeded velocities."""
    mode = EXACT if path.startswith("exact") else FAST
    p, pos = _scene(mode, G, V)
    vel = _seeded_vel(p)
    steps = 10
    if path.endswith("xsph"):
        # (test_xsph_and_surface_tension_terms' kappa of 40 drives these velocities to 30-60 m/s in 10 steps: 0.5 keeps
        # the flow as gentle as the plain runs, and each term still moves the result by far more than the tolerance)
        p.xsph_eps, p.st_kappa = 0.25, 0.5
        ora = _oracle(p, pos, vel, steps)
        _guard(p, ora, _oracle(_flipped(p, xsph_eps=0.0), pos, vel, steps), steps)
        _guard(p, ora, _oracle(_flipped(p, st_kappa=0.0), pos, vel, steps), steps)
    else:
        ora = _oracle(p, pos, vel, steps)
    # the term that is off must matter: the oracle with both terms on differs
    _guard(p, ora, _oracle(_flipped(p, wcsph_pressure_force=1, wcsph_viscosity=1), pos, vel, steps), steps)
    skin = path.startswith("fast_skin")
    eng = _engine(p, pos, vel, skin=0.1 if skin else 0.0)
    if path.endswith("queue"):
        eng.set_option("tile_queue", 2)
    eng.wcsph_step(steps)
    if skin:
        assert eng.get_option("skin_steps") == steps and eng.get_option("skin_rebuilds") >= 2
        assert eng.get_option("skin_list_overflow") == 0
    else:
        assert eng.get_option("skin_steps") == 0
    _check(eng, ora, p, steps)
    eng.close()


@pytest.mark.parametrize("mode", [FAST, EXACT])
def test_attracting_pressure_sign(mode):
    """pressure_sign = +1 (the reference's fluid.go:168-169) with the pressure force on, both terms on.  The pressure
    pulls compressed particles together and the block collapses -- the oracle's maxVel doubles every step from step 3
    on (3 m/s after 3 steps, 850 after 10) --, so the run is 3 steps long: past that no float32 pair can agree"""
    p, pos = _scene(mode)
    p.pressure_sign = 1.0
    vel = _seeded_vel(p)
    steps = 3
    ora = _oracle(p, pos, vel, steps)
    _guard(p, ora, _oracle(_flipped(p, pressure_sign=-1.0), pos, vel, steps), steps)
    eng = _engine(p, pos, vel)
    eng.wcsph_step(steps)
    _check(eng, ora, p, steps)
    eng.close()


@pytest.mark.parametrize("G,V,sign", [(1, 0, -1.0), (0, 1, -1.0), (1, 1, 1.0)])
def test_one_fast_step_against_float64(G, V, sign):
    """one FAST step of every particle of the seeded 16^3 dam-break against the float64 brute force"""
    p, pos = _scene(FAST, G, V)
    p.pressure_sign = sign
    vel = _seeded_vel(p)
    eng = _engine(p, pos, vel)
    eng.wcsph_step(1)
    _check_brute_force(p, pos, vel, eng.download("positions"), eng.download("velocities"))
    eng.close()


# ---- B: the running-mass viscosity in the fused step ------------------------------------------------------------------

@pytest.mark.parametrize("path", ["fast", "fast_skin", "exact"])
@pytest.mark.parametrize("G", [1, 0])
def test_running_mass_with_unit_mass(G, path):
    """visc_running_mass = 1 with m = 1 (rho_phys = 16^3): the product (force + t) * m is the plain sum bit for bit,
    and the FAST step takes the tiled kernels and the skin step (which never apply it)"""
    mode = EXACT if path == "exact" else FAST
    p, pos = _scene(mode, G, 1, rho_phys=float(N3 ** 3))
    assert p.mass == 1.0
    p.visc_running_mass = 1
    vel = _seeded_vel(p)
    steps = 10
    ora = _oracle(p, pos, vel, steps)
    _guard(p, ora, _oracle(_flipped(p, wcsph_viscosity=0), pos, vel, steps), steps)
    eng = _engine(p, pos, vel, skin=0.1 if path == "fast_skin" else 0.0)
    eng.wcsph_step(steps)
    assert eng.get_option("skin_steps") == (steps if path == "fast_skin" else 0)
    _check(eng, ora, p, steps)
    eng.close()


@pytest.mark.parametrize("mode", [FAST, EXACT])
@pytest.mark.parametrize("G", [1, 0])
def test_running_mass_with_the_dambreak_mass(G, mode):
    """visc_running_mass = 1 with m != 1: FAST takes the lane-per-particle kernel, EXACT the tiled kernel that applies
    the product itself; the skin option is ignored (it needs the tiled kernels)"""
    p, pos = _scene(mode, G, 1)
    assert p.mass != 1.0
    p.visc_running_mass = 1
    vel = _seeded_vel(p)
    steps = 10
    ora = _oracle(p, pos, vel, steps)
    _guard(p, ora, _oracle(_flipped(p, visc_running_mass=0), pos, vel, steps), steps)
    eng = _engine(p, pos, vel, skin=0.1 if mode == FAST else 0.0)
    eng.wcsph_step(steps)
    assert eng.get_option("skin_steps") == 0
    _check(eng, ora, p, steps)
    eng.close()


@pytest.mark.parametrize("G", [1, 0])
def test_running_mass_unit_mass_against_float64(G):
    p, pos = _scene(FAST, G, 1, rho_phys=float(N3 ** 3))
    p.visc_running_mass = 1
    vel = _seeded_vel(p)
    eng = _engine(p, pos, vel)
    eng.wcsph_step(1)
    _check_brute_force(p, pos, vel, eng.download("positions"), eng.download("velocities"))
    eng.close()


# ---- C: walls with restitution ----------------------------------------------------------------------------------------

WALL_STEPS = 5


def _wall_scene(mode):
    """the dam-break block expanding from its centre at up to 20 m/s: its outer layers (0.5 dx from the planes x = 0,
    y = 0, z = 0 and z = L) cross them within 5 steps (0.07 m of travel), restitution 0.5"""
    p, pos = _scene(mode)
    p.restitution = 0.5
    centre = np.float32(0.5)
    vel = ((pos - centre) * np.float32(40.0)).astype(np.float32)
    return p, pos, vel


def test_wall_scene_reflects_on_several_planes():
    """the oracle itself: the wall planes that clamp particles in 5 steps (x = 0, y = 0, z = 0, z = L), and the velocity
    it leaves them points away from the wall"""
    p, pos, vel = _wall_scene(FAST)
    ora = _oracle(p, pos, vel)
    hit = set()
    for _ in range(WALL_STEPS):
        ora.wcsph_step(1)
        x, v = ora.positions(), ora.velocities()
        for a in range(3):
            for side, plane in ((0, p.box_min[a]), (1, p.box_max[a])):
                at = x[:, a] == np.float32(plane)
                if not at.any():
                    continue
                hit.add((a, side))
                # reflected: away from the wall (restitution 0 would leave 0 here)
                assert np.all(v[at, a] > 0) if side == 0 else np.all(v[at, a] < 0)
    assert len(hit) >= 3 and (2, 1) in hit, hit
    ora0 = _oracle(_flipped(p, restitution=0.0), pos, vel, WALL_STEPS)
    _guard(p, _oracle(p, pos, vel, WALL_STEPS), ora0, WALL_STEPS)


@pytest.mark.parametrize("path", ["fast", "fast_skin", "exact"])
def test_walls_with_restitution(path):
    mode = EXACT if path == "exact" else FAST
    p, pos, vel = _wall_scene(mode)
    ora = _oracle(p, pos, vel, WALL_STEPS)
    eng = _engine(p, pos, vel, skin=0.1 if path == "fast_skin" else 0.0)
    eng.wcsph_step(WALL_STEPS)
    assert eng.get_option("skin_steps") == (WALL_STEPS if path == "fast_skin" else 0)
    _check(eng, ora, p, WALL_STEPS)
    eng.close()


def test_walls_with_restitution_against_float64():
    """the step in which the outer layer reaches the walls, from the oracle's state two steps in"""
    p, pos, vel = _wall_scene(FAST)
    ora = _oracle(p, pos, vel, 2)
    x, v = ora.positions().copy(), ora.velocities().copy()
    eng = _engine(p, x, v)
    eng.wcsph_step(1)
    x1, v1 = eng.download("positions"), eng.download("velocities")
    at_wall = (x1 == 0.0).any(axis=1) | (x1[:, 2] == np.float32(p.box_max[2]))
    assert at_wall.sum() > 100
    _check_brute_force(p, x, v, x1, v1)
    eng.close()


# ---- D: per-particle forces -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("path", ["fast", "fast_skin", "exact"])
def test_per_particle_forces(path, steps):
    """An uploaded field, a different vector on every particle: the first step reads it per slot after the sort has
    carried it (the three force arrays in the scatter), Update resets it to force_reset, and a skin engine takes that
    first step as a plain one."""
    mode = EXACT if path == "exact" else FAST
    p, pos = _scene(mode)
    vel = _seeded_vel(p)
    frc = _force_field(p)
    ora = _oracle(p, pos, vel, steps, force=frc)
    _guard(p, ora, _oracle(p, pos, vel, steps), steps)
    eng = _engine(p, pos, vel, skin=0.1 if path == "fast_skin" else 0.0, force=frc)
    assert np.array_equal(eng.download("forces"), frc)
    eng.wcsph_step(steps)
    assert eng.get_option("skin_steps") == (steps - 1 if path == "fast_skin" else 0)
    _check(eng, ora, p, steps)
    assert np.array_equal(eng.download("forces"), _reset_field(p))
    eng.close()


def test_per_particle_forces_against_float64():
    p, pos = _scene(FAST)
    vel = _seeded_vel(p)
    frc = _force_field(p)
    eng = _engine(p, pos, vel, force=frc)
    eng.wcsph_step(1)
    _check_brute_force(p, pos, vel, eng.download("positions"), eng.download("velocities"), force=frc)
    eng.close()


def test_force_upload_in_the_middle_of_a_skin_run():
    """4 skin steps, a new field, 4 more: the step after the upload is a plain one (it reads the field), the rest are
    skin steps again; the skin engine, its twin without a skin and the oracle agree"""
    p, pos = _scene(FAST)
    vel = _seeded_vel(p)
    frc = _force_field(p, seed=23)
    ora = _oracle(p, pos, vel, 4)
    ora.set_forces(frc)
    ora.wcsph_step(4)
    ora0 = _oracle(p, pos, vel, 8)
    _guard(p, ora, ora0, 8)
    a = _engine(p, pos, vel, skin=0.1)
    b = _engine(p, pos, vel, skin=0.0)
    for eng in (a, b):
        eng.wcsph_step(4)
        eng.upload("forces", frc)
        eng.wcsph_step(1)
    assert a.get_option("skin_steps") == 4
    a.wcsph_step(3); b.wcsph_step(3)
    assert a.get_option("skin_steps") == 7 and b.get_option("skin_steps") == 0
    _check(a, ora, p, 8)
    _check(b, ora, p, 8)
    assert helpers.rel_err(a.download("positions"), b.download("positions")) < TOL_X
    assert np.abs(a.download("velocities").astype(np.float64) - b.download("velocities")).max() < \
        2 * helpers.fast_velocity_tolerance(p, 8)
    a.close(); b.close()


# ---- E: the unordered sort --------------------------------------------------------------------------------------------

def _permuted(pos, vel=None, seed=5):
    perm = np.random.default_rng(seed).permutation(pos.shape[0])  # ids unrelated to the position in the lattice
    return pos[perm].copy(), (None if vel is None else vel[perm].copy())


def _some_cell_out_of_id_order(eng):
    """the guard of the unordered sort: after nn(), at least one cell is not ascending in particle id"""
    eng.nn()
    ids, cs = eng.download_ids(), eng.download_cell_start()
    cell_of_slot = np.repeat(np.arange(cs.size - 1), np.diff(cs))
    same_cell = cell_of_slot[1:] == cell_of_slot[:-1]
    return bool(np.any(np.diff(ids)[same_cell] < 0))


@pytest.mark.parametrize("h_over_dx", [2.0, 5.0])
@pytest.mark.parametrize("mode", [FAST, EXACT])
def test_unordered_sort_invariants(mode, h_over_dx):
    """after nn(): the slot map is a permutation, cell_start a prefix table of the cells' counts, and the particle in
    every slot lies in that slot's cell (floor((x - grid_min) / h), the device's rule)"""
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(N3, math_mode=mode, h_over_dx=h_over_dx)
    if h_over_dx > 2.0:
        p.dt = p.dt * 0.2
    p.sort_unordered = 1
    pos, _ = _permuted(pos)
    eng = _engine(p, pos)
    eng.wcsph_step(3)
    assert _some_cell_out_of_id_order(eng)  # (nn() inside)
    n = eng.n
    ids, cs = eng.download_ids(), eng.download_cell_start()
    assert np.array_equal(np.sort(ids), np.arange(n))
    st = eng.stats()
    assert cs.size == st.grid_cells + 1 and cs[0] == 0 and cs[-1] == n and np.all(np.diff(cs) >= 0)
    assert (np.diff(cs).max() > 32) == (h_over_dx > 2.0)
    assert np.diff(cs).max() == st.max_cell_count
    spos = eng.download("positions", sorted_order=True)
    assert np.array_equal(spos, eng.download("positions")[ids])
    dims = np.array(st.grid_dims[:])
    inv = np.float32(1.0) / np.float32(p.h)
    gmin = np.array(p.grid_min[:], dtype=np.float32)
    c = np.clip(np.floor((spos - gmin) * inv).astype(np.int64), 0, dims - 1)
    cell = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    cell_of_slot = np.repeat(np.arange(cs.size - 1), np.diff(cs))
    assert np.array_equal(cell, cell_of_slot)
    eng.close()


@pytest.mark.parametrize("path", ["fast", "fast_skin", "exact"])
def test_unordered_sort_wcsph_steps(path):
    """10 WCSPH steps (plain, skin, EXACT) with unordered cells against the oracle: FAST tolerances in both math modes,
    the sums no longer run in the oracle's order"""
    mode = EXACT if path == "exact" else FAST
    p, pos = _scene(mode)
    p.sort_unordered = 1
    pos, vel = _permuted(pos, _seeded_vel(p))
    steps = 10
    ora = _oracle(p, pos, vel, steps)
    eng = _engine(p, pos, vel, skin=0.1 if path == "fast_skin" else 0.0)
    eng.wcsph_step(steps)
    assert eng.get_option("skin_steps") == (steps if path == "fast_skin" else 0)
    q = _flipped(p, math_mode=FAST)
    x, v, rho = eng.download("positions"), eng.download("velocities"), eng.download("densities")
    ex, ev, er = _fast_errs(x, v, rho, ora)
    assert ex < TOL_X and ev < helpers.fast_velocity_tolerance(q, steps) and er < TOL_RHO, (ex, ev, er)
    tol_v, tol_f = _stat_tols(q, steps)
    st = eng.stats()
    assert abs(st.max_vel - ora.max_vel) <= tol_v and abs(st.max_f - ora.max_f) <= tol_f
    assert _some_cell_out_of_id_order(eng)
    eng.close()


@pytest.mark.parametrize("binning", [0, 1])
@pytest.mark.parametrize("mode", [FAST, EXACT])
def test_unordered_sort_pcisph_steps(mode, binning):
    """test_pcisph_steps' set-up and FAST tolerance (2e-4) with unordered cells, both math modes"""
    from dieselfluid_amd import SPHEngine, scenes
    n3, tol = 12, 2e-4
    p, _ = scenes.reference_scene(n3)
    p.math_mode = mode
    p.sort_unordered = 1
    p.pci_max_iters = 5
    p.delta = 1.0e-4
    pos, vel = _permuted(helpers.jittered_lattice(n3, 0.1), helpers.seeded_velocities(n3 ** 3, 0.05))
    eng = SPHEngine(p, device=0)
    eng.pcisph_set_binning(binning)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, vel=vel)
    ora.delta = p.delta
    eng.pcisph_begin(); ora.pcisph_begin()
    for _ in range(2):
        eng.pcisph_step(1); ora.pcisph_step(1)
        st = eng.stats()
        assert st.pci_iters == ora.pci_iters
        assert abs(st.pci_max_error - ora.pci_error) <= tol * max(abs(ora.pci_error), 1e-3)
        for got, want in ((eng.download("positions"), ora.positions()), (eng.download("velocities"), ora.velocities()),
                          (eng.download("pci_positions"), ora.pci_positions()),
                          (eng.download("pci_velocities"), ora.pci_velocities())):
            assert helpers.rel_err(got, want) < tol
    assert _some_cell_out_of_id_order(eng)
    eng.close()


@pytest.mark.parametrize("mode", [FAST, EXACT])
def test_unordered_sort_carries_derived_arrays(mode):
    """the unordered twin of test_stale_densities_stay_on_their_particles: DensityAll, then nn() -- the densities move
    with their particles"""
    p, pos = _scene(mode)
    p.sort_unordered = 1
    pos, _ = _permuted(pos)
    eng = _engine(p, pos)
    eng.density_all()
    rho0 = eng.download("densities")
    assert rho0.min() > 0 and np.unique(rho0).size > 100
    for _ in range(2):
        assert _some_cell_out_of_id_order(eng)  # (nn() inside)
        assert np.array_equal(eng.download("densities"), rho0)
    eng.close()


@pytest.mark.parametrize("mode", [FAST, EXACT])
def test_unordered_sort_keeps_the_running_mass_in_id_order(mode):
    """visc_running_mass = 1 with m != 1 weights a neighbour's viscous term by m^k, k its place from the end of the sum:
    the in-cell order decides the force, so the library keeps the cells ordered for it (include/dslsph.h) -- two runs
    agree bit for bit, and the oracle (DSLO_ORDER_CELL) to the usual tolerance of the math mode"""
    p, pos = _scene(mode)
    p.visc_running_mass = 1
    p.sort_unordered = 1
    pos, vel = _permuted(pos, _seeded_vel(p))
    steps = 10
    ora = _oracle(p, pos, vel, steps)
    _guard(p, ora, _oracle(_flipped(p, visc_running_mass=0), pos, vel, steps), steps)
    runs = []
    for _ in range(2):
        eng = _engine(p, pos, vel)
        eng.wcsph_step(steps)
        runs.append((eng.download("positions"), eng.download("velocities"), eng.download("densities")))
        _check(eng, ora, p, steps)
        assert not _some_cell_out_of_id_order(eng)
        eng.close()
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
