"""GPU: dsl_field_divergence / curl / laplacian / interpolate (k_field_div_curl, k_field_laplacian, k_field_interpolate,
the k_pack1 / k_pack3 read-out) against the oracle, past the one fresh lattice of test_gpu_parity.test_field_operators.
The oracle's operators are themselves held to a float64 brute force in tests/test_field_ops_cpu.py.

  a. after real sorts: shuffled ids, an uploaded per-particle force field, 3 and 4 steps (both parities of the
     position / force / id ping-pong pairs), every operator on both tensors and both scalars
  b. an operator call leaves the run alone: a handle that called every operator between its steps ends in the bits of
     one that only downloaded positions -- plain steps in both math modes, with and without a force field uploaded
     right before the operators (Curl parks y and z in the idle half of the force pair), and out of a live skin episode
  c. boundary particles: N() rows, targets skipped, candidates with density 0 (Inf / NaN where the oracle has them)
  d. the reference's LSH neighbours (100 samples, no distance test)
  e. edges: n = 1, 2, 65; coincident particles; particles and query points outside the grid box; ~125 particles per
     cell; query sets of 0, 1 and `capacity` points
  f. the refusals of the four entry points

Tolerances.  EXACT: bit for bit, NaN where the oracle has NaN (as test_field_operators).  FAST: test_field_operators'
own -- 5e-5 of max |oracle| for Div, Curl and Interpolate(density), twice that for Laplacian(density) and for the force
tensor (Curl(forces) sums the products Div(forces) sums), eight times that for the pressure field.  One exception, in
the scenes of (a) and (e): the Laplacian subtracts nearly equal values (for n = 2 the oracle's is exactly 0), so a
relative bound can ask for more than the FAST densities give.  There helpers.field_ops_f64 computes on the CPU how far
each operator moves when every density is multiplied by 1 +- 2e-6 (seeded signs; eps_rho of
helpers.fast_velocity_tolerance, the project's FAST density error), and four times that is used where it is larger; the
test prints the tolerance it used.  On the oracle's states that exception is larger than the relative bound for
(computed on the CPU, fraction of max |oracle|):

  scene                      operator              4 x sensitivity   relative bound
  (a) 3 steps                Laplacian(pressure)   4.7e-4            4e-4
  (a) 3 steps                Interpolate(pressure) 6.8e-4            4e-4
  (a) 4 steps                Laplacian(pressure)   6.0e-4            4e-4
  (a) 4 steps                Interpolate(pressure) 9.8e-4            4e-4
  (e) coincident pairs       Laplacian(pressure)   1.8e-3            4e-4
  (e) coincident pairs       Interpolate(pressure) 1.8e-3            4e-4
  (e) outside the grid box   Interpolate(pressure) 5.7e-4            4e-4
  (e) n = 2                  Laplacian(density)    1.18 absolute     0 (the oracle's values are exactly 0)

(the pressure field is the Tait EOS just above eos_d0_grad, where (rho / d0)^7.16 - 1 loses the leading digits of rho;
the density field never needs the exception in these scenes but for n = 2).  Everywhere else the relative bound holds.

What the tests found.  (b) dsl_field_divergence / dsl_field_curl of the forces made the implicit forces explicit, and
the step driver then took a plain step where the other handle took a skin step: fixed in the host layer, the skin test
asserts equal skin step counts.  (e) two properties of the FAST DENSITY pass: densities of particles far outside the grid
box were off by up to 1.8e-4, over which test_particles_and_queries_outside_the_grid_box[FAST] failed -- fixed in the
tiled density kernels (tile_target_far); and a lone particle's density is a rounding residue, not 0, left as it is and
written up in test_tiny_and_ragged_counts.
"""
import ctypes as C

import numpy as np
import pytest

import helpers
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
EXACT, FAST = 0, 1
TOL = 5e-5
FACTOR = {"div_velocities": 1, "curl_velocities": 1, "div_forces": 2, "curl_forces": 2, "lap_densities": 2,
          "lap_pressures": 8, "int_densities": 1, "int_pressures": 8}
KEYS = tuple(FACTOR)
EPS_RHO = 2.0e-6
OTENSOR = {"velocities": "velocity", "forces": "force"}
OSCALAR = {"densities": "density", "pressures": "pressure"}


# ---- shared pieces -----------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    """bit for bit, NaN where `want` has NaN (the sign and payload of a NaN are the processor's, not the formula's)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(_bits(got)[ok], _bits(want)[ok])


def _device_ops(eng, q, keys=KEYS):
    out = {}
    for k in keys:
        op, field = k.split("_")
        if op == "div":
            out[k] = eng.field_div(field)
        elif op == "curl":
            out[k] = eng.field_curl(field)
        elif op == "lap":
            out[k] = eng.field_laplacian(field)
        else:  # (at most `capacity` query points per call)
            step = max(int(eng.capacity), 1)
            parts = [eng.field_interpolate(q[s:s + step], field) for s in range(0, q.shape[0], step)]
            out[k] = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    return out


def _oracle_ops(ora, q, keys=KEYS):
    out = {}
    for k in keys:
        op, field = k.split("_")
        if op == "div":
            out[k] = ora.field_div(OTENSOR[field])
        elif op == "curl":
            out[k] = ora.field_curl(OTENSOR[field])
        elif op == "lap":
            out[k] = ora.field_laplacian(OSCALAR[field])
        else:
            out[k] = ora.field_interpolate(q, OSCALAR[field])
    return out


def _sensitivity(p, ora, q, keys=KEYS, stride=5):
    """max |operator(rho (1 +- 2e-6)) - operator(rho)| per key, float64 on the CPU, every `stride`-th particle; the
    larger of two sign patterns, seeded and alternating"""
    x, rho = ora.positions(), ora.densities().astype(np.float64)
    sign = np.where(np.random.default_rng(3).random(rho.size) < 0.5, -1.0, 1.0)
    alternating = np.where(np.arange(rho.size) % 2 == 0, 1.0, -1.0)  # (two particles must not get the same sign)
    probe = np.arange(0, x.shape[0], stride)
    scalars = {"lap_densities": "lap_density", "lap_pressures": "lap_pressure", "int_densities": "interp_density",
               "int_pressures": "interp_pressure"}
    out = {}
    with np.errstate(all="ignore"):
        for tensor, t in (("velocities", ora.velocities()), ("forces", ora.forces())):
            src_of = {"div_" + tensor: "div", "curl_" + tensor: "curl"}
            if tensor == "velocities":
                src_of.update(scalars)
            src_of = {k: s for k, s in src_of.items() if k in keys}
            if not src_of:
                continue
            a = helpers.field_ops_f64(p, x, t, rho, probe, q)
            for sg in (sign, alternating):
                b = helpers.field_ops_f64(p, x, t, rho * (1.0 + EPS_RHO * sg), probe, q)
                for k, s in src_of.items():
                    d = np.abs(np.nan_to_num(b[s] - a[s], nan=0.0, posinf=0.0, neginf=0.0))
                    out[k] = max(out.get(k, 0.0), float(d.max()) if d.size else 0.0)
    return out


def _check(tag, math_mode, got, want, sens=None, zero_density=False):
    """EXACT: the oracle's bits.  FAST: non-finite exactly where the oracle is, elsewhere within FACTOR x 5e-5 of
    max |oracle| -- or four times the density sensitivity, where that is larger.  `zero_density`: a fluid particle of
    the scene has density exactly 0 in the oracle; where the oracle divides by it, FAST is not compared (see
    test_tiny_and_ragged_counts)"""
    missed = []
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (tag, k, g.shape, w.shape)
        if math_mode == EXACT:
            assert _same_bits(g, w), (tag, k, "EXACT: not the oracle's bits")
            continue
        ok = np.isfinite(w)
        if zero_density:
            assert np.isfinite(g[ok]).all(), (tag, k, "FAST: non-finite where the oracle is finite")
            g = np.where(ok, g, w)
        assert np.array_equal(np.isfinite(g), ok), (tag, k, "FAST: non-finite values not where the oracle has them")
        if not ok.any():
            continue
        scale = float(np.abs(w[ok]).max())
        tol = FACTOR[k] * TOL * scale
        floor = 4.0 * sens[k] if sens else 0.0
        err = float(np.abs(g[ok].astype(np.float64) - w[ok]).max())
        print(f"{tag} {k}: FAST max |device - oracle| = {err:.3e}, tolerance {max(tol, floor):.3e} "
              f"({'4 x density sensitivity' if floor > tol else 'relative'}; max |oracle| = {scale:.3e})")
        if not err <= max(tol, floor):
            missed.append((tag, k, err, max(tol, floor)))
    assert not missed, missed  # (every figure is printed before the first one fails)


def _queries(pos, lo, hi, h, seed=17, n_between=150, n_on=50):
    """points between particles, exactly on particles, and 50 more than h outside [lo, hi]^3"""
    rng = np.random.default_rng(seed)
    n = pos.shape[0]
    a = pos[:: max(n // n_between, 1)]
    between = a + ((rng.random(a.shape) - 0.5) * 0.5 * h).astype(np.float32)
    on = pos[1:: max(n // n_on, 1)]
    out = (hi + 1.5 * h + rng.random((50, 3)) * 3 * h).astype(np.float32)
    out[::2, 1] = (lo - 1.5 * h - rng.random(25) * h).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([between, on, out]), dtype=np.float32)


def _engine(p, pos, vel=None, force=None, skin=0.0):
    from dieselfluid_amd import SPHEngine
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    if vel is not None:
        eng.upload("velocities", vel)
    if force is None:
        eng.reset_forces()
    else:
        eng.upload("forces", force)
    if skin:
        eng.set_option("skin", skin)
    return eng


def _reset_field(p, n):
    return np.tile(np.array(p.force_reset[:], dtype=np.float32), (n, 1))


def _force_field(p, n, seed=17):
    """force_reset + m g U(-1,1)^3, a different vector on every particle (test_gpu_configs._force_field)"""
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3))
    return (_reset_field(p, n).astype(np.float64) + float(p.mass) * 9.81 * u).astype(np.float32)


# ---- a. developed, both parities ---------------------------------------------------------------------------------------

N3 = 16
_DEV = {}


def _developed_scene(math_mode, vel_frac=0.0):
    """the 16^3 dam-break, ids unrelated to the place in the lattice, a different force on every particle"""
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(N3, math_mode=math_mode)
    perm = np.random.default_rng(5).permutation(pos.shape[0])
    pos = np.ascontiguousarray(pos[perm])
    vel = None
    if vel_frac:
        vel = helpers.seeded_velocities(pos.shape[0], scale=vel_frac * float(np.sqrt(p.eos_w / p.mass)))
    return p, pos, vel, _force_field(p, pos.shape[0])


def _developed_oracle(steps):
    """oracle operators and density sensitivities after `steps` steps, once per step count"""
    if steps not in _DEV:
        p, pos, _, frc = _developed_scene(EXACT)
        ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, force=frc)
        ora.wcsph_step(steps)
        ora.sampler_update()  # (dsl_density_pass sorts the moved particles first; the oracle's DensityAll does not)
        ora.density_all()
        q = _queries(ora.positions(), 0.0, 1.0, float(p.h))
        _DEV[steps] = (q, _oracle_ops(ora, q), _sensitivity(p, ora, q))
        ora.close()
    return _DEV[steps]


@pytest.mark.parametrize("steps", [3, 4])
@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_operators_after_real_sorts_both_parities(math_mode, steps):
    """Results are computed in slot order and come back through ids[cur_ids]; Curl parks y and z in frc[cur_f ^ 1]; a
    step flips both.  3 and 4 steps cover both parities; the ids are shuffled, so a result left in slot order is
    wrong at almost every particle."""
    p, pos, _, frc = _developed_scene(math_mode)
    q, want, sens = _developed_oracle(steps)
    eng = _engine(p, pos, force=frc)
    eng.wcsph_step(steps)
    eng.density_all()
    ids = eng.download_ids()
    assert np.array_equal(np.sort(ids), np.arange(pos.shape[0]))
    assert np.mean(ids != np.arange(pos.shape[0])) > 0.5  # the sort really permuted
    got = _device_ops(eng, q)
    for k in KEYS:  # the comparison must be about something: most rows are non-zero
        rows = np.asarray(want[k]).reshape(len(want[k]), -1)
        assert np.mean(np.any(rows != 0, axis=1)) > 0.5, k
    _check(f"developed/{steps} steps", math_mode, got, want, sens)
    eng.close()


# ---- b. an operator call leaves the run alone ---------------------------------------------------------------------------

def _state_bits(eng):
    return [_bits(eng.download(name)) for name in ("positions", "velocities", "forces", "densities")]


@pytest.mark.parametrize("mid_upload", [False, True])
@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_an_operator_call_between_steps_changes_nothing(math_mode, mid_upload):
    """3 steps, every operator (both tensors, both scalars, 64 query points), 3 steps -- against 3 steps, a download, 3
    steps.  `mid_upload`: a new per-particle force field goes up right before the operators, so the next step reads
    the very arrays the operators' results were parked next to."""
    p, pos, _, frc = _developed_scene(math_mode)
    frc2 = _force_field(p, pos.shape[0], seed=23)
    a, b = _engine(p, pos, force=frc), _engine(p, pos, force=frc)
    a.wcsph_step(3); b.wcsph_step(3)
    if mid_upload:
        a.upload("forces", frc2); b.upload("forces", frc2)
    q = _queries(pos, 0.0, 1.0, float(p.h))[:64]
    got = _device_ops(a, q)
    assert all(np.isfinite(v).all() for v in got.values())
    b.download("positions")
    if mid_upload:
        assert np.array_equal(_bits(a.download("forces")), _bits(frc2))
        assert np.array_equal(_bits(b.download("forces")), _bits(frc2))
    a.wcsph_step(3); b.wcsph_step(3)
    for name, sa, sb in zip(("positions", "velocities", "forces", "densities"), _state_bits(a), _state_bits(b)):
        assert np.array_equal(sa, sb), name
    a.close(); b.close()


def test_an_operator_call_out_of_a_live_skin_episode():
    """FAST with DSL_OPT_SKIN: the operators arrive in the middle of a skin episode, which every entry point but the
    step driver settles first; the other handle settles through a download.  Same bits after 3 more steps.  Then the
    settled handle's operators equal those of a fresh handle given the downloaded positions and velocities."""
    p, pos, vel, frc = _developed_scene(FAST, vel_frac=0.03)
    a, b = _engine(p, pos, vel, frc, skin=0.1), _engine(p, pos, vel, frc, skin=0.1)
    a.wcsph_step(4); b.wcsph_step(4)
    assert a.get_option("skin_steps") > 0 and b.get_option("skin_steps") > 0  # skin steps are live
    q = _queries(pos, 0.0, 1.0, float(p.h))[:64]
    got = _device_ops(a, q)
    assert all(np.isfinite(v).all() for v in got.values())
    b.download("positions")
    a.wcsph_step(3); b.wcsph_step(3)
    assert a.get_option("skin_steps") == b.get_option("skin_steps") > 3
    for name, sa, sb in zip(("positions", "velocities", "forces", "densities"), _state_bits(a), _state_bits(b)):
        assert np.array_equal(sa, sb), name
    a.density_all()
    settled = _device_ops(a, q)
    c = _engine(p, a.download("positions"), a.download("velocities"))
    c.density_all()
    fresh = _device_ops(c, q)
    for k in KEYS:
        assert np.array_equal(_bits(settled[k]), _bits(fresh[k])), k
    a.close(); b.close(); c.close()


# ---- c. boundary particles ---------------------------------------------------------------------------------------------

def _plate():
    t = np.arange(-1.25, 1.25 + 1e-6, 0.25, dtype=np.float32)
    u, v = np.meshgrid(t, t, indexing="ij")
    return np.stack([u.reshape(-1), np.full(u.size, -1.25, np.float32), v.reshape(-1)], axis=-1).astype(np.float32)


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_boundary_particles_are_candidates_but_not_targets(math_mode):
    """The plate of test_boundary_particles_volume_is_field_interpolate_bit_for_bit, added after density_all: the
    operators loop over N() particles, a boundary candidate carries density 0 (m / 0 = Inf, Inf * 0 = NaN)."""
    from dieselfluid_amd import SPHEngine, scenes
    n3 = 8
    n = n3 ** 3
    p, _ = scenes.reference_scene(n3)
    p.math_mode = math_mode
    pos = helpers.jittered_lattice(n3, 0.2)
    vel = helpers.seeded_velocities(n, 0.1)
    frc = helpers.seeded_velocities(n, 5.0, seed=41)
    plate = _plate()
    p.capacity = n + plate.shape[0]
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.upload("forces", frc)
    eng.density_all()
    eng.add_boundary_particles(plate)
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, vel=vel, force=frc)
    ora.density_all()
    assert ora.add_boundary(plate) == n + plate.shape[0] == eng.n
    q = scenes.volume_points((-1.6, -1.7, -1.5), (0.4, 0.3, 0.5), (9, 9, 7))
    got, want = _device_ops(eng, q), _oracle_ops(ora, q)
    for k in ("div_velocities", "curl_velocities", "lap_densities"):
        assert got[k].shape[0] == n  # N() rows, not Total()
        rows = want[k].reshape(n, -1)
        finite = np.isfinite(rows).all(axis=1)
        live = np.mean(finite & np.any(rows != 0, axis=1))
        print(f"{k}: oracle finite and non-zero at {100 * live:.1f} %, non-finite at {100 * np.mean(~finite):.1f} %")
        assert live >= 0.15 and np.mean(~finite) >= 0.15, (k, live)
    assert np.isnan(want["int_densities"]).any() and np.any(np.isfinite(want["int_densities"]) & (want["int_densities"] != 0))
    _check("boundary", math_mode, got, want)
    # count = Total() is refused
    L, total = eng._L, eng.n
    out = np.full(3 * total, -7.0, dtype=np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    assert L.dsl_field_divergence(eng._h, 1, fp, total) == -1
    assert L.dsl_field_curl(eng._h, 1, fp, 3 * total) == -1
    assert L.dsl_field_laplacian(eng._h, 3, fp, total) == -1
    assert np.all(out == -7.0)
    eng.close()


# ---- d. the reference's LSH neighbours ---------------------------------------------------------------------------------

def test_lsh_neighbours():
    """DSL_NEIGH_LSH_REF: candidates are the 100 samples of the query's bucket, with duplicates and far particles, and no
    distance test but the kernels' own cut-offs.  Density field: bit for bit; pressure field: 1e-6 (a float64 pow,
    device libm against glibc, as test_gpu_lsh.py); non-finite values in the oracle's places."""
    from dieselfluid_amd import SPHEngine
    from dieselfluid_amd.engine import reference_params
    n3 = 12
    hv = po.default_hash_vectors(5)
    pos = helpers.jittered_lattice(n3, 0.25)
    vel = helpers.seeded_velocities(n3 ** 3, 0.1)
    frc = helpers.seeded_velocities(n3 ** 3, 5.0, seed=41)
    p = reference_params(n3)
    p.neigh_mode = 0  # DSL_NEIGH_LSH_REF
    p.math_mode = EXACT
    eng = SPHEngine(p)
    eng.set_hash_vectors(hv)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.upload("forces", frc)
    ora = po.OracleSPH.from_state(po.params_reference(n3), pos, vel=vel, force=frc, hash_vectors=hv)
    eng.density_all(); ora.density_all()
    assert np.array_equal(_bits(eng.download("densities")), _bits(ora.densities()))
    q = _queries(pos, -1.0, 1.0, 0.5)
    got, want = _device_ops(eng, q), _oracle_ops(ora, q)
    for k in KEYS:
        g, w = got[k], want[k]
        if not k.endswith("pressures"):
            assert _same_bits(g, w), k
            continue
        ok = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(_bits(g)[~ok & ~np.isnan(w)], _bits(w)[~ok & ~np.isnan(w)]), k
        assert ok.any() and np.abs(g[ok].astype(np.float64) - w[ok]).max() < 1e-6 * np.abs(w[ok]).max(), k
    for k in ("div_velocities", "curl_velocities", "lap_densities", "int_densities"):
        assert np.mean(np.isfinite(want[k]) & (want[k] != 0)) > 0.5, k
    eng.close()


# ---- e. edges ----------------------------------------------------------------------------------------------------------

def _edge_compare(tag, p, pos, vel, q, keys=KEYS, mode=po.NEIGH_GRID, judge=False, zero_density=False):
    """upload, density_all, the operators against the oracle (grid neighbours, cell order: EXACT bit for bit); `judge`:
    also against the oracle's all-pairs rule, at the FAST tolerances in both math modes"""
    frc = helpers.seeded_velocities(pos.shape[0], 5.0 * float(p.mass), seed=41)
    eng = _engine(p, pos, vel, frc)
    eng.density_all()
    ora = po.OracleSPH.from_state(helpers.oracle_params(p, mode=mode), pos, vel=vel, force=frc)
    ora.density_all()
    got, want = _device_ops(eng, q, keys), _oracle_ops(ora, q, keys)
    sens = _sensitivity(p, ora, q, keys, stride=1 if pos.shape[0] <= 1024 else 5)
    _check(tag, p.math_mode, got, want, sens, zero_density)
    if judge:
        brute = po.OracleSPH.from_state(helpers.oracle_params(p, mode=po.NEIGH_ALL), pos, vel=vel, force=frc)
        brute.density_all()
        _check(tag + " (all pairs)", FAST, got, _oracle_ops(brute, q, keys), sens)
    return eng, got, want


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("n", [1, 2, 65])
def test_tiny_and_ragged_counts(n, math_mode):
    """test_tiny_and_ragged_particle_counts' clumps: no neighbour at all (rho = 0: Interpolate on the particle divides
    by it), one pair (Laplacian(density) is exactly 0 in the oracle), a count that is no multiple of a wave.

    n = 1 in FAST: the density sweep meets the particle itself and subtracts that term afterwards, in the expanded
    form of r^2, so the lone particle's density is a rounding residue of the self term m W0 and not 0 (measured:
    -3.97e-4 = -2.0e-6 m W0; EXACT: 0).  m / rho is then some finite number where the oracle has m / 0, and
    Interpolate within h of the particle returns m F(r) where the oracle and EXACT return NaN.  A density error of
    2e-6 of the sum with the self term is FAST's own bar, so those two query points are not compared in FAST; every
    other value (0 everywhere, and finite) is."""
    from dieselfluid_amd import scenes
    p, _ = scenes.dambreak_scene(12, math_mode=math_mode, positions=False)
    p.n_particles = n
    rng = np.random.default_rng(n)
    pos = (0.3 + 0.2 * rng.random((n, 3))).astype(np.float32)
    vel = helpers.seeded_velocities(n, 0.1, seed=n)
    q = np.concatenate([pos, pos + np.float32(0.03), np.full((2, 3), 3.0, np.float32)]).astype(np.float32)
    eng, got, want = _edge_compare(f"n={n}", p, pos, vel, q, zero_density=(n == 1))
    if n == 1:
        assert np.isnan(want["int_densities"][:2]).all() and np.all(want["int_densities"][2:] == 0)
        assert math_mode == FAST or np.isnan(got["int_densities"][:2]).all()
    assert got["div_velocities"].shape == (n,) and got["curl_velocities"].shape == (n, 3)
    eng.close()


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_coincident_pairs(math_mode):
    """two pairs at r = 0 among 64 particles: Norm() of the zero vector is zero (the dist != 0 branch), the pair counts
    in Laplacian and Interpolate; everything stays finite"""
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(4, math_mode=math_mode)
    pos = pos.copy()
    pos[1] = pos[0]
    pos[37] = pos[20]
    vel = helpers.seeded_velocities(64, 0.2)
    q = _queries(pos, 0.0, 1.0, float(p.h), n_between=64, n_on=64)
    eng, got, want = _edge_compare("coincident", p, pos, vel, q)
    assert all(np.isfinite(got[k]).all() and np.isfinite(want[k]).all() for k in KEYS)
    eng.close()


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_particles_and_queries_outside_the_grid_box(math_mode):
    """test_particles_outside_the_grid_box's clumps (cell_coord clamps, and clamping is monotone: the 27-cell sweep stays
    complete).  The grid oracle clamps by the same rule (EXACT: its bits); the all-pairs oracle is the judge of
    completeness.  Query points inside the displaced clumps, outside the box, and at 1e6: zeros there.

    FAST missed this check at first (EXACT passed, bit for bit), and the operator kernels were not the reason.  Measured
    on an MI355X, max |device - oracle| against the tolerance: Div(velocities) 6.99e-5 / 4.62e-5, Curl(velocities)
    6.96e-5 / 5.02e-5, Laplacian(density) 31.2 / 15.9, all three at the clump beyond the far x end.  Cause: the FAST
    density pass stages positions relative to the centre of the particle's grid tile and forms r^2 in the expanded
    form (kernels_tiled.hpp, "D (tiled)"), whose cancellation error grows with the square of the tile-relative
    coordinate; a particle clamped into an edge cell from 23 cells outside the box is that far from its tile's centre.
    FAST densities against the oracle, relative: 2.4e-6 inside the box, 1.5e-5 in the clump 0.9 below it, 1.8e-4 in the
    clump 9.0 beyond it -- ninety times the 2e-6 the tolerances are built on.  The tiled density kernels now take the
    density of a target further than 3 cells from its tile's centre from the global-memory sweep (tile_target_far);
    with that: Div(velocities) 6.56e-7, Curl(velocities) 1.01e-6, Laplacian(density) 1.02, against the same
    tolerances."""
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(8, math_mode=math_mode)
    p.walls = 0
    pos = pos.copy()
    pos[:64] -= np.float32(0.9)
    pos[64:128, 0] += np.float32(9.0)
    vel = helpers.seeded_velocities(pos.shape[0], 0.1)
    far = np.array([[1e6, 0.5, 0.5], [-1e6, -1e6, -1e6], [0.5, 1e6, 0.5], [30.0, 0.5, 0.5], [0.5, 0.5, -7.0]], np.float32)
    q = np.concatenate([pos[:128] + np.float32(0.02), pos[200:264], far]).astype(np.float32)
    eng, got, want = _edge_compare("outside", p, pos, vel, q, judge=True)
    for k in ("int_densities", "int_pressures"):
        assert np.all(got[k][-5:] == 0) and np.all(want[k][-5:] == 0)
    assert np.mean(want["int_densities"][:128] != 0) > 0.5  # (the thin clumps lie below eos_d0_grad: their pressure is 0)
    assert np.any(want["int_pressures"] != 0)
    eng.close()


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_about_125_particles_per_cell(math_mode):
    """h = 5 dx: more candidates per cell than a key row holds; Interpolate and Laplacian(density)"""
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(16, math_mode=math_mode, h_over_dx=5.0)
    q = _queries(pos, 0.0, 1.0, float(p.h))
    eng, got, want = _edge_compare("h=5dx", p, pos, None, q, keys=("lap_densities", "int_densities"))
    eng.nn()
    assert np.diff(eng.download_cell_start()).max() > 100
    eng.close()


@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_query_sets_of_0_1_and_capacity_points(math_mode):
    """query positions travel through the staging buffer of 3 x capacity floats: exactly `capacity` points fit; no
    point: an empty array, and nothing is launched"""
    from dieselfluid_amd import scenes
    from dieselfluid_amd.engine import KERNEL_IDS
    p, pos = scenes.dambreak_scene(8, math_mode=math_mode)
    n = pos.shape[0]
    eng = _engine(p, pos, helpers.seeded_velocities(n, 0.1))
    eng.density_all()
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos)
    ora.density_all()
    assert eng.capacity == n
    rng = np.random.default_rng(2)
    q = (rng.random((n, 3)) * 1.2 - 0.1).astype(np.float32)  # `capacity` points, in and around the block
    for scalar in ("densities", "pressures"):
        k = "int_" + scalar
        full = eng.field_interpolate(q, scalar)
        one = eng.field_interpolate(q[17:18], scalar)
        want = {k: ora.field_interpolate(q, OSCALAR[scalar])}
        assert np.mean(want[k] != 0) > 0.5
        _check("capacity points", math_mode, {k: full}, want)
        assert one.shape == (1,) and _bits(one)[0] == _bits(full)[17]
    eng.timing_enable(True)
    eng.timing_reset()
    before = eng.download("densities")
    counts = [eng.timing(name)[1] for name in KERNEL_IDS]
    empty = eng.field_interpolate(np.zeros((0, 3), np.float32), "densities")
    assert empty.shape == (0,)
    assert [eng.timing(name)[1] for name in KERNEL_IDS] == counts
    assert np.array_equal(_bits(eng.download("densities")), _bits(before))
    eng.close()


# ---- f. refusals -------------------------------------------------------------------------------------------------------

SENTINEL = np.float32(-12345.0)
POS, VEL, FRC, RHO, PRS = 0, 1, 2, 3, 4


def test_refusals_change_nothing():
    """Every refused call returns DSL_ERR_INVALID (-1), leaves the output array alone and allocates nothing; the next
    valid call returns the bits from before.  After dsl_slab_config: DSL_ERR_UNSUPPORTED (-4), "slab" in the text."""
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(8, math_mode=FAST)
    n = pos.shape[0]
    eng = _engine(p, pos, helpers.seeded_velocities(n, 0.1), _force_field(p, n))
    eng.density_all()
    q = _queries(pos, 0.0, 1.0, float(p.h))
    before = _device_ops(eng, q)
    nbytes = eng.get_option("device_bytes")
    L, h = eng._L, eng._h
    out = np.full(3 * n + 8, SENTINEL, dtype=np.float32)
    fp = out.ctypes.data_as(C.POINTER(C.c_float))
    qbig = np.zeros((eng.capacity + 1, 3), dtype=np.float32)
    qp, qbp = q.ctypes.data_as(C.POINTER(C.c_float)), qbig.ctypes.data_as(C.POINTER(C.c_float))
    refused = [
        # NULL output
        lambda: L.dsl_field_divergence(h, VEL, None, n), lambda: L.dsl_field_curl(h, VEL, None, 3 * n),
        lambda: L.dsl_field_laplacian(h, RHO, None, n), lambda: L.dsl_field_interpolate(h, RHO, qp, q.shape[0], None),
        lambda: L.dsl_field_interpolate(h, RHO, None, q.shape[0], fp),
        # wrong count: one short, and x 3 mixed up between Div and Curl
        lambda: L.dsl_field_divergence(h, VEL, fp, n - 1), lambda: L.dsl_field_curl(h, VEL, fp, 3 * n - 1),
        lambda: L.dsl_field_laplacian(h, RHO, fp, n - 1), lambda: L.dsl_field_divergence(h, FRC, fp, 3 * n),
        lambda: L.dsl_field_curl(h, FRC, fp, n),
        # a scalar buffer for a tensor operator and the reverse; a buffer that is neither
        lambda: L.dsl_field_divergence(h, RHO, fp, n), lambda: L.dsl_field_curl(h, PRS, fp, 3 * n),
        lambda: L.dsl_field_laplacian(h, VEL, fp, n), lambda: L.dsl_field_interpolate(h, FRC, qp, q.shape[0], fp),
        lambda: L.dsl_field_divergence(h, POS, fp, n), lambda: L.dsl_field_laplacian(h, 5, fp, n),
        # more query points than the staging buffer holds
        lambda: L.dsl_field_interpolate(h, RHO, qbp, eng.capacity + 1, fp),
    ]
    for k, call in enumerate(refused):
        assert call() == -1, k
        assert L.dsl_last_error(h), k
        assert np.all(out == SENTINEL), k
    assert eng.get_option("device_bytes") == nbytes
    after = _device_ops(eng, q)
    for k in KEYS:
        assert np.array_equal(_bits(after[k]), _bits(before[k])), k
    eng.close()
    # slab mode
    slab = _engine(p, pos)
    slab.slab_config(0, 0.0, 4.0)
    L, h = slab._L, slab._h
    for k, call in enumerate([lambda: L.dsl_field_divergence(h, VEL, fp, n), lambda: L.dsl_field_curl(h, VEL, fp, 3 * n),
                              lambda: L.dsl_field_laplacian(h, RHO, fp, n),
                              lambda: L.dsl_field_interpolate(h, RHO, qp, q.shape[0], fp)]):
        assert call() == -4, k
        assert b"slab" in L.dsl_last_error(h), k
        assert np.all(out == SENTINEL), k
    slab.close()
