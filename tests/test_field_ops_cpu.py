"""CPU: the oracle's field operators (dslo_field_div / curl / laplacian / interpolate, the judge of every device test of
dsl_field_*) against helpers.field_ops_f64 -- float64, brute force over all particles, written from sph_field.go:124-135,
203-294, std_kernel.go and field_types.go:39-42 independently of oracle and engine.  Device and oracle were written from
one reading of sph_field.go; a shared misreading (a sign, a kernel, the wrong density in the quotient, the self term)
is wrong by order 1 and fails here.

Two states: the seeded 16^3 dam-break after 10 oracle WCSPH steps and a density_all, and the jittered 12^3 reference
lattice with seeded velocities.  Every fifth particle, and about 500 query points: between particles, exactly on a
particle, and more than h outside the fluid (where every sum is empty: 0 on both sides).

Measure: max |oracle - float64| / max |float64| over the probes.  Bound: ten times the measured figure, rounded up to
one digit (float32 sums of ~30 to ~60 terms against float64: 1e-7 to 1e-6; the pressure field amplifies a rounding of
rho by gamma = 7.16, and its Laplacian subtracts nearly equal pressures).  Measured (gcc, -ffp-contract=off):

  state      Div      Curl     Lap(density)  Lap(pressure)  Int(density)  Int(pressure)
  dambreak   1.59e-7  8.71e-7  2.49e-7       4.53e-6        2.41e-7       3.00e-6
  lattice    5.29e-7  5.28e-7  1.38e-6       8.37e-7        1.27e-6       7.46e-7

Every compared array is non-zero at more than half of its probes by the float64 reference (asserted)."""
import numpy as np
import pytest

import helpers
from oracle import pyoracle as po

KEYS = ("div", "curl", "lap_density", "lap_pressure", "interp_density", "interp_pressure")
BOUND = {
    "dambreak": dict(zip(KEYS, (2e-6, 9e-6, 3e-6, 5e-5, 3e-6, 3e-5))),
    "lattice": dict(zip(KEYS, (6e-6, 6e-6, 2e-5, 9e-6, 2e-5, 8e-6))),
}
_STATE = {}


def _queries(pos, lo, hi, h, seed):
    """~500 points: ~300 between particles, ~100 exactly on a particle, 100 more than h outside [lo, hi]^3"""
    rng = np.random.default_rng(seed)
    n = pos.shape[0]
    a = pos[:: max(n // 300, 1)]
    between = a + ((rng.random(a.shape) - 0.5) * 0.5 * h).astype(np.float32)
    on = pos[3:: max(n // 100, 1)]
    out = (hi + 1.5 * h + rng.random((100, 3)) * 3 * h).astype(np.float32)
    out[::2, 1] = (lo - 1.5 * h - rng.random(50) * h).astype(np.float32)  # half of them below, half beyond the far corner
    return np.concatenate([between, on, out]).astype(np.float32)


def _state(name):
    """(oracle values, float64 values) of the six compared arrays, computed once per state"""
    if name in _STATE:
        return _STATE[name]
    from dieselfluid_amd import scenes
    if name == "dambreak":
        p, pos = scenes.dambreak_scene(16, math_mode=0, jitter=0.05)
        frc = np.tile(np.array(p.force_reset[:], dtype=np.float32), (pos.shape[0], 1))
        ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, force=frc)
        ora.wcsph_step(10)
        ora.sampler_update()  # (the step sorted the particles where they were before it moved them)
        lo, hi = 0.0, 1.0
    else:
        p, _ = scenes.reference_scene(12)
        pos = helpers.jittered_lattice(12, 0.2)
        ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, vel=helpers.seeded_velocities(12 ** 3, 0.1))
        lo, hi = -1.0, 1.0
    ora.density_all()
    x, v, rho = ora.positions(), ora.velocities(), ora.densities()
    probe = np.arange(0, x.shape[0], 5)
    q = _queries(x, lo, hi, float(p.h), 17)
    got = {"div": ora.field_div("velocity")[probe], "curl": ora.field_curl("velocity")[probe],
           "lap_density": ora.field_laplacian("density")[probe], "lap_pressure": ora.field_laplacian("pressure")[probe],
           "interp_density": ora.field_interpolate(q, "density"), "interp_pressure": ora.field_interpolate(q, "pressure")}
    want = helpers.field_ops_f64(p, x, v, rho, probe, q)
    ora.close()
    _STATE[name] = (got, want)
    return _STATE[name]


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("state", ["dambreak", "lattice"])
def test_oracle_field_operator_against_float64(state, key):
    got, want = _state(state)
    g, w = np.asarray(got[key], dtype=np.float64), want[key]
    assert g.shape == w.shape and np.isfinite(g).all() and np.isfinite(w).all()
    rows = w.reshape(w.shape[0], -1)
    nonzero = float(np.mean(np.any(rows != 0, axis=1)))
    err = helpers.rel_err(g, w)
    print(f"{state} {key}: max |oracle - float64| / max |float64| = {err:.2e} (bound {BOUND[state][key]:.0e}), "
          f"non-zero at {100 * nonzero:.1f} % of {rows.shape[0]} probes, max |float64| = {np.abs(w).max():.4g}")
    assert nonzero > 0.5
    assert err < BOUND[state][key]
