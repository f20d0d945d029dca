"""No GPU: tests/contact_ref.py, the numpy restatement of the contact rule of csrc/contact.hip, on its own -- the point rule
against a brute-force count, the wall sums against float64, a glancing hit's momentum and energy, a dropped sphere's rest, a
kinematic body, the order of the bodies -- and the new names across header, ctypes table, engine, Go and C++."""
import math
import os
import re

import numpy as np

import bodies_ref as br
import contact_cases as cc
import contact_ref as cr

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _brute_points(vol):
    """the rule voxel by voxel, in plain Python"""
    nz, ny, nx = vol.shape
    out = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                v = vol[k, j, i]
                if not (np.isfinite(v) and v <= 0):
                    continue
                nb = [(k, j, i - 1), (k, j, i + 1), (k, j - 1, i), (k, j + 1, i), (k - 1, j, i), (k + 1, j, i)]
                if any(0 <= c < nz and 0 <= b < ny and 0 <= a < nx and np.isfinite(vol[c, b, a]) and vol[c, b, a] > 0 for c, b, a in nb):
                    out.append((k * ny + j) * nx + i)
    return np.array(out, dtype=np.int32)


def test_the_point_rule_picks_the_innermost_shell():
    for vol, count in ((cc.sphere(), 656), (cc.sphere(16, 5.2), 264), (cc.sphere_nan(), 655), (cc.sphere_unsigned(), 0)):
        got = cr.points(vol)
        assert got.dtype == np.int32 and len(got) == count and np.array_equal(got, _brute_points(vol))
        assert (np.diff(got) > 0).all()
    # the NaN voxel itself leaves the list and nothing else changes: NaN is neither <= 0 nor > 0
    nan_at = (12 * 24 + 12) * 24 + 4
    assert np.array_equal(np.setdiff1d(cr.points(cc.sphere()), cr.points(cc.sphere_nan())), [nan_at])
    # the sizes the device tests rely on
    assert len(cr.points(cc.cube())) == 1016 and len(cr.points(cc.cube(116, 53.3))) == 66152
    # a lattice two voxels thin: every voxel's neighbour is inside the lattice on one side only
    thin = cc.sphere()[11:13]
    assert np.array_equal(cr.points(thin), _brute_points(thin)) and len(cr.points(thin)) > 0
    # the coordinates are origin + step * index
    o, s = cc.lattice(24)
    pl = cr.point_coords(o, s, (24, 24, 24), np.array([nan_at]))
    assert _same(pl[0], np.array([f32(o[0]) + f32(s[0]) * f32(4), f32(o[1]) + f32(s[1]) * f32(12), f32(o[2]) + f32(s[2]) * f32(12)], dtype=f32))


def test_the_wall_sums_of_a_sphere_under_the_floor_against_float64():
    bodies = cc.sunk_sphere()
    con = cr.contributions(bodies, cr.WALLS, 1, cc.BOX_MIN, cc.BOX_MAX)
    E = cr.table_of(con, 1)
    assert not E[0, [0, 1, 3, 4, 5, 6]].any() and E[0, 2, 7] == 121  # the floor alone, 121 points under it
    c = con[(0, 2)][:, :8].astype(np.float64)
    exact = np.array([math.fsum(c[:, k]) for k in range(8)])
    err, bound = np.abs(E[0, 2, :8] - exact), len(c) * 2.0 ** -24 * np.abs(c).sum(axis=0)
    print(f"|total - fsum| = {err}, bound n 2^-24 sum|c| = {bound}")
    assert (err <= bound).all() and (np.abs(exact[[0, 1, 2, 4, 6]]) > 10 * bound[[0, 1, 2, 4, 6]]).all()
    assert E[0, 2, 8] == con[(0, 2)][:, 8].max() > 0.06
    # walls off, or the kind off: nine +0 everywhere
    assert not _bits(cr.detect(bodies, cr.WALLS, 0, cc.BOX_MIN, cc.BOX_MAX)).any()
    assert not _bits(cr.detect(bodies, cr.BODIES, 1, cc.BOX_MIN, cc.BOX_MAX)).any()


def _momentum_energy(bodies):
    """float64, from the float32 states: sum v / inv_mass, sum (v.v / inv_mass + sum wl_a^2 / inv_inertia_a) / 2"""
    p, e = np.zeros(3), 0.0
    for bd in bodies:
        im, ii = float(bd["props"]["inv_mass"]), bd["props"]["inv_inertia"].astype(np.float64)
        v, w = bd["state"]["lin_vel"].astype(np.float64), bd["state"]["ang_vel"].astype(np.float64)
        wl = bd["state"]["rot"].astype(np.float64).T @ w
        p += v / im
        e += 0.5 * (v @ v) / im + 0.5 * (wl * wl / ii).sum()
    return p, e


# Measured here, the float32 reference with its sums taken in float64:
#   the glancing pair over 400 steps at dt = 0.002 (two entries solved): the total momentum (-1, 0, 0) does not move by one
#   bit -- both masses are powers of two and each impulse is added to one body and subtracted from the other -- and the
#   kinetic energy 1.5 drifts by 2.03e-7;
#   the sphere dropped from 0.5 for 1500 steps ends 8.06e-5 above the height at which its innermost shell stands on the
#   floor (7.5 steps = 0.15), still bouncing by one step's worth of gravity (there is no resting contact in the rule).
# Each asserted at four times the measured value.
PAIR_MOMENTUM_TOL = 4 * 0.0
PAIR_ENERGY_TOL = 4 * 2.03e-7
REST_HEIGHT_TOL = 4 * 8.06e-5


def test_a_glancing_hit_at_restitution_one_keeps_momentum_and_energy():
    bodies = cc.glancing_pair()
    p0, e0 = _momentum_energy(bodies)
    solved = 0
    for _ in range(400):
        solved += cr.step_dry(bodies, cc.DT, cr.BODIES, 1, cc.BOX_MIN, cc.BOX_MAX)[1]
    p1, e1 = _momentum_energy(bodies)
    dp, de = float(np.abs(p1 - p0).max()), abs(e1 - e0)
    print(f"entries solved {solved}, |dp| = {dp:.3e} of {np.abs(p0).max():.3g}, |dE| = {de:.3e} of {e0:.3g}")
    assert solved >= 2 and dp <= PAIR_MOMENTUM_TOL and de <= PAIR_ENERGY_TOL
    # it was a hit, and a glancing one: both bodies turned away and picked up the other axis
    assert bodies[0]["state"]["lin_vel"][0] < 0 < bodies[1]["state"]["lin_vel"][0]
    assert abs(bodies[0]["state"]["lin_vel"][2]) > 0.05


def test_a_dropped_sphere_stays_in_the_box_and_comes_to_rest_on_its_innermost_shell():
    bodies = cc.dropped_sphere()
    lowest = np.inf
    for _ in range(1500):
        cr.step_dry(bodies, cc.DT, cr.WALLS, 1, cc.BOX_MIN, cc.BOX_MAX)
        lowest = min(lowest, float(bodies[0]["state"]["trans"][1]) - cc.REST_HEIGHT)
    s = bodies[0]["state"]
    err = abs(float(s["trans"][1]) - cc.REST_HEIGHT)
    print(f"lowest point of the shell over the run {lowest:.3e}, |trans.y - 0.15| at the end = {err:.3e}, lin_vel.y = {s['lin_vel'][1]:.3e}")
    assert lowest > cc.BOX_MIN[1] - cc.STEP and err <= REST_HEIGHT_TOL
    assert abs(float(s["lin_vel"][1])) <= 9.81 * cc.DT  # one step of gravity is all the motion that is left
    assert s["trans"][0] == 1 and s["trans"][2] == 1  # (a wall's normal is its axis: nothing pushes sideways without friction)
    # without the stage it has left the box long before
    free = cc.dropped_sphere()
    for _ in range(300):
        cr.step_dry(free, cc.DT, 0, 1, cc.BOX_MIN, cc.BOX_MAX)
    assert free[0]["state"]["trans"][1] < cc.BOX_MIN[1]


def test_a_kinematic_body_keeps_every_bit_of_its_record_and_others_bounce_off_it():
    bodies = cc.overlapping_pair()
    bodies[1]["props"] = br.props(radius=0.01, restitution=0.8)
    before = cr.state_words(bodies)
    E, solved = cr.contact(bodies, cr.WALLS | cr.BODIES, 1, cc.BOX_MIN, cc.BOX_MAX)
    after = cr.state_words(bodies)
    assert solved == 2 and _same(after[1], before[1])
    assert not _same(after[0, 4:7], before[0, 4:7]) and not _same(after[0, 7:10], before[0, 7:10])
    # two kinematic bodies: k = 0, nothing is solved
    bodies[0]["props"] = br.props(radius=0.01, restitution=0.5)
    assert cr.solve(bodies, E) == 0


def test_swapping_two_bodies_changes_the_result_only_where_both_take_part():
    def scene(order):
        pair, loner = cc.overlapping_pair(), cc.sunk_sphere()[0]
        return [pair[order[0]], pair[order[1]], loner]
    fwd, rev = scene((0, 1)), scene((1, 0))
    Ef, nf = cr.contact(fwd, 3, 1, cc.BOX_MIN, cc.BOX_MAX)
    Er, nr = cr.contact(rev, 3, 1, cc.BOX_MIN, cc.BOX_MAX)
    assert nf == nr == 3
    # the detection does not know the order: the entries move with the bodies
    assert _same(Ef[0, 7], Er[1, 6]) and _same(Ef[1, 6], Er[0, 7]) and _same(Ef[2], Er[2]) and Ef[2, 2, 7] == 121
    sf, sr = cr.state_words(fwd), cr.state_words(rev)
    assert _same(sf[2], sr[2])  # the loner meets the floor alone
    assert not _same(sf[0], sr[1]) and not _same(sf[1], sr[0])  # the pair is solved at its first entry, which is another one


def test_the_bindings_agree_on_the_new_names():
    from dieselfluid_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "dslsph.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {"dsl_contact_points": 5, "dsl_contact_pass": 3, "dsl_contact_table": 3}
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(dsl_contact_\w+)\s*\(([^)]*)\)", code)}
    assert {k: len(v.split(",")) for k, v in decl.items()} == want
    assert {k: len(_lib.EXPORTS[k][1]) for k in want} == want
    assert re.search(r"\bDSL_OPT_BODIES_CONTACT\s*=\s*80\b", code) and re.search(r"\bDSL_OPT_BODIES_CONTACTS\s*=\s*81\b", code)
    assert re.search(r"\bDSL_K_COUNT\s*=\s*19\b", code)  # the new launches are timed under DSL_K_COLLIDE
    assert engine.SPHEngine.OPTIONS["bodies_contact"] == 80 and engine.SPHEngine.OPTIONS["bodies_contacts"] == 81
    for name in ("contact_points", "contact_pass", "contact_table"):
        assert callable(getattr(engine.SPHEngine, name))
    assert "contact.hip" in _lib.UNITS
    go = open(os.path.join(ROOT, "bindings", "go", "dslsph", "dslsph.go")).read()
    for name in ["C." + k + "(" for k in want] + ["C.DSL_OPT_BODIES_CONTACT)", "C.DSL_OPT_BODIES_CONTACTS)", "func (e *Engine) ContactPoints(",
                                                 "func (e *Engine) ContactPass(", "func (e *Engine) ContactTable("]:
        assert name in go, name
    hpp = open(os.path.join(ROOT, "dieselfluid_amd", "host", "dieselfluid.hpp")).read()
    for name in [k + "(" for k in want] + ["DSL_OPT_BODIES_CONTACT,", "DSL_OPT_BODIES_CONTACTS,", "ContactPoints(", "ContactPass(", "ContactTable("]:
        assert name in hpp, name
