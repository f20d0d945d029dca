"""GPU: the rigid bodies' contact stage (include/dslsph.h: dsl_contact_points and its calls, DSL_OPT_BODIES_CONTACT;
csrc/contact.hip) against tests/contact_ref.py, the numpy float32 restatement of the build-defined rule: the contact points,
the detection's table, the solve, and the step drivers that run them behind the integration.  One arithmetic in both math
modes and a fixed order of additions: every check of a device result is an equality, bit for bit.  The inputs are pinned in
tests/contact_cases.py; tests/test_contact_cpu.py asserts on the reference what they cover."""
import ctypes as C
import functools

import numpy as np
import pytest

import bodies_ref as br
import contact_cases as cc
import contact_ref as cr
import helpers
import test_gpu_bodies as tb  # its dam-break handle in lockstep with the oracle, its two dynamic balls
import test_gpu_sdf_collider as static_case
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = 0, 1
KEYS = ("quat", "trans", "lin_vel", "ang_vel")
# a handful of particles far from every body of contact_cases
FAR = np.array([[3.2 + 0.3 * (k & 1), 3.2 + 0.3 * ((k >> 1) & 1), 3.2 + 0.3 * ((k >> 2) & 1)] for k in range(8)], dtype=f32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _engine(math_mode=EXACT, walls=1):
    from dieselfluid_amd import SPHEngine, scenes
    p, _ = scenes.reference_scene(10)  # h = 1, m = 1, grid box [-4, 4]^3
    p.n_particles = len(FAR)
    p.math_mode = math_mode
    p.dt = cc.DT
    p.walls = walls
    for a in range(3):
        p.box_min[a], p.box_max[a] = cc.BOX_MIN[a], cc.BOX_MAX[a]
    eng = SPHEngine(p, device=0)
    eng.upload("positions", FAR)
    return eng


def _add(eng, bd):
    return eng.add_body(bd["vol"], bd["origin"], bd["step"], br.api_props(bd["props"]), br.api_state(bd["state"]))


def _loaded(bodies, math_mode=EXACT, walls=1):
    eng = _engine(math_mode, walls)
    for b, bd in enumerate(bodies):
        assert _add(eng, bd) == b
    return eng


def _states(eng, K):
    return np.stack([np.concatenate([eng.body_state(b)[0][k] for k in KEYS]) for b in range(K)])


def _table_then_solve(bodies, kinds=3, math_mode=EXACT, walls=1):
    """the table alone, then table and solve, against the reference for every word: (E, entries solved)"""
    eng = _loaded(bodies, math_mode, walls)
    want = cr.detect(bodies, kinds, walls, cc.BOX_MIN, cc.BOX_MAX)
    eng.contact_pass(kinds, solve=False)
    assert _same(eng.contact_table(), want)
    assert _same(_states(eng, len(bodies)), cr.state_words(bodies))  # detection alone moves nothing
    assert eng.get_option("bodies_contact") == 0  # (the call runs whatever the option is)
    solved = cr.clone(bodies)
    n = cr.solve(solved, want)
    eng.contact_pass(kinds, solve=True)
    assert _same(eng.contact_table(), want)
    assert _same(_states(eng, len(bodies)), cr.state_words(solved))
    assert eng.get_option("bodies_contacts") == n
    assert _same(eng.download("positions"), FAR)  # no particle is touched
    eng.close()
    return want, n


# ---- the point lists ----
@pytest.mark.parametrize("case", ["sphere", "device", "nan", "unsigned", "thin"])
def test_the_contact_points_are_the_references(case):
    import torch
    vol = {"sphere": cc.sphere(), "device": cc.sphere(), "nan": cc.sphere_nan(), "unsigned": cc.sphere_unsigned(),
           "thin": np.ascontiguousarray(cc.sphere()[:, 11:13, :])}[case]  # (dims = (24, 2, 24))
    want = cr.points(vol)
    assert len(want) == {"sphere": 656, "device": 656, "nan": 655, "unsigned": 0, "thin": len(want)}[case] and (case != "thin" or len(want) > 50)
    eng = _engine()
    o, s = cc.lattice(24)
    if case == "device":
        buf = torch.from_numpy(vol.copy()).to("cuda:0")
        eng.add_body(None, o, s, br.api_props(br.props(**cc.BALL)), dims=vol.shape[::-1], dev_volume=buf.data_ptr())
    else:
        eng.add_body(vol, o, s, br.api_props(br.props(**cc.BALL)))
    before = eng.get_option("device_bytes")
    m = C.c_int64(-1)
    assert eng._L.dsl_contact_points(eng._h, 0, None, 0, C.byref(m)) == 0 and m.value == len(want)  # the counting call
    assert eng.get_option("device_bytes") > before or case == "unsigned"  # (the lists were built by the call, and are counted)
    got, total = eng.contact_points(0)
    assert total == len(want) and got.dtype == np.int32 and np.array_equal(got, want)
    if len(want) > 300:  # cap < M: the first cap of them and nothing beyond
        buf = np.full(301, -7, dtype=np.int32)
        assert eng._L.dsl_contact_points(eng._h, 0, buf.ctypes.data_as(C.POINTER(C.c_int32)), 300, C.byref(m)) == 0
        assert m.value == len(want) and np.array_equal(buf[:300], want[:300]) and buf[300] == -7
    assert eng.get_option("bodies_contact") == 0
    eng.close()


# ---- walls ----
@pytest.mark.parametrize("math_mode", [EXACT, FAST])
@pytest.mark.parametrize("scene", ["sunk_sphere", "corner_cube"])
def test_the_wall_table_and_solve_are_the_references(scene, math_mode):
    bodies = getattr(cc, scene)()
    E, n = _table_then_solve(bodies, kinds=cr.WALLS, math_mode=math_mode)
    if scene == "sunk_sphere":  # 656 points in three workgroups, the floor alone
        assert n == 1 and E[0, 2, 7] == 121 and not E[0, [0, 1, 3, 4, 5, 6]].any()
    else:  # 1016 points, three walls at once
        assert n == 3 and (E[0, [0, 2, 4], 7] > 50).all() and not E[0, [1, 3, 5, 6]].any()


def test_without_walls_or_without_the_kind_the_table_is_all_zero():
    bodies = cc.corner_cube()
    for walls, kinds in ((0, 3), (1, cr.BODIES), (1, 0)):
        eng = _loaded(bodies, walls=walls)
        eng.contact_pass(kinds, solve=True)
        assert not _bits(eng.contact_table()).any() and eng.get_option("bodies_contacts") == 0
        assert _same(_states(eng, 1), cr.state_words(bodies))
        eng.close()


def test_a_body_of_more_than_65536_points_takes_the_folds_second_trip():
    bodies = cc.big_cube()
    eng = _loaded(bodies)
    got, m = eng.contact_points(0, cap=16)
    want_pts = cr.points(bodies[0]["vol"])
    assert m == len(want_pts) == 66152 and np.array_equal(got, want_pts[:16])  # 259 workgroups
    want = cr.detect(bodies, cr.WALLS, 1, cc.BOX_MIN, cc.BOX_MAX)
    assert 25000 < want[0, 2, 7] < 40000  # half under the floor
    eng.contact_pass(cr.WALLS, solve=False)
    assert _same(eng.contact_table(), want)
    eng.close()


# ---- pairs ----
def test_two_overlapping_spheres_both_ordered_entries():
    E, n = _table_then_solve(cc.overlapping_pair())
    assert n == 2 and E[0, 7, 7] >= 30 and E[1, 6, 7] >= 30


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
def test_three_bodies_in_both_orders(order):
    scene = cc.three_bodies()
    E, n = _table_then_solve([scene[b] for b in order])
    assert n == 4 and (E[:, 6:, 7] > 0).sum() == 4


def test_a_dynamic_body_bounces_off_a_kinematic_one_which_keeps_every_bit():
    bodies = cc.overlapping_pair()
    bodies[1]["props"] = br.props(radius=0.01, restitution=0.8)
    before = cr.state_words(bodies)
    E, n = _table_then_solve(bodies)
    assert n == 2
    solved = cr.clone(bodies)
    cr.solve(solved, E)
    assert _same(cr.state_words(solved)[1], before[1]) and not _same(cr.state_words(solved)[0], before[0])


def test_an_unsigned_body_initiates_nothing():
    """Its volume has no value below zero, so no point of it exists and -- d < 0 never holding -- none of A's points finds it
    either: the entries of both directions are the reference's, nine +0 each, while A meets the floor as if alone."""
    bodies = cc.sunk_sphere() + [cc.body(cc.sphere_unsigned(), dict(cc.BALL, accel=(0.0, 0.0, 0.0)), dict(trans=(1.1, 0.25, 1.0)))]
    E, n = _table_then_solve(bodies)
    assert n == 1 and not _bits(E[1]).any() and not _bits(E[0, 6:]).any() and E[0, 2, 7] == 121


# ---- the step drivers ----
def _falling():
    return [cc.body(cc.sphere(), cc.BALL, dict(trans=(1.0, 0.16, 1.0), lin_vel=(0.0, -1.2, 0.0)))]


@functools.lru_cache(maxsize=None)
def _fifty_single_steps():
    bodies = _falling()
    eng = _loaded(bodies)
    eng.set_option("bodies_contact", cr.WALLS)
    assert eng.get_option("bodies_contact") == 1
    solved = 0
    for k in range(50):
        eng.wcsph_step(1)
        solved += cr.step_dry(bodies, cc.DT, cr.WALLS, 1, cc.BOX_MIN, cc.BOX_MAX)[1]
        assert _same(_states(eng, 1), cr.state_words(bodies)), k
    assert solved >= 2  # it came down, and came down again
    snap = [eng.download("positions"), eng.download("velocities"), _states(eng, 1), np.concatenate(eng.body_state(0)[1:])]
    eng.close()
    return snap


def test_fifty_wcsph_steps_keep_a_falling_sphere_in_the_box_as_the_reference_does():
    snap = _fifty_single_steps()
    assert snap[2][0, 5] - f32(cc.REST_HEIGHT) > cc.BOX_MIN[1] - cc.STEP and not snap[3].any()
    # without the stage it ends below the floor
    free = _falling()
    for _ in range(50):
        cr.step_dry(free, cc.DT, 0, 1, cc.BOX_MIN, cc.BOX_MAX)
    assert free[0]["state"]["trans"][1] < cc.BOX_MIN[1]


def test_one_call_of_fifty_wcsph_steps_equals_fifty_calls_of_one_in_every_byte():
    eng = _loaded(_falling())
    eng.set_option("bodies_contact", cr.WALLS)
    eng.wcsph_step(50)
    got = [eng.download("positions"), eng.download("velocities"), _states(eng, 1), np.concatenate(eng.body_state(0)[1:])]
    for a, b in zip(got, _fifty_single_steps()):
        assert _same(a, b)
    eng.close()


def test_ten_wcsph_steps_with_fluid_equal_the_oracle_the_reference_pass_and_the_reference_contact():
    run = tb._Lockstep()
    p = run.p
    run.eng.set_option("bodies_contact", 3)
    lo, hi = tuple(p.box_min[:]), tuple(p.box_max[:])
    solved, met = 0, np.zeros((2, 8), dtype=bool)
    for _ in range(10):
        run.eng.wcsph_step(1)
        run.ora.wcsph_step(1)
        ids = run.eng.download_ids()
        x, v, hit, responded, run.acc = br.step(run.bodies, run.ora.positions(), run.ora.velocities(), run.mass, ids, run.dt, run.acc)
        E, n = cr.contact(run.bodies, 3, int(p.walls), lo, hi)
        solved += n
        met |= E[:, :, 6] > 0
        run.ora.set_positions(x)
        run.ora.set_velocities(v)
        run.responses += responded.sum(axis=1)
        run.check(x, v)
        assert _same(run.eng.contact_table(), E) and run.eng.get_option("bodies_contacts") == n
    print(f"responses per body {run.responses}, entries solved {solved}")
    # the ball at the foot of the block met the floor, the one that starts beyond box_max.z that wall
    assert (run.responses > 20).all() and solved >= 2 and met[0, 2] and met[1, 5]
    run.eng.close()


def test_one_pcisph_step_is_the_oracle_step_the_reference_pass_and_the_reference_contact():
    eng, p, pos, frc = static_case._dam(EXACT)
    bodies = tb._dynamic_bodies(p)
    for bd in bodies:
        _add(eng, bd)
    eng.set_option("bodies_contact", 3)
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, force=frc)
    ora.delta = p.delta
    eng.pcisph_begin()
    ora.pcisph_begin()
    eng.pcisph_step(1)
    ora.pcisph_step(1)
    x, v, hit, responded, acc = br.step(bodies, ora.positions(), ora.velocities(), float(p.mass), eng.download_ids(), float(p.dt),
                                        np.zeros((2, 6), dtype=f32))
    E, n = cr.contact(bodies, 3, int(p.walls), tuple(p.box_min[:]), tuple(p.box_max[:]))
    assert n >= 1 and _same(eng.download("positions"), x) and _same(eng.download("velocities"), v)
    assert _same(_states(eng, 2), cr.state_words(bodies)) and _same(eng.contact_table(), E)
    eng.close()


def test_with_the_option_or_the_integration_off_no_bit_and_no_byte_changes():
    def run(setup):
        eng = _loaded(_falling())
        setup(eng)
        eng.wcsph_step(50)
        out = [eng.download("positions"), eng.download("velocities"), _states(eng, 1)], eng.get_option("device_bytes")
        eng.close()
        return out
    plain, plain_bytes = run(lambda eng: None)
    assert plain[2][0, 5] < cc.BOX_MIN[1]  # it fell through
    off, off_bytes = run(lambda eng: eng.set_option("bodies_contact", 0))
    assert all(_same(a, b) for a, b in zip(plain, off)) and off_bytes == plain_bytes

    def scripted(eng, contact):
        eng.set_option("bodies_integrate", 0)
        if contact:
            eng.set_option("bodies_contact", 3)
    held, _ = run(lambda eng: scripted(eng, False))
    both, _ = run(lambda eng: scripted(eng, True))
    assert all(_same(a, b) for a, b in zip(held, both)) and _same(both[2], cr.state_words(_falling()))


# ---- other ----
def test_every_refusal_changes_nothing():
    from dieselfluid_amd import DslError
    eng = _engine()
    with pytest.raises(DslError, match="no bodies"):
        eng.contact_pass(3)
    with pytest.raises(DslError, match="unknown body id"):
        eng.contact_points(0)
    for bad in (4, -1, 1.5):
        with pytest.raises(DslError, match="DSL_OPT_BODIES_CONTACT"):
            eng.set_option("bodies_contact", bad)
    assert eng.get_option("bodies_contact") == 0 and eng.get_option("bodies_contacts") == 0
    bodies = cc.sunk_sphere()
    _add(eng, bodies[0])
    bytes_before = eng.get_option("device_bytes")
    for body in (-1, 1, 16):
        with pytest.raises(DslError, match="unknown body id"):
            eng.contact_points(body)
    m = C.c_int64(0)
    assert eng._L.dsl_contact_points(eng._h, 0, None, 5, C.byref(m)) == -1  # cap > 0 without an array
    for kinds in (4, -1, 8):
        with pytest.raises(DslError, match="kinds"):
            eng.contact_pass(kinds)
    with pytest.raises(DslError, match="no detection"):
        eng.contact_table()
    assert eng.get_option("device_bytes") == bytes_before  # nothing was built by a refused call
    eng.contact_pass(1)
    out = np.zeros(64, dtype=f32)
    for count in (0, 62, 64):
        assert eng._L.dsl_contact_table(eng._h, out.ctypes.data_as(C.POINTER(C.c_float)), count) == -1
    assert eng._L.dsl_contact_table(eng._h, None, 63) == -1
    assert b"count" in eng._L.dsl_last_error(eng._h) or b"host" in eng._L.dsl_last_error(eng._h)
    assert not out.any() and _same(_states(eng, 1), cr.state_words(bodies))
    assert _same(eng.contact_table(), cr.detect(bodies, 1, 1, cc.BOX_MIN, cc.BOX_MAX))
    eng.close()
    # a slab handle
    pos, _vel = static_case._particles()
    slab = static_case._engine(static_case.N, FAST)
    slab.upload("positions", pos)
    slab.slab_config(0, -0.5, 0.5)
    assert slab._L.dsl_contact_points(slab._h, 0, None, 0, C.byref(m)) == -4  # DSL_ERR_UNSUPPORTED
    assert slab._L.dsl_contact_pass(slab._h, 3, 0) == -4 and b"slab" in slab._L.dsl_last_error(slab._h)
    assert slab._L.dsl_contact_table(slab._h, out.ctypes.data_as(C.POINTER(C.c_float)), 63) == -4
    slab.close()


def test_clearing_the_bodies_frees_the_lists_and_a_body_added_with_the_option_on_gets_its_list_at_once():
    eng = _engine()
    empty = eng.get_option("device_bytes")
    eng.set_option("bodies_contact", 3)  # (no bodies yet: nothing to build)
    assert eng.get_option("device_bytes") == empty
    first = cc.sunk_sphere()
    _add(eng, first[0])
    with_list = eng.get_option("device_bytes")
    assert eng.contact_points(0)[1] == 656 and eng.get_option("device_bytes") == with_list  # built by dsl_body_add
    eng.wcsph_step(1)
    assert eng.get_option("bodies_contacts") == 1
    eng.clear_bodies()
    assert eng.get_option("bodies") == 0 and eng.get_option("bodies_contacts") == 0
    eng.set_option("bodies_contact", 0)
    assert eng.get_option("device_bytes") < with_list
    second = cc.corner_cube()
    eng.set_option("bodies_contact", 1)
    _add(eng, second[0])
    assert np.array_equal(eng.contact_points(0)[0], cr.points(cc.cube()))
    eng.wcsph_step(1)
    E, n = cr.step_dry(second, cc.DT, 1, 1, cc.BOX_MIN, cc.BOX_MAX)
    assert n == 3 and _same(eng.contact_table(), E) and _same(_states(eng, 1), cr.state_words(second))
    eng.close()


def test_two_runs_agree_byte_for_byte():
    def run():
        eng = _loaded(cc.three_bodies() + cc.corner_cube())
        eng.set_option("bodies_contact", 3)
        eng.wcsph_step(5)
        out = [eng.contact_table(), _states(eng, 4), eng.download("positions")]
        eng.close()
        return out
    a, b = run(), run()
    assert all(_same(x, y) for x, y in zip(a, b)) and a[0][:, :, 7].any()
