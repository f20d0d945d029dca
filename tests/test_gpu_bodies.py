"""GPU: rigid bodies (include/dslsph.h: dsl_body_add and its calls; csrc/bodies.hip: k_bodies_pass, k_body_query,
k_bodies_fold) against tests/bodies_ref.py, the numpy float32 restatement of the build-defined rule: the pass over the
bodies in order, the two-level sums per body, the integration of the poses.  One arithmetic in both math modes and a fixed
order of additions: every check of a device result is an equality, bit for bit.  The inputs are pinned in
tests/bodies_cases.py; tests/test_bodies_cpu.py asserts on the reference what they cover."""
import ctypes as C
import functools

import numpy as np
import pytest

import bodies_cases as bc
import bodies_ref as br
import helpers
import sdf_rigid_ref as rr
import test_gpu_sdf_collider as static_case  # its sphere volume with the NaN voxel, its cloud of 1000, its dam-break handles
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = 0, 1
ORIGIN, STEP, RADIUS, N = bc.ORIGIN, bc.STEP, bc.RADIUS, bc.N
STATE_KEYS = ("quat", "trans", "lin_vel", "ang_vel")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _loaded(math_mode):
    pos, vel = static_case._particles()
    eng = static_case._engine(N, math_mode)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.nn()  # slots in cell order, as the step drivers have them
    return eng


def _add(eng, bd):
    return eng.add_body(bd["vol"], bd["origin"], bd["step"], br.api_props(bd["props"]), br.api_state(bd["state"]))


def _acc(eng, b, reset=False):
    _s, imp, trq = eng.body_state(b, reset=reset)
    return np.concatenate([imp, trq])


def _state_is(eng, b, want):
    got = eng.body_state(b)[0]
    return all(_same(got[k], want[k]) for k in STATE_KEYS)


def _xv(eng):
    return eng.download("positions"), eng.download("velocities")


# ---- case 1: one kinematic body at the identity is the static volume collider ----
@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_a_kinematic_body_at_the_identity_gives_the_static_pass_bit_for_bit(math_mode):
    vol = static_case._volume()
    eng, static = _loaded(math_mode), _loaded(math_mode)
    static.set_collider_volume(vol, ORIGIN, STEP, radius=RADIUS, restitution=0.5)
    assert eng.get_option("bodies") == 0
    assert _add(eng, bc.sphere_body(dict(radius=RADIUS, restitution=0.5))) == 0
    assert eng.get_option("bodies") == 1 and eng.get_option("bodies_integrate") == 1
    for got, want in zip(eng.body_query(0), static.collider_volume_query()):
        assert _same(got, want)
    assert np.array_equal(eng.download_ids(), static.download_ids())
    eng.collide()
    static.collide()
    for got, want in zip(_xv(eng), _xv(static)):
        assert _same(got, want)
    assert eng.get_option("collide_hits") == static.get_option("collide_hits") > 100
    assert _acc(eng, 0).any() and _state_is(eng, 0, br.state())
    eng.close()
    static.close()


def test_a_kinematic_body_at_the_identity_keeps_every_bit_of_its_state_over_five_steps():
    vol = static_case._sphere_volume(static_case.DAM_O, static_case.DAM_S, static_case.DAM_D, static_case.DAM_C, static_case.DAM_R)
    eng, p, _pos, _frc = static_case._dam(EXACT)
    static, _p, _pos, _frc = static_case._dam(EXACT)
    radius = 0.5 * float(p.h)
    static.set_collider_volume(vol, static_case.DAM_O, static_case.DAM_S, radius=radius, restitution=0.3)
    eng.add_body(vol, static_case.DAM_O, static_case.DAM_S, dict(radius=radius, restitution=0.3))
    eng.wcsph_step(5)
    static.wcsph_step(5)
    for got, want in zip(_xv(eng), _xv(static)):
        assert _same(got, want)
    assert eng.get_option("collide_hits") == static.get_option("collide_hits")
    want = br.state()
    got = eng.body_state(0)[0]
    assert all(not (_bits(got[k]) ^ _bits(want[k])).any() for k in STATE_KEYS)  # (every zero is +0 still)
    assert _acc(eng, 0)[:3].any()
    eng.close()
    static.close()


# ---- case 2: a general pose ----
@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_one_body_at_a_general_pose_equals_the_reference_and_the_moving_volume_collider(math_mode):
    vol, (pos, vel) = static_case._volume(), static_case._particles()
    bd = bc.sphere_body(dict(radius=RADIUS, restitution=0.5), bc.GENERAL)
    eng, old = _loaded(math_mode), _loaded(math_mode)
    _add(eng, bd)
    assert _state_is(eng, 0, bd["state"])
    s = bd["state"]
    old.set_collider_volume(vol, ORIGIN, STEP, radius=RADIUS, restitution=0.5)
    old.set_collider_volume_motion(rot=s["rot"], trans=s["trans"], lin_vel=s["lin_vel"], ang_vel=s["ang_vel"])
    want_d, want_n = br.body_query(bd, pos)
    for got, want, other in zip(eng.body_query(0), (want_d, want_n), old.collider_volume_query()):
        assert _same(got, want) and _same(got, other)
    x, v, hit, responded, contrib = br.bodies_pass([bd], pos, vel, float(eng.params.mass))
    assert responded.sum() >= 30
    ids = eng.download_ids()
    eng.collide()
    old.collide()
    for got, want, other in zip(_xv(eng), (x, v), _xv(old)):
        assert _same(got, want) and _same(got, other)
    assert eng.get_option("collide_hits") == old.get_option("collide_hits") == int(hit.sum())
    got = _acc(eng, 0)
    assert _same(got, br.totals(contrib, ids)[0]) and _same(got, np.concatenate(old.collider_volume_impulse())) and got.all()
    assert _state_is(eng, 0, bd["state"])  # (dsl_collide_pass does not integrate)
    eng.close()
    old.close()


# ---- cases 3 and 4: three bodies, two of them overlapping; the impulses per body ----
@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_three_bodies_in_order_equal_the_reference_and_hand_each_body_its_own_impulse(math_mode):
    bodies = bc.three_bodies()
    x, v, hit, responded, contrib = bc.three_bodies_pass()
    eng = _loaded(math_mode)
    assert float(eng.params.mass) == 1.0
    assert [_add(eng, bd) for bd in bodies] == [0, 1, 2] and eng.get_option("bodies") == 3
    ids = eng.download_ids()
    eng.collide()
    gx, gv = _xv(eng)
    assert _same(gx, x) and _same(gv, v)
    assert eng.get_option("collide_hits") == int(hit.sum())  # (particle, body) pairs
    want = br.totals(contrib, ids)
    c64 = contrib.astype(np.float64)
    for b in range(3):
        got = _acc(eng, b)
        assert _same(got, want[b]), b
        bound = N * 2.0 ** -24 * np.abs(c64[b]).sum(axis=0)
        assert (np.abs(got - c64[b].sum(axis=0)) <= bound).all() and (np.abs(got[:3]) > 10 * bound[:3]).any(), b
    # the other order is another pass
    swapped = _loaded(math_mode)
    for b in (1, 0, 2):
        _add(swapped, bodies[b])
    swapped.collide()
    sx, sv, _h, _r, _c = bc.three_bodies_pass((1, 0, 2))
    assert _same(swapped.download("positions"), sx) and _same(swapped.download("velocities"), sv) and not _same(sx, x)
    eng.close()
    swapped.close()


# ---- case 5: more workgroups than the fold has lanes ----
def test_the_folds_second_trip_with_three_bodies_on_290_workgroups():
    """74,088 slots are 290 workgroups: lanes 0 .. 33 of each body's fold add two partials.  Body 0 (the sphere at the foot of
    the block, turned and lifted) has responders all over; body 1 comes down on the block's top layer, whose slots are the
    last ones; body 2 is nowhere near the fluid."""
    from dieselfluid_amd import SPHEngine, scenes
    p, pos = scenes.dambreak_scene(42, math_mode=FAST)
    assert pos.shape[0] == 74088 > 65536
    radius, mass, dt = 0.5 * float(p.h), float(p.mass), float(p.dt)
    foot = static_case._sphere_volume(static_case.DAM_O, static_case.DAM_S, static_case.DAM_D, static_case.DAM_C, static_case.DAM_R)
    ball_o = (-0.4, -0.4, -0.4)
    ball = static_case._sphere_volume(ball_o, static_case.DAM_S, static_case.DAM_D, np.zeros(3), 0.25)  # centred on its own frame's origin
    top = float(pos[:, 2].max())
    bodies = [
        br.body(foot, static_case.DAM_O, static_case.DAM_S, br.props(radius=radius, restitution=0.3),
                br.state(quat=br.axis_angle((0, 0, 1), 0.3), trans=(0.02, 0.0, 0.35), lin_vel=(-0.5, 0.1, 0.0), ang_vel=(0.0, 0.0, 1.0))),
        br.body(ball, ball_o, static_case.DAM_S, br.props(radius=radius, restitution=0.0),
                br.state(quat=br.axis_angle((1, 0, 0), 0.4), trans=(0.5, 0.5, top - 0.02 + 0.25 + radius), lin_vel=(0.0, 0.0, -0.5))),
        br.body(ball, ball_o, static_case.DAM_S, br.props(inv_mass=2.0, inv_inertia=(1.0, 2.0, 3.0), accel=(0.0, 0.0, -9.81), radius=radius),
                br.state(quat=br.axis_angle((1, 1, 0), 0.2), trans=(5.0, 5.0, 5.0), lin_vel=(0.1, 0.2, 0.3), ang_vel=(0.4, -0.5, 0.6))),
    ]
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.nn()
    for bd in bodies:
        _add(eng, bd)
    ids = eng.download_ids()
    x, v, hit, responded, contrib = br.bodies_pass(bodies, pos, np.zeros_like(pos), mass)
    groups = np.zeros((3, 290 * 256), dtype=bool)
    groups[:, :ids.size] = responded[:, ids]
    groups = groups.reshape(3, 290, 256).any(axis=2)
    print(f"hits {hit.sum(axis=1)}, responding {responded.sum(axis=1)}, workgroups with a responder {groups.sum(axis=1)}, "
          f"of the last 34: {groups[:, 256:].sum(axis=1)}")
    assert groups[0].sum() >= 20 and groups[0, 256:].any() and groups[0, :256].any()
    assert groups[1, 256:].any() and not groups[1, :256].any() and responded[1].sum() >= 20
    assert not hit[2].any()
    eng.collide()
    gx, gv = _xv(eng)
    assert _same(gx, x) and _same(gv, v)
    assert eng.get_option("collide_hits") == int(hit.sum()) > 1000
    want = br.totals(contrib, ids)
    for b in range(3):
        assert _same(_acc(eng, b), want[b]), b
    assert want[0][:3].all() and want[1][2] != 0 and not _bits(want[2]).any()
    assert all(_state_is(eng, b, bodies[b]["state"]) for b in range(3))
    # a step driver integrates: the body without a responder moves by its accel and its velocities alone
    eng.wcsph_step(1)
    assert _state_is(eng, 2, br.integrate(bodies[2]["props"], bodies[2]["state"], np.zeros(6, dtype=f32), dt))
    assert not _bits(_acc(eng, 2)).any() and not _state_is(eng, 0, bodies[0]["state"])
    eng.close()


# ---- case 6: accumulation and reset ----
def _two_passes():
    pos, vel = static_case._particles()
    bodies = bc.three_bodies()[:2]
    eng = _loaded(FAST)
    for bd in bodies:
        _add(eng, bd)
    ids = eng.download_ids()
    seen, acc, x, v = [], np.zeros((2, 6), dtype=f32), pos, vel
    # body 0 changes its course between the passes: a particle it has just reflected recedes from it until it does
    second = dict(bc.GENERAL, trans=(0.0, 0.02, 0.0), lin_vel=(-1.5, 1.0, -1.0))
    for k in range(2):
        if k == 1:
            bodies[0]["state"] = br.state(**second)
            eng.set_body_state(0, **br.api_state(bodies[0]["state"]))
        eng.collide()
        x, v, hit, responded, contrib = br.bodies_pass(bodies, x, v, 1.0)
        assert responded.sum(axis=1).min() >= 5
        acc = np.stack([rr.accumulate(a, t) for a, t in zip(acc, br.totals(contrib, ids))])
        seen.append(np.stack([_acc(eng, b) for b in range(2)]))
        assert _same(seen[-1], acc)
    assert not _same(seen[0], seen[1])
    seen.append(_acc(eng, 0, reset=True))  # returns the sum ...
    assert _same(seen[-1], acc[0])
    assert not _bits(_acc(eng, 0)).any() and _same(_acc(eng, 1), acc[1])  # ... and leaves +0, in that body alone
    eng.collide()
    x, v, hit, responded, contrib = br.bodies_pass(bodies, x, v, 1.0)
    tot = br.totals(contrib, ids)
    seen.append(np.stack([_acc(eng, b) for b in range(2)]))
    assert _same(seen[-1][0], tot[0]) and _same(seen[-1][1], rr.accumulate(acc[1], tot[1]))
    state = list(_xv(eng)) + seen
    assert _same(state[0], x) and _same(state[1], v)
    eng.close()
    return state


def test_two_passes_accumulate_reset_zeroes_and_a_repeated_run_gives_the_same_bytes():
    first, again = _two_passes(), _two_passes()
    for a, b in zip(first, again):
        assert _same(a, b)


# ---- cases 7 to 9 and 12: the WCSPH driver with dynamic bodies ----
BALL_O = (-0.4, -0.4, -0.4)


@functools.lru_cache(maxsize=None)
def _ball():
    vol = static_case._sphere_volume(BALL_O, static_case.DAM_S, static_case.DAM_D, np.zeros(3), static_case.DAM_R)
    vol.setflags(write=False)
    return vol


def _dynamic_bodies(p, count=2):
    """spheres with their frames at their centres (the centre of mass), finite mass and inertia, under gravity: one at the foot
    of the dam-break block, moving into it, one coming down on its top"""
    radius, g = 0.5 * float(p.h), tuple(float(t) for t in p.force_reset[:])
    assert any(g)
    return [
        br.body(_ball(), BALL_O, static_case.DAM_S, br.props(inv_mass=0.02, inv_inertia=(0.5, 0.6, 0.7), accel=g, radius=radius, restitution=0.3),
                br.state(quat=br.axis_angle((0, 0, 1), 0.2), trans=static_case.DAM_C, lin_vel=(-0.6, 0.2, 0.1), ang_vel=(0.0, 0.0, 2.0))),
        br.body(_ball(), BALL_O, static_case.DAM_S, br.props(inv_mass=0.05, inv_inertia=(1.5, 1.0, 2.0), accel=g, radius=radius, restitution=0.0),
                br.state(quat=br.axis_angle((1, 2, 3), 0.7), trans=(0.4, 0.5, 1.15), lin_vel=(0.1, 0.0, -1.0), ang_vel=(0.5, -1.0, 0.8))),
    ][:count]


class _Lockstep:
    """a handle, the oracle and the reference bodies, advanced together one step at a time and compared after each"""

    def __init__(self, count=2):
        self.eng, self.p, pos, frc = static_case._dam(EXACT)
        self.mass, self.dt = float(self.p.mass), float(self.p.dt)
        assert self.mass != 1.0  # (the product mass f is exercised)
        self.ora = po.OracleSPH.from_state(helpers.oracle_params(self.p), pos, force=frc)
        self.bodies = _dynamic_bodies(self.p, count)
        for bd in self.bodies:
            _add(self.eng, bd)
        self.acc = np.zeros((count, 6), dtype=f32)
        self.responses = np.zeros(count, dtype=np.int64)

    def step(self, do_integrate=True):
        self.eng.wcsph_step(1)
        self.ora.wcsph_step(1)
        ids = self.eng.download_ids()  # (the pass ran on the slots the step's sort left)
        x, v, hit, responded, self.acc = br.step(self.bodies, self.ora.positions(), self.ora.velocities(), self.mass, ids, self.dt,
                                                 self.acc, do_integrate)
        self.ora.set_positions(x)
        self.ora.set_velocities(v)
        self.responses += responded.sum(axis=1)
        self.check(x, v)
        assert self.eng.get_option("collide_hits") == int(hit.sum())

    def check(self, x, v):
        gx, gv = _xv(self.eng)
        assert _same(gx, x) and _same(gv, v)
        for b, bd in enumerate(self.bodies):
            assert _state_is(self.eng, b, bd["state"]), b
            assert _same(_acc(self.eng, b), self.acc[b]), b

    def snapshot(self):
        out = list(_xv(self.eng))
        for b in range(len(self.bodies)):
            s = self.eng.body_state(b)[0]
            out += [s[k] for k in STATE_KEYS] + [_acc(self.eng, b)]
        return out


@functools.lru_cache(maxsize=None)
def _ten_single_steps():
    run = _Lockstep()
    plain, _p, _pos, _frc = static_case._dam(EXACT)
    for k in range(10):
        run.step()
        if k == 0:  # dsl_stats stay what Update saw
            plain.wcsph_step(1)
            assert run.eng.stats().max_vel == plain.stats().max_vel and run.eng.stats().max_f == plain.stats().max_f
    print(f"responses per body over ten steps: {run.responses}")
    assert (run.responses > 20).all() and run.acc[:, :3].any(axis=1).all() and run.acc[:, 3:].any(axis=1).all()
    assert not _same(run.bodies[0]["state"]["ang_vel"], _dynamic_bodies(run.p)[0]["state"]["ang_vel"])  # (the fluid turned it)
    snap = run.snapshot()
    run.eng.close()
    plain.close()
    return snap


def test_ten_wcsph_steps_with_two_dynamic_bodies_equal_the_oracle_the_reference_pass_and_the_reference_integration():
    _ten_single_steps()


def test_one_call_of_ten_wcsph_steps_equals_ten_calls_of_one_in_every_byte():
    eng, p, _pos, _frc = static_case._dam(EXACT)
    for bd in _dynamic_bodies(p):
        _add(eng, bd)
    eng.wcsph_step(10)
    got = list(_xv(eng))
    for b in range(2):
        s = eng.body_state(b)[0]
        got += [s[k] for k in STATE_KEYS] + [_acc(eng, b)]
    for a, b in zip(got, _ten_single_steps()):
        assert _same(a, b)
    eng.close()


def test_one_body_equals_the_moving_volume_collider_with_a_host_that_integrates_the_pose():
    new, p, _pos, _frc = static_case._dam(EXACT)
    old, _p, _pos, _frc = static_case._dam(EXACT)
    bd = _dynamic_bodies(p, 1)[0]
    _add(new, bd)
    pr, s = bd["props"], bd["state"]
    old.set_collider_volume(bd["vol"], bd["origin"], bd["step"], radius=float(pr["radius"]), restitution=float(pr["restitution"]))
    acc = np.zeros(6, dtype=f32)
    for _ in range(10):
        old.set_collider_volume_motion(rot=s["rot"], trans=s["trans"], lin_vel=s["lin_vel"], ang_vel=s["ang_vel"])
        old.wcsph_step(1)
        total = np.concatenate(old.collider_volume_impulse(reset=True))  # (from +0: the pass total itself)
        acc = rr.accumulate(acc, total)
        s = br.integrate(pr, s, total, float(p.dt))
    new.wcsph_step(10)
    for got, want in zip(_xv(new), _xv(old)):
        assert _same(got, want)
    assert _state_is(new, 0, s) and _same(_acc(new, 0), acc) and acc.all()
    new.close()
    old.close()


# ---- case 10: the PCISPH driver ----
def test_one_pcisph_step_is_the_oracle_step_the_reference_pass_and_the_reference_integration():
    eng, p, pos, frc = static_case._dam(EXACT)
    bodies = _dynamic_bodies(p)
    for bd in bodies:
        _add(eng, bd)
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, force=frc)
    ora.delta = p.delta
    eng.pcisph_begin()
    ora.pcisph_begin()
    eng.pcisph_step(1)
    ora.pcisph_step(1)
    x, v, hit, responded, acc = br.step(bodies, ora.positions(), ora.velocities(), float(p.mass), eng.download_ids(), float(p.dt),
                                        np.zeros((2, 6), dtype=f32))
    assert responded[0].sum() > 5
    gx, gv = _xv(eng)
    assert _same(gx, x) and _same(gv, v)
    # the predictor state is not touched
    assert _same(eng.download("pci_positions"), ora.pci_positions()) and _same(eng.download("pci_velocities"), ora.pci_velocities())
    assert eng.get_option("collide_hits") == int(hit.sum())
    for b, bd in enumerate(bodies):
        assert _state_is(eng, b, bd["state"]) and _same(_acc(eng, b), acc[b]), b
    eng.close()


# ---- case 11: DSL_OPT_BODIES_INTEGRATE = 0 ----
def test_without_integration_the_poses_stay_and_the_impulses_accumulate():
    run = _Lockstep()
    run.eng.set_option("bodies_integrate", 0)
    assert run.eng.get_option("bodies_integrate") == 0
    start = [dict(bd["state"]) for bd in run.bodies]
    for _ in range(3):
        run.step(do_integrate=False)
    assert all(_state_is(run.eng, b, start[b]) for b in range(2)) and run.acc[0, :3].all()
    run.eng.set_option("bodies_integrate", 1)
    run.step()
    assert not _state_is(run.eng, 0, start[0])
    run.eng.close()


# ---- case 12: state and props changed between steps ----
def test_a_state_and_props_set_between_steps_hold_from_the_next_step_on():
    run = _Lockstep()
    run.step()
    run.step()
    # the state the library holds goes through dsl_body_set_state again (and is normalised again), the props change
    s = run.bodies[0]["state"]
    moved = br.state(quat=s["quat"], trans=s["trans"] + f32(0.01), lin_vel=(-0.3, 0.0, 0.2), ang_vel=s["ang_vel"])
    run.bodies[0]["state"] = moved
    run.eng.set_body_state(0, **br.api_state(moved))
    pr = br.props(inv_mass=0.1, inv_inertia=(0.0, 2.0, 0.0), accel=(0.0, 0.0, 1.0), radius=float(run.bodies[1]["props"]["radius"]) * 1.5,
                  restitution=0.7)
    run.bodies[1]["props"] = pr
    run.eng.set_body_props(1, **br.api_props(pr))
    assert _state_is(run.eng, 0, moved)
    run.step()
    run.step()
    assert (run.responses > 5).all()
    run.eng.close()


# ---- case 13: dsl_bodies_clear ----
def test_clearing_the_bodies_restores_the_plain_steps_bits():
    eng, p, _pos, _frc = static_case._dam(EXACT)
    plain, _p, _pos, _frc = static_case._dam(EXACT)
    _add(eng, _dynamic_bodies(p)[0])
    eng.clear_bodies()
    before = eng.get_option("device_bytes")  # (with the hit counter, which a handle's first collider of any kind allocates)
    for bd in _dynamic_bodies(p):
        _add(eng, bd)
    assert eng.get_option("device_bytes") > before
    eng.clear_bodies()
    assert eng.get_option("bodies") == 0 and eng.get_option("device_bytes") == before
    eng.clear_bodies()  # (nothing to clear: no error)
    eng.wcsph_step(3)
    plain.wcsph_step(3)
    for got, want in zip(_xv(eng), _xv(plain)):
        assert _same(got, want)
    eng.collide()  # no bodies: no launch, no bit changes
    assert _same(eng.download("positions"), plain.download("positions"))
    # ... and the ids start again at 0
    assert _add(eng, _dynamic_bodies(p)[1]) == 0 and not _bits(_acc(eng, 0)).any()
    eng.close()
    plain.close()


# ---- case 14: the skin step is not taken ----
def test_the_skin_option_changes_nothing_while_bodies_exist():
    out = []
    for skin in (0.0, 0.1):
        eng, p, _pos, _frc = static_case._dam(FAST)
        eng.set_option("skin", skin)
        for bd in _dynamic_bodies(p):
            _add(eng, bd)
        eng.wcsph_step(5)
        assert eng.get_option("skin_steps") == 0
        out.append(list(_xv(eng)) + [eng.body_state(b)[0][k] for b in range(2) for k in STATE_KEYS] + [_acc(eng, b) for b in range(2)])
        eng.close()
    for a, b in zip(*out):
        assert _same(a, b)
    assert out[0][-2].any()


# ---- case 15: refusals ----
def _raw_add(eng, vol, origin=ORIGIN, step=STEP, dims=None, props=None, state=None, dev=None, host=True, with_props=True):
    """the raw call: (return code, dsl_last_error)"""
    from dieselfluid_amd import _lib
    vol = np.ascontiguousarray(vol, dtype=f32)
    o, s = np.array(origin, dtype=f32), np.array(step, dtype=f32)
    d = np.array(vol.shape[::-1] if dims is None else dims, dtype=np.int32)
    pr = eng._body_props(**(props or dict(radius=RADIUS, restitution=0.5)))
    st = eng._body_state(**state) if state else None
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = eng._L.dsl_body_add(eng._h, C.c_void_p(dev) if dev else None, fp(vol) if host else None, fp(o), fp(s),
                             d.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(pr) if with_props else None,
                             C.byref(st) if st is not None else None, None)
    return rc, eng._L.dsl_last_error(eng._h)


def test_every_refusal_leaves_the_state_and_the_bodies_as_they_were():
    from dieselfluid_amd import DslError, scenes
    vol, (pos, vel) = static_case._volume(), static_case._particles()
    eng = _loaded(FAST)
    bd = bc.sphere_body(dict(radius=RADIUS, restitution=0.5), bc.GENERAL)
    _add(eng, bd)
    bytes_before = eng.get_option("device_bytes")
    nan, inf = float("nan"), float("inf")
    bad_adds = [
        (dict(host=False), b"exactly one"), (dict(dev=1 << 20), b"exactly one"),
        (dict(dims=(12, 11, 1)), b"dims"), (dict(step=(0.1, 0.0, 0.1)), b"step"), (dict(step=(0.1, nan, 0.1)), b"step"),
        (dict(origin=(0.0, inf, 0.0)), b"origin"), (dict(with_props=False), b"props"),
        (dict(props=dict(inv_mass=-1.0)), b"inv_mass"), (dict(props=dict(inv_inertia=(0.0, -1.0, 0.0))), b"inv_inertia"),
        (dict(props=dict(radius=-0.1)), b"radius"), (dict(props=dict(accel=(0.0, nan, 0.0))), b"props"),
        (dict(props=dict(restitution=inf)), b"props"), (dict(props=dict(inv_mass=inf)), b"props"),
        (dict(state=dict(quat=(0.0, 0.0, 0.0, 0.0))), b"quat"), (dict(state=dict(quat=(1.0, nan, 0.0, 0.0))), b"state"),
        (dict(state=dict(trans=(0.0, 0.0, inf))), b"state"), (dict(state=dict(ang_vel=(nan, 0.0, 0.0))), b"state"),
    ]
    for kw, word in bad_adds:
        rc, msg = _raw_add(eng, vol, **kw)
        assert rc == -1 and b"dsl_body_add" in msg and word in msg, (kw, rc, msg)
    # an unknown body id, a bad state, bad props: by name
    for body in (-1, 1, 16):
        with pytest.raises(DslError, match="unknown body id"):
            eng.body_state(body)
        with pytest.raises(DslError, match="unknown body id"):
            eng.set_body_state(body)
        with pytest.raises(DslError, match="unknown body id"):
            eng.set_body_props(body, radius=0.1)
        with pytest.raises(DslError, match="unknown body id"):
            eng.body_query(body)
    with pytest.raises(DslError, match="quat"):
        eng.set_body_state(0, quat=(0.0, 0.0, 0.0, 0.0))
    with pytest.raises(DslError, match="state"):
        eng.set_body_state(0, lin_vel=(0.0, nan, 0.0))
    with pytest.raises(DslError, match="inv_mass"):
        eng.set_body_props(0, inv_mass=-2.0)
    with pytest.raises(DslError, match="props"):
        eng.set_body_props(0, radius=nan)
    assert eng._L.dsl_body_set_state(eng._h, 0, None) == -1 and eng._L.dsl_body_set_props(eng._h, 0, None) == -1
    # the three kinds of collider exclude each other, in both directions
    verts, normals = scenes.box_mesh((0.05, -0.1, 0.0), (1.3, 1.1, 1.2))
    with pytest.raises(DslError, match="dsl_bodies_clear"):
        eng.set_collider_mesh(verts, normals, 0.1, 0.0)
    with pytest.raises(DslError, match="dsl_bodies_clear"):
        eng.set_collider_volume(vol, ORIGIN, STEP, radius=RADIUS, restitution=0.5)
    assert eng.get_option("collider_triangles") == 0 and eng.get_option("collider_volume") == 0
    with pytest.raises(DslError, match="slab"):
        eng.slab_config(0, -0.5, 0.5)
    # nothing changed: one body, its state, the bytes, and the pass is the reference's
    assert eng.get_option("bodies") == 1 and eng.get_option("device_bytes") == bytes_before and _state_is(eng, 0, bd["state"])
    assert _same(eng.download("positions"), pos) and _same(eng.download("velocities"), vel)
    x, v, hit, responded, contrib = br.bodies_pass([bd], pos, vel, 1.0)
    eng.collide()
    gx, gv = _xv(eng)
    assert _same(gx, x) and _same(gv, v)
    # a seventeenth body
    for k in range(1, 16):
        assert _add(eng, bd) == k
    full = eng.get_option("device_bytes")
    rc, msg = _raw_add(eng, vol)
    assert rc == -1 and b"DSL_MAX_BODIES" in msg and eng.get_option("bodies") == 16 and eng.get_option("device_bytes") == full
    eng.close()
    # a mesh or a volume that is set refuses a body, and says what to remove
    for which in ("mesh", "volume"):
        other = _loaded(FAST)
        if which == "mesh":
            other.set_collider_mesh(verts, normals, 0.1, 0.0)
        else:
            other.set_collider_volume(vol, ORIGIN, STEP, radius=RADIUS, restitution=0.5)
        rc, msg = _raw_add(other, vol)
        assert rc == -1 and (b"dsl_collider_set_mesh" if which == "mesh" else b"dsl_collider_set_volume") in msg
        assert other.get_option("bodies") == 0
        other.close()


def test_a_slab_handle_is_refused():
    pos, _vel = static_case._particles()
    eng = static_case._engine(N, FAST)
    eng.upload("positions", pos)
    eng.slab_config(0, -0.5, 0.5)
    rc, msg = _raw_add(eng, static_case._volume())
    assert rc == -4 and b"slab" in msg  # DSL_ERR_UNSUPPORTED
    assert eng._L.dsl_body_get_state(eng._h, 0, None, None, None, 0) == -4
    assert eng.get_option("bodies") == 0
    eng.close()


# ---- case 16: life cycle ----
def test_device_bytes_rise_with_each_body_fall_on_clear_and_a_handle_is_destroyed_with_bodies_set():
    vol = static_case._volume()
    eng = _loaded(FAST)
    _add(eng, bc.three_bodies()[0])
    eng.body_query(0)
    eng.clear_bodies()  # (the hit counter and the query's staging array stay with the handle)
    seen = [eng.get_option("device_bytes")]
    for k in range(3):
        _add(eng, bc.three_bodies()[k])
        seen.append(eng.get_option("device_bytes"))
        # the volume's copy and six partial sums for each of the four workgroups, per body
        assert seen[-1] - seen[-2] >= vol.size * 4 + 6 * 4 * 4
    eng.collide()
    eng.body_query(1)
    eng.clear_bodies()
    assert eng.get_option("device_bytes") == seen[0]
    _add(eng, bc.three_bodies()[0])
    eng.collide()
    eng.close()  # with a body set
