"""CPU: the rule of the rigid bodies (include/dslsph.h: dsl_body_add) as tests/bodies_ref.py restates it -- one body is the
rule of the moving volume collider bit for bit, the order of the bodies matters exactly where two bodies move one particle,
the impulses are the momentum the particles lost, a kinematic body ignores the fluid, the integrator against float64 --
and the names and numbers the header, the Python binding, the Go binding and the C++ mirror give to the new calls.  The
inputs of the GPU cases (tests/bodies_cases.py) are pinned here: what they cover is asserted on the reference alone."""
import os
import re

import numpy as np

import bodies_cases as bc
import bodies_ref as br
import sdf_rigid_ref as rr
import test_gpu_sdf_collider as static_case

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def test_one_body_at_the_identity_is_the_moving_colliders_rule_bit_for_bit():
    vol, (pos, vel) = static_case._volume(), static_case._particles()
    for rest in (0.0, 0.5):
        x, v, hit, responded, contrib = br.bodies_pass([bc.sphere_body(dict(radius=bc.RADIUS, restitution=rest))], pos, vel, 0.37)
        wx, wv, whit, wresp, J, tau = rr.rigid_pass(vol, bc.ORIGIN, bc.STEP, pos, vel, bc.RADIUS, rest, 0.37)
        assert _same(x, wx) and _same(v, wv) and np.array_equal(hit[0], whit) and np.array_equal(responded[0], wresp)
        assert _same(contrib[0], np.concatenate([J, tau], axis=1)) and wresp.sum() > 20
        ids = np.random.default_rng(1).permutation(bc.N)
        assert _same(br.totals(contrib, ids)[0], rr.fold(np.concatenate([J, tau], axis=1)[ids]))
    s = br.state()
    assert _same(s["rot"], np.eye(3, dtype=f32)) and _same(s["quat"], np.array([1, 0, 0, 0], dtype=f32))  # (every zero is +0)


def test_the_pose_of_a_quaternion_is_a_rotation():
    for axis, angle in (((1, 2, 3), 0.7), ((0, 0, 1), np.pi / 2), ((-2, 1, 0.5), 3.0)):
        R = br.quat_to_rot(br.quat_normalize(br.axis_angle(axis, angle) * f32(3.7))).astype(np.float64)  # (any length will do)
        assert np.abs(R @ R.T - np.eye(3)).max() < 4e-7 and abs(np.linalg.det(R) - 1) < 4e-7
        assert np.abs(R - rr.rotation(axis, angle).astype(np.float64)).max() < 4e-7


def test_the_order_of_the_bodies_matters_exactly_where_two_bodies_move_one_particle():
    x, v, hit, responded, contrib = bc.three_bodies_pass()
    both01 = hit[0] & hit[1]
    print(f"hits per body {hit.sum(axis=1)}, responders per body {responded.sum(axis=1)}, moved by bodies 0 and 1: {both01.sum()}, "
          f"by two or more: {(hit.sum(axis=0) >= 2).sum()}")
    assert (hit.sum(axis=0) >= 2).sum() >= 20 and both01.sum() >= 20  # what the GPU cases rely on
    assert (responded.sum(axis=1) >= 20).all()
    assert ((hit.sum(axis=0) == 1).sum() >= 20) and (hit.sum(axis=0) == 0).sum() >= 100
    # bodies 0 and 1 swapped: body 2 still comes last
    sx, sv, shit, sresp, scontrib = bc.three_bodies_pass((1, 0, 2))
    shit = shit[[1, 0, 2]]  # (rows by body again, not by place in the order)
    first_only = hit[0] & ~hit[1] & ~shit[1] & shit[0]  # moved by body 0 alone, whichever order
    second_only = hit[1] & ~hit[0] & ~shit[0] & shit[1]
    untouched_by_both = ~(hit[0] | hit[1] | shit[0] | shit[1])
    same_rows = first_only | second_only | untouched_by_both
    assert first_only.sum() + second_only.sum() >= 20
    assert _same(x[same_rows], sx[same_rows]) and _same(v[same_rows], sv[same_rows])
    moved_by_both = both01 | (shit[0] & shit[1])  # (in either order)
    differs = (_bits(x) != _bits(sx)).any(axis=1)
    assert moved_by_both.sum() >= 20 and differs[moved_by_both].all()


def test_the_bodies_impulses_are_the_momentum_the_particles_lost():
    pos, vel = static_case._particles()
    mass = 0.37
    bodies = bc.three_bodies()
    x, v, hit, responded, contrib = br.bodies_pass(bodies, pos, vel, mass)
    # body by body, for the bound: the velocities each body saw and left
    bound, cx, cv = np.zeros(3), pos, vel
    for bd in bodies:
        nx, nv, _h, resp, _c = br.bodies_pass([bd], cx, cv, mass)
        dv = np.abs(nv.astype(np.float64) - cv.astype(np.float64))
        # per particle and component J = fl(fl(m f) n) against m (v - fl(v - fl(f n))): four half-ulps of m (|v| + |f n|), summed
        bound += (4 * 2.0 ** -24 * float(f32(mass)) * (np.abs(cv.astype(np.float64)) + dv)[resp[0]]).sum(axis=0)
        cx, cv = nx, nv
    assert _same(cx, x) and _same(cv, v)  # (body by body is the pass)
    got = contrib[:, :, :3].astype(np.float64).sum(axis=(0, 1))
    want = -float(f32(mass)) * (v.astype(np.float64) - vel.astype(np.float64)).sum(axis=0)
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)
    assert (np.abs(got) > 100 * bound).any()  # (the bound is no loophole: the sum is far above it)


def test_a_kinematic_body_ignores_the_total_bit_for_bit():
    rng = np.random.default_rng(11)
    p = br.props(radius=0.05, restitution=0.5)  # inv_mass, inv_inertia and accel are zero
    s = br.state(**bc.GENERAL)
    want = br.integrate(p, s, np.zeros(6, dtype=f32), 0.01)
    for _ in range(20):
        total = (rng.standard_normal(6) * 10.0 ** rng.uniform(-3, 3)).astype(f32)
        got = br.integrate(p, s, total, 0.01)
        assert all(_same(got[k], want[k]) for k in want)
    # ... and moves with its velocities
    assert _same(want["lin_vel"], s["lin_vel"]) and _same(want["ang_vel"], s["ang_vel"])
    assert _same(want["trans"], s["trans"] + f32(0.01) * s["lin_vel"]) and not _same(want["quat"], s["quat"])
    # at the identity, at rest, with zeros everywhere, every step is exact
    rest = br.state()
    for _ in range(5):
        rest = br.integrate(p, rest, np.zeros(6, dtype=f32), 0.01)
    assert all(_same(rest[k], br.state()[k]) for k in rest)


# Measured here, the reference against float64 over 1000 steps at dt = 0.002 (t = 2):
#   torque-free spin, w = (0.3, -1.1, 2): |R R^T - I| <= 9.23e-7 at every step; the quaternion is within 2.77e-6 of the exact
#   rotation about w by |w| t (the first-order step turns by 2 atan(|w| dt / 2) instead of |w| dt: 1000 (|w| dt)^3 / 24 = 4.1e-6 in
#   the half angle, times the components' |sin| and |cos|);
#   fall from rest under accel = (0, 0, -9.81): |trans - (a t^2 / 2 + a t dt / 2)| <= 1.82e-5 of 19.6 (the second term is the
#   semi-implicit Euler step's first-order term: lin is advanced before trans).
# Each asserted at four times the measured value.
ORTHO_TOL = 4 * 9.23e-7
SPIN_TOL = 4 * 2.77e-6
FALL_TOL = 4 * 1.82e-5


def test_the_integrator_against_float64():
    dt, steps = 0.002, 1000
    w = np.array([0.3, -1.1, 2.0])
    p = br.props()
    s = br.state(ang_vel=w)
    ortho = 0.0
    for _ in range(steps):
        s = br.integrate(p, s, np.zeros(6, dtype=f32), dt)
        R = s["rot"].astype(np.float64)
        ortho = max(ortho, float(np.abs(R @ R.T - np.eye(3)).max()))
    t = float(f32(dt)) * steps
    half = 0.5 * np.linalg.norm(w) * t
    exact = np.concatenate([[np.cos(half)], np.sin(half) * w / np.linalg.norm(w)])
    spin = float(min(np.abs(s["quat"] - exact).max(), np.abs(s["quat"] + exact).max()))
    a = np.array([0.0, 0.0, -9.81])
    f = br.state()
    pf = br.props(accel=a)
    for _ in range(steps):
        f = br.integrate(pf, f, np.zeros(6, dtype=f32), dt)
    a32, dt32 = a.astype(f32).astype(np.float64), float(f32(dt))
    fall = float(np.abs(f["trans"] - (0.5 * a32 * t * t + 0.5 * a32 * t * dt32)).max())
    print(f"|R R^T - I| = {ortho:.3e}, |q - exact| = {spin:.3e}, |trans - (a t^2 / 2 + a t dt / 2)| = {fall:.3e}")
    assert ortho <= ORTHO_TOL and spin <= SPIN_TOL and fall <= FALL_TOL
    assert _same(f["quat"], br.state()["quat"]) and _same(f["lin_vel"][:2], np.zeros(2, dtype=f32))


def test_the_bindings_agree_on_the_new_names():
    from dieselfluid_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "dslsph.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {"dsl_body_add": 9, "dsl_bodies_clear": 1, "dsl_body_set_state": 3, "dsl_body_set_props": 3, "dsl_body_get_state": 6,
            "dsl_body_query": 4}
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(dsl_bod(?:y|ies)_\w+)\s*\(([^)]*)\)", code)}
    assert {k: len(v.split(",")) for k, v in decl.items()} == want
    assert {k: len(_lib.EXPORTS[k][1]) for k in want} == want
    assert re.search(r"#define\s+DSL_MAX_BODIES\s+16\b", code) and br.MAX_BODIES == 16
    assert re.search(r"\bDSL_OPT_BODIES\s*=\s*78\b", code) and re.search(r"\bDSL_OPT_BODIES_INTEGRATE\s*=\s*79\b", code)
    assert re.search(r"\bDSL_K_COUNT\s*=\s*19\b", code)  # the new launches are timed under DSL_K_COLLIDE
    assert engine.SPHEngine.OPTIONS["bodies"] == 78 and engine.SPHEngine.OPTIONS["bodies_integrate"] == 79
    import ctypes as C
    assert C.sizeof(_lib.BodyProps) == 9 * 4 and C.sizeof(_lib.BodyState) == 13 * 4
    for name in ("add_body", "clear_bodies", "set_body_state", "set_body_props", "body_state", "body_query"):
        assert callable(getattr(engine.SPHEngine, name))
    assert "bodies.hip" in _lib.UNITS
    go = open(os.path.join(ROOT, "bindings", "go", "dslsph", "dslsph.go")).read()
    for name in ["C." + k + "(" for k in want] + ["C.DSL_OPT_BODIES", "C.DSL_OPT_BODIES_INTEGRATE", "C.DSL_MAX_BODIES",
                                                 "func (e *Engine) AddBody(", "func (e *Engine) ClearBodies(", "func (e *Engine) SetBodyState(",
                                                 "func (e *Engine) SetBodyProps(", "func (e *Engine) BodyState(", "func (e *Engine) BodyQuery("]:
        assert name in go, name
    hpp = open(os.path.join(ROOT, "dieselfluid_amd", "host", "dieselfluid.hpp")).read()
    for name in ["struct Body", "struct Bodies"] + [k + "(" for k in want] + ["DSL_OPT_BODIES_INTEGRATE"]:
        assert name in hpp, name
