"""numpy restatement of the build-defined rule of csrc/bodies.hip (include/dslsph.h: dsl_body_add): several
volume colliders applied in the order they were added, what the fluid hands to each, and the integration of their poses.

numpy float32 with the rounding order written out, as in sdf_ref.py and sdf_rigid_ref.py: every binary operation has float32
operands and numpy rounds its float32 result once, nothing is fused; a dot product is (x0*y0 + x1*y1) + x2*y2.  The pass of
one body is sdf_rigid_ref.rigid_pass itself, the sums are sdf_rigid_ref.fold and accumulate."""
import numpy as np

import sdf_rigid_ref as rr

f32 = np.float32
MAX_BODIES = 16


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _v(a, n):
    a = np.asarray(a, dtype=f32).reshape(-1)
    assert a.size == n
    return a.copy()


def quat_normalize(q):
    """q / |q|, |q| = sqrt(((ww + xx) + yy) + zz), each component divided"""
    q = _v(q, 4)
    return (q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])).astype(f32)


def quat_to_rot(q):
    """the row-major R of q = (w, x, y, z): every product, sum and difference rounded, each parenthesis formed first"""
    w, x, y, z = _v(q, 4)
    one, two = f32(1), f32(2)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return np.array([[one - two * (yy + zz), two * (xy - wz), two * (xz + wy)],
                     [two * (xy + wz), one - two * (xx + zz), two * (yz - wx)],
                     [two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]], dtype=f32)


def axis_angle(axis, angle):
    """a test's orientation: the quaternion of a rotation in float64, rounded to float32 (the library normalises it again)"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a]).astype(f32)


def state(quat=(1, 0, 0, 0), trans=(0, 0, 0), lin_vel=(0, 0, 0), ang_vel=(0, 0, 0)):
    """what dsl_body_set_state stores: the unit quaternion, the three vectors, and R"""
    q = quat_normalize(quat)
    return dict(quat=q, trans=_v(trans, 3), lin_vel=_v(lin_vel, 3), ang_vel=_v(ang_vel, 3), rot=quat_to_rot(q), quat_given=_v(quat, 4))


def props(inv_mass=0, inv_inertia=(0, 0, 0), accel=(0, 0, 0), radius=0, restitution=0):
    return dict(inv_mass=f32(inv_mass), inv_inertia=_v(inv_inertia, 3), accel=_v(accel, 3), radius=f32(radius),
                restitution=f32(restitution))


def body(vol, origin, step, props_, state_=None):
    return dict(vol=np.asarray(vol, dtype=f32), origin=origin, step=step, props=props_, state=state_ if state_ is not None else state())


def api_state(s):
    """the keyword arguments of SPHEngine.add_body / set_body_state for a state of state(): the quaternion as it was given,
    since the library normalises what it gets (a state of integrate() has only its own unit quaternion: pass it through
    state() again for what the library will hold)"""
    out = {k: tuple(float(t) for t in s[k]) for k in ("trans", "lin_vel", "ang_vel")}
    out["quat"] = tuple(float(t) for t in s.get("quat_given", s["quat"]))
    return out


def api_props(p):
    return dict(inv_mass=float(p["inv_mass"]), inv_inertia=tuple(float(t) for t in p["inv_inertia"]),
                accel=tuple(float(t) for t in p["accel"]), radius=float(p["radius"]), restitution=float(p["restitution"]))


def bodies_pass(bodies, pos, vel, mass):
    """The pass: body 0, then 1, ..., each applied to what the one before left.  (pos', vel', hit (K, N) bool, responded (K, N),
    contrib (K, N, 6): J then tau, +0 where the particle did not respond to that body)"""
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    vel = np.asarray(vel, dtype=f32).reshape(-1, 3)
    K, n = len(bodies), pos.shape[0]
    hit, responded, contrib = np.zeros((K, n), dtype=bool), np.zeros((K, n), dtype=bool), np.zeros((K, n, 6), dtype=f32)
    for b, bd in enumerate(bodies):
        p, s = bd["props"], bd["state"]
        pos, vel, hit[b], responded[b], J, tau = rr.rigid_pass(bd["vol"], bd["origin"], bd["step"], pos, vel, p["radius"], p["restitution"],
                                                               mass, s["rot"], s["trans"], s["lin_vel"], s["ang_vel"])
        contrib[b] = np.concatenate([J, tau], axis=1)
    return pos, vel, hit, responded, contrib


def totals(contrib, ids):
    """(K, 6): every body's pass total of its contributions (host order) in the slot order `ids`"""
    return np.stack([rr.fold(c[ids]) for c in contrib]) if len(contrib) else np.zeros((0, 6), dtype=f32)


def body_query(bd, pos):
    s = bd["state"]
    return rr.rigid_query(bd["vol"], bd["origin"], bd["step"], pos, s["rot"], s["trans"])


def integrate(p, s, total, dt):
    """Steps 1 to 5 of include/dslsph.h: the new state of a body with props p and state s after a pass whose total is
    (J, tau) = total.  No gyroscopic term."""
    dt = f32(dt)
    J, tau = _v(total, 6)[:3], _v(total, 6)[3:]
    R, q = s["rot"], s["quat"]
    with np.errstate(all="ignore"):
        lin = (s["lin_vel"] + (J * p["inv_mass"] + p["accel"] * dt)).astype(f32)
        tl = np.array([_dot(R[0, a], R[1, a], R[2, a], tau[0], tau[1], tau[2]) for a in range(3)], dtype=f32)
        wl = (tl * p["inv_inertia"]).astype(f32)
        ang = np.array([s["ang_vel"][a] + _dot(R[a, 0], R[a, 1], R[a, 2], wl[0], wl[1], wl[2]) for a in range(3)], dtype=f32)
        trans = (s["trans"] + dt * lin).astype(f32)
        qw, qx, qy, qz = q
        wx, wy, wz = ang
        d = np.array([-((wx * qx + wy * qy) + wz * qz),
                      qw * wx + (wy * qz - wz * qy),
                      qw * wy + (wz * qx - wx * qz),
                      qw * wz + (wx * qy - wy * qx)], dtype=f32)
        hd = f32(0.5) * dt
        qn = quat_normalize((q + hd * d).astype(f32))
    return dict(quat=qn, trans=trans, lin_vel=lin, ang_vel=ang, rot=quat_to_rot(qn))


def step(bodies, pos, vel, mass, ids, dt, acc, do_integrate=True):
    """One collide pass of a step driver on the oracle's positions and velocities: (pos', vel', hit, responded, acc'); the
    bodies' states are advanced in place."""
    pos, vel, hit, responded, contrib = bodies_pass(bodies, pos, vel, mass)
    tot = totals(contrib, ids)
    acc = np.stack([rr.accumulate(a, t) for a, t in zip(acc, tot)])
    if do_integrate:
        for bd, t in zip(bodies, tot):
            bd["state"] = integrate(bd["props"], bd["state"], t, dt)
    return pos, vel, hit, responded, acc
