"""numpy restatement of the build-defined rule of csrc/sdf_rigid.hip (include/dslsph.h: dsl_collider_volume_motion, DESIGN.md
4.6): the volume collider in rigid motion, and the two-level sum of what the fluid hands to the body.

numpy float32 with the rounding order written out, as in sdf_ref.py: every binary operation has float32 operands and numpy
rounds its float32 result once, nothing is fused; a dot product is (x0*y0 + x1*y1) + x2*y2.  The cell evaluation is
sdf_ref.collider_eval itself, at the particle's position in the body's frame."""
import numpy as np

import sdf_ref

f32 = np.float32
BLOCK = 256
IDENTITY = np.eye(3, dtype=f32)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def motion(rot=None, trans=None, lin_vel=None, ang_vel=None):
    """the four arrays in float32, None being the identity / zero (what dsl_collider_volume_motion takes for NULL)"""
    R = IDENTITY if rot is None else np.asarray(rot, dtype=f32).reshape(3, 3)
    t, lv, av = (np.zeros(3, dtype=f32) if a is None else np.asarray(a, dtype=f32).reshape(3) for a in (trans, lin_vel, ang_vel))
    return R, t, lv, av


def rotation(axis, angle):
    """Rodrigues' matrix in float64, rounded to float32 (a test's pose: the library takes R as supplied)"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)).astype(f32)


def rigid_eval(vol, origin, step, pos, R, trans):
    """(q (N, 3), cell, d, n (N, 3) world, mag): q = x - trans, xl = R^T q, sdf_ref.collider_eval at xl, n = R (g / |g|)"""
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q = (pos - trans[None, :]).astype(f32)
        xl = np.stack([_dot(R[0, a], R[1, a], R[2, a], q[:, 0], q[:, 1], q[:, 2]) for a in range(3)], axis=1)
        cell, d, g, mag = sdf_ref.collider_eval(vol, origin, step, xl.astype(f32))
        nl = (g / mag[:, None]).astype(f32)
        n = np.stack([_dot(R[a, 0], R[a, 1], R[a, 2], nl[:, 0], nl[:, 1], nl[:, 2]) for a in range(3)], axis=1).astype(f32)
    return q, cell, d, n, mag


def rigid_query(vol, origin, step, pos, rot=None, trans=None):
    """dsl_collider_volume_query while a motion is set: (dist (N,), world-space normal (N, 3))"""
    R, t, _lv, _av = motion(rot, trans)
    _q, cell, d, n, mag = rigid_eval(vol, origin, step, pos, R, t)
    has_n = cell & (mag > 0)
    return np.where(cell, d, f32(0)).astype(f32), np.where(has_n[:, None], n, f32(0)).astype(f32)


def rigid_pass(vol, origin, step, pos, vel, radius, restitution, mass, rot=None, trans=None, lin_vel=None, ang_vel=None):
    """The collide pass while a motion is set: (pos', vel', hit (N,) bool, responded (N,) bool, J (N, 3), tau (N, 3)); J and tau
    are +0 where the particle did not respond."""
    R, t, lv, av = motion(rot, trans, lin_vel, ang_vel)
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    vel = np.asarray(vel, dtype=f32).reshape(-1, 3)
    q, cell, d, n, mag = rigid_eval(vol, origin, step, pos, R, t)
    with np.errstate(all="ignore"):
        hit = cell & (mag > 0) & (d < f32(radius))
        pen = f32(radius) - d
        new_pos = pos + pen[:, None] * n
        u = np.stack([lv[0] + (av[1] * q[:, 2] - av[2] * q[:, 1]),
                      lv[1] + (av[2] * q[:, 0] - av[0] * q[:, 2]),
                      lv[2] + (av[0] * q[:, 1] - av[1] * q[:, 0])], axis=1).astype(f32)
        r = (vel - u).astype(f32)
        vn = _dot(r[:, 0], r[:, 1], r[:, 2], n[:, 0], n[:, 1], n[:, 2])
        f = (f32(1) + f32(restitution)) * vn
        new_vel = vel - f[:, None] * n
        mf = f32(mass) * f
        J = (mf[:, None] * n).astype(f32)
        tau = np.stack([q[:, 1] * J[:, 2] - q[:, 2] * J[:, 1],
                        q[:, 2] * J[:, 0] - q[:, 0] * J[:, 2],
                        q[:, 0] * J[:, 1] - q[:, 1] * J[:, 0]], axis=1).astype(f32)
        responded = hit & (vn < 0)
    out_pos = np.where(hit[:, None], new_pos, pos).astype(f32)
    out_vel = np.where(responded[:, None], new_vel, vel).astype(f32)
    zero = np.zeros_like(J)
    return out_pos, out_vel, hit, responded, np.where(responded[:, None], J, zero), np.where(responded[:, None], tau, zero)


def _tree(c):
    """(..., 256, K) -> (..., K): for off in 128, 64, ..., 1: c[l] += c[l + off] for l < off"""
    c = np.array(c, dtype=f32)
    off = BLOCK // 2
    while off >= 1:
        c[..., :off, :] = c[..., :off, :] + c[..., off:2 * off, :]
        off //= 2
    return c[..., 0, :]


def partials(contrib):
    """(nb, K): the tree of every workgroup's 256 slots, slots past the last one counting as +0"""
    c = np.asarray(contrib, dtype=f32)
    c = c.reshape(c.shape[0], -1)
    nb = max(1, -(-c.shape[0] // BLOCK))
    padded = np.zeros((nb * BLOCK, c.shape[1]), dtype=f32)
    padded[:c.shape[0]] = c
    return _tree(padded.reshape(nb, BLOCK, c.shape[1]))


def fold(contrib):
    """The pass total of contributions (n_slots, K) in slot order: the workgroups' partials; lane l of 256 adds the partials
    l, l + 256, ... in ascending order from +0 (a missing partial is +0: x + 0 = x, and no sum is ever -0); the same tree over
    the 256 lane sums."""
    part = partials(contrib)
    rows = -(-part.shape[0] // BLOCK)
    padded = np.zeros((rows * BLOCK, part.shape[1]), dtype=f32)
    padded[:part.shape[0]] = part
    lanes = np.zeros((BLOCK, part.shape[1]), dtype=f32)
    for r in range(rows):
        lanes = lanes + padded[r * BLOCK:(r + 1) * BLOCK]
    return _tree(lanes)


def accumulate(acc, total):
    """acc <- acc + total, once per pass"""
    return (np.asarray(acc, dtype=f32) + np.asarray(total, dtype=f32)).astype(f32)
