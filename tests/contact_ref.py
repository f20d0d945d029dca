"""numpy restatement of the build-defined rule of csrc/contact.hip (include/dslsph.h: dsl_contact_points): the
rigid bodies' contact points, the detection against the wall box and against each other, and the solve.

numpy float32 with the rounding order written out, as in bodies_ref.py: every binary operation has float32 operands and numpy
rounds its float32 result once, nothing is fused; a dot product is (x0*y0 + x1*y1) + x2*y2, a cross product has each product
and difference rounded.  A body is bodies_ref.body's dict; the evaluation of a point against a body is
sdf_rigid_ref.rigid_eval, the sums are sdf_rigid_ref.fold."""
import copy

import numpy as np

import bodies_ref as br
import sdf_rigid_ref as rr

f32 = np.float32
WALLS, BODIES = 1, 2


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], dtype=f32)


def points(vol):
    """the contact points of a volume (nz, ny, nx): voxels whose value is finite and <= 0 with at least one axis neighbour
    inside the lattice that is finite and > 0, as int32 linear indices (x fastest), ascending"""
    v = np.asarray(vol, dtype=f32)
    with np.errstate(invalid="ignore"):
        inside = np.isfinite(v) & (v <= 0)
        outside = np.isfinite(v) & (v > 0)
    near = np.zeros(v.shape, dtype=bool)
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        near[tuple(lo)] |= outside[tuple(hi)]
        near[tuple(hi)] |= outside[tuple(lo)]
    return np.flatnonzero((inside & near).reshape(-1)).astype(np.int32)


def point_coords(origin, step, dims, idx):
    """(M, 3): origin + step * (float)index per axis, the rule of dsl_field_volume; dims = (nx, ny, nz)"""
    o, s = np.asarray(origin, dtype=f32), np.asarray(step, dtype=f32)
    idx = np.asarray(idx, dtype=np.int64)
    nx, ny = int(dims[0]), int(dims[1])
    ijk = np.stack([idx % nx, (idx // nx) % ny, idx // (nx * ny)], axis=1).astype(f32)
    return (o[None, :] + s[None, :] * ijk).astype(f32)


def body_points(bd):
    vol = bd["vol"]
    return point_coords(bd["origin"], bd["step"], vol.shape[::-1], points(vol))


def contributions(bodies, kinds, walls, box_min, box_max):
    """{(A, t): (M_A, 9)}: per point of A and target t the eight sums' terms and the depth, nine +0 where the point does not
    contribute; targets that are off are left out (their entry is nine +0)"""
    lo, hi = np.asarray(box_min, dtype=f32), np.asarray(box_max, dtype=f32)
    out = {}
    for A, a in enumerate(bodies):
        pl = body_points(a)
        R, tr = a["state"]["rot"], a["state"]["trans"]
        with np.errstate(all="ignore"):
            q = np.stack([_dot(R[c, 0], R[c, 1], R[c, 2], pl[:, 0], pl[:, 1], pl[:, 2]) for c in range(3)], axis=1).astype(f32)
            x = (tr[None, :] + q).astype(f32)

        def entry(on, pen, n):
            with np.errstate(all="ignore"):
                c = np.concatenate([pen[:, None] * q, pen[:, None] * n, pen[:, None], np.ones_like(pen)[:, None], pen[:, None]],
                                   axis=1).astype(f32)
            return np.where(on[:, None], c, f32(0)).astype(f32)

        if (kinds & WALLS) and walls:
            for ax in range(3):
                for side in range(2):
                    with np.errstate(all="ignore"):
                        pen = (lo[ax] - x[:, ax]) if side == 0 else (x[:, ax] - hi[ax])
                    n = np.zeros((len(pl), 3), dtype=f32)
                    n[:, ax] = f32(1) if side == 0 else f32(-1)
                    out[(A, 2 * ax + side)] = entry(pen > 0, pen.astype(f32), n)
        if kinds & BODIES:
            for B, b in enumerate(bodies):
                if B == A:
                    continue
                s = b["state"]
                _r, cell, d, n, mag = rr.rigid_eval(b["vol"], b["origin"], b["step"], x, s["rot"], s["trans"])
                with np.errstate(all="ignore"):
                    on = cell & (mag > 0) & (d < 0)
                    pen = (-d).astype(f32)
                out[(A, 6 + B)] = entry(on, pen, n)
    return out


def table_of(contrib, K):
    """E (K, 6 + K, 9) = (S[3], N[3], W, C, D): the eight sums in the fold's order (workgroups of 256 points, the tree, the
    partials lane-strided from +0, the tree again), the depth the maximum"""
    E = np.zeros((K, 6 + K, 9), dtype=f32)
    for (A, t), c in contrib.items():
        if len(c):  # (a body without points: nine +0)
            E[A, t, :8] = rr.fold(c[:, :8])
            E[A, t, 8] = c[:, 8].max()
    return E


def detect(bodies, kinds, walls, box_min, box_max):
    return table_of(contributions(bodies, kinds, walls, box_min, box_max), len(bodies))


def _iw(s, p, t):
    """the integration's step 2 on a vector: tl = R^T t, wl_a = tl_a inv_inertia_a, R wl"""
    R = s["rot"]
    tl = np.array([_dot(R[0, a], R[1, a], R[2, a], t[0], t[1], t[2]) for a in range(3)], dtype=f32)
    wl = (tl * p["inv_inertia"]).astype(f32)
    return np.array([_dot(R[a, 0], R[a, 1], R[a, 2], wl[0], wl[1], wl[2]) for a in range(3)], dtype=f32)


def solve(bodies, E):
    """The solve over the table, A ascending and inside A t ascending, on the bodies' states in place (new arrays: a state
    that was shared is not written through).  Returns the number of entries that got past k > 0."""
    K = len(bodies)
    done = 0
    zero3 = np.zeros(3, dtype=f32)
    with np.errstate(all="ignore"):
        for A in range(K):
            for t in range(6 + K):
                S, N, W, D = E[A, t, 0:3], E[A, t, 3:6], E[A, t, 6], E[A, t, 8]
                if not W > 0:
                    continue
                wall = t < 6
                a, pa = bodies[A]["state"], bodies[A]["props"]
                qc = (S / W).astype(f32)
                if wall:
                    n = np.zeros(3, dtype=f32)
                    n[t >> 1] = f32(-1) if (t & 1) else f32(1)
                else:
                    b, pb = bodies[t - 6]["state"], bodies[t - 6]["props"]
                    ln = np.sqrt(_dot(N[0], N[1], N[2], N[0], N[1], N[2]))
                    if not ln > 0:
                        continue
                    n = (N / ln).astype(f32)
                tA = _iw(a, pa, _cross(qc, n))
                y = _cross(tA, qc)
                k = pa["inv_mass"] + _dot(y[0], y[1], y[2], n[0], n[1], n[2])
                rB, tB = zero3, zero3
                if not wall:
                    rB = ((a["trans"] + qc) - b["trans"]).astype(f32)
                    tB = _iw(b, pb, _cross(rB, n))
                    y = _cross(tB, rB)
                    kB = pb["inv_mass"] + _dot(y[0], y[1], y[2], n[0], n[1], n[2])
                    k = k + kB
                if not k > 0:
                    continue
                done += 1
                uA = (a["lin_vel"] + _cross(a["ang_vel"], qc)).astype(f32)
                uB = zero3 if wall else (b["lin_vel"] + _cross(b["ang_vel"], rB)).astype(f32)
                r = (uA - uB).astype(f32)
                vn = _dot(r[0], r[1], r[2], n[0], n[1], n[2])
                if vn < 0:
                    e = pa["restitution"] if wall else min(pa["restitution"], pb["restitution"])
                    f = (f32(1) + e) * vn
                    j = (-f) / k
                    a["lin_vel"] = (a["lin_vel"] + (j * pa["inv_mass"]) * n).astype(f32)
                    a["ang_vel"] = (a["ang_vel"] + j * tA).astype(f32)
                    if not wall:
                        b["lin_vel"] = (b["lin_vel"] - (j * pb["inv_mass"]) * n).astype(f32)
                        b["ang_vel"] = (b["ang_vel"] - j * tB).astype(f32)
                if wall:
                    if pa["inv_mass"] > 0:
                        a["trans"] = (a["trans"] + D * n).astype(f32)
                else:
                    s = pa["inv_mass"] + pb["inv_mass"]
                    if s > 0:
                        a["trans"] = (a["trans"] + ((f32(0.5) * D) * (pa["inv_mass"] / s)) * n).astype(f32)
                        b["trans"] = (b["trans"] - ((f32(0.5) * D) * (pb["inv_mass"] / s)) * n).astype(f32)
    return done


def contact(bodies, kinds, walls, box_min, box_max):
    """detection at the bodies' poses and the solve behind it, in place: (E, entries past k > 0)"""
    E = detect(bodies, kinds, walls, box_min, box_max)
    return E, solve(bodies, E)


def clone(bodies):
    """bodies whose states may be solved without touching the originals (the volumes are shared)"""
    return [dict(bd, state=copy.deepcopy(bd["state"]), props=bd["props"]) for bd in bodies]


def step_dry(bodies, dt, kinds, walls, box_min, box_max):
    """a step driver's act on the bodies when no particle touches them: the integration with a zero total, then the contact"""
    zero = np.zeros(6, dtype=f32)
    for bd in bodies:
        bd["state"] = br.integrate(bd["props"], bd["state"], zero, dt)
    return contact(bodies, kinds, walls, box_min, box_max) if kinds else (None, 0)


def state_words(bodies):
    """(K, 13): quat, trans, lin_vel, ang_vel of every body -- dsl_body_state's words"""
    return np.stack([np.concatenate([bd["state"][k] for k in ("quat", "trans", "lin_vel", "ang_vel")]) for bd in bodies]).astype(f32)
