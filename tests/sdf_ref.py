"""numpy restatement of the two build-defined rules of csrc/sdf.hip (include/dslsph.h): the distance volume
of a triangle mesh (dsl_mesh_distance_volume) and the collision of a particle with a distance volume
(dsl_collider_set_volume).

numpy float32 with the rounding order written out: every binary operation below has float32 operands and numpy rounds its
float32 result once, nothing is fused; a dot product is (x0*y0 + x1*y1) + x2*y2; square roots and divisions are the
correctly rounded ones.  The loop over triangles is brute force (the minimum and the parity do not depend on its order);
the voxels, or the lattice rows, are the vector axis.
"""
import numpy as np

f32 = np.float32
UNSIGNED = 1  # DSL_SDF_UNSIGNED


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def axes(origin, step, dims):
    """the lattice's coordinates per axis: origin + step * float32(idx), each operation rounded once"""
    o = np.broadcast_to(np.asarray(origin, dtype=f32), (3,))
    s = np.broadcast_to(np.asarray(step, dtype=f32), (3,))
    return [(o[a] + s[a] * np.arange(int(dims[a])).astype(f32)).astype(f32) for a in range(3)]


def tri_dist2(px, py, pz, tri, dtype=f32):
    """squared distance of the points to the closest point of one triangle (3, 3): the seven regions on d1..d6, vertex
    regions first, then the edges, then the face.  Non-finite where the branch taken divides zero by zero.  (dtype: the
    same formulas in float64, for the tests' error measurement; px, py, pz must have that type too.)"""
    a, b, c = (np.asarray(tri[k], dtype=dtype) for k in range(3))
    ab, ac, bc = b - a, c - a, c - b
    apx, apy, apz = px - a[0], py - a[1], pz - a[2]
    d1 = _dot(ab[0], ab[1], ab[2], apx, apy, apz)
    d2 = _dot(ac[0], ac[1], ac[2], apx, apy, apz)
    bpx, bpy, bpz = px - b[0], py - b[1], pz - b[2]
    d3 = _dot(ab[0], ab[1], ab[2], bpx, bpy, bpz)
    d4 = _dot(ac[0], ac[1], ac[2], bpx, bpy, bpz)
    cpx, cpy, cpz = px - c[0], py - c[1], pz - c[2]
    d5 = _dot(ab[0], ab[1], ab[2], cpx, cpy, cpz)
    d6 = _dot(ac[0], ac[1], ac[2], cpx, cpy, cpz)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e1, e2 = d4 - d3, d5 - d6
    with np.errstate(all="ignore"):
        t_ab = d1 / (d1 - d3)
        t_ac = d2 / (d2 - d6)
        t_bc = e1 / (e1 + e2)
        s = (va + vb) + vc
        v, w = vb / s, vc / s
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e1 >= 0) & (e2 >= 0)]
        q = []
        for k in range(3):
            one = np.ones_like(px)
            q.append(np.select(conds, [a[k] * one, b[k] * one, c[k] * one, a[k] + ab[k] * t_ab, a[k] + ac[k] * t_ac,
                                       b[k] + bc[k] * t_bc], (a[k] + ab[k] * v) + ac[k] * w).astype(dtype))
        ex, ey, ez = px - q[0], py - q[1], pz - q[2]
        return _dot(ex, ey, ez, ex, ey, ez)


def distance(vertices, origin, step, dims, band=np.inf):
    """(nz, ny, nx) float32: min(sqrt(min_t d2), band); a triangle whose d2 is not finite never wins"""
    tris = np.asarray(vertices, dtype=f32).reshape(-1, 3, 3)
    x, y, z = axes(origin, step, dims)
    pz, py, px = (g.reshape(-1) for g in np.meshgrid(z, y, x, indexing="ij"))
    best = np.full(px.shape, np.inf, dtype=f32)
    for tri in tris:
        d2 = tri_dist2(px, py, pz, tri)
        best = np.where(d2 < best, d2, best)  # (NaN and +inf never win)
    d = np.minimum(np.sqrt(best), f32(band)).astype(f32)
    return d.reshape(int(dims[2]), int(dims[1]), int(dims[0]))


def row_crossings(tri, y, z):
    """For one triangle and the lattice rows (y, z) (arrays of one shape): claim, whether the row's ray towards +x belongs
    to the triangle, and x_hit, where it crosses the triangle's plane."""
    P = np.asarray(tri, dtype=f32).reshape(3, 3)
    claim = np.ones(y.shape, dtype=bool)
    for e in range(3):
        p0, p1, r = P[e], P[(e + 1) % 3], P[(e + 2) % 3]
        swap = (p1[1] < p0[1]) or (p1[1] == p0[1] and p1[2] < p0[2])
        lo, hi = (p1, p0) if swap else (p0, p1)
        dy, dz = hi[1] - lo[1], hi[2] - lo[2]
        if dy == 0 and dz == 0:
            return np.zeros(y.shape, dtype=bool), np.zeros(y.shape, dtype=f32)
        er = dy * (r[2] - lo[2]) - dz * (r[1] - lo[1])
        if not (er > 0 or er < 0):
            return np.zeros(y.shape, dtype=bool), np.zeros(y.shape, dtype=f32)
        ev = dy * (z - lo[2]) - dz * (y - lo[1])
        pos = (ev > 0) | ((ev == 0) & bool(dz <= 0))
        neg = (ev < 0) | ((ev == 0) & bool(dz > 0))
        claim &= pos if er > 0 else neg
    # the rows of the triangle's own projected box only (no rounding in a comparison: this is what lets a sweep visit
    # those rows alone)
    claim &= (y >= P[:, 1].min()) & (y <= P[:, 1].max()) & (z >= P[:, 2].min()) & (z <= P[:, 2].max())
    a, ab, ac = P[0], P[1] - P[0], P[2] - P[0]
    nx = ab[1] * ac[2] - ab[2] * ac[1]
    ny = ab[2] * ac[0] - ab[0] * ac[2]
    nz = ab[0] * ac[1] - ab[1] * ac[0]
    with np.errstate(all="ignore"):
        x_hit = a[0] - (ny * (y - a[1]) + nz * (z - a[2])) / nx
    return claim, x_hit.astype(f32)


def inside(vertices, origin, step, dims):
    """(nz, ny, nx) bool: the ray from the voxel towards +x crosses an odd number of triangles"""
    tris = np.asarray(vertices, dtype=f32).reshape(-1, 3, 3)
    x, y, z = axes(origin, step, dims)
    zz, yy = np.meshgrid(z, y, indexing="ij")
    count = np.zeros((int(dims[2]), int(dims[1]), int(dims[0])), dtype=np.int64)
    for tri in tris:
        claim, x_hit = row_crossings(tri, yy, zz)
        with np.errstate(invalid="ignore"):
            count += claim[:, :, None] & (x_hit[:, :, None] > x[None, None, :])
    return (count & 1) == 1


def volume(vertices, origin, step, dims, band=np.inf, flags=0):
    """dsl_mesh_distance_volume: (nz, ny, nx) float32"""
    d = distance(vertices, origin, step, dims, band)
    if flags & UNSIGNED:
        return d
    return np.where(inside(vertices, origin, step, dims), -d, d).astype(f32)


# ---- the collider ----
def _lerp(a, b, t):
    return a + t * (b - a)


def collider_eval(vol, origin, step, pos):
    """The cell, d, g and |g| of every position: (cell (N,) bool, d (N,), g (N, 3), mag (N,)).  cell: every index
    floor((x - origin) / step) lies in [0, n - 2], the eight corners and x are finite."""
    vol = np.asarray(vol, dtype=f32)
    nz, ny, nx = vol.shape
    o = np.broadcast_to(np.asarray(origin, dtype=f32), (3,))
    s = np.broadcast_to(np.asarray(step, dtype=f32), (3,))
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    n = pos.shape[0]
    dims = (nx, ny, nz)
    cell = np.ones(n, dtype=bool)
    idx, t = [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            u = (pos[:, a] - o[a]) / s[a]
            fl = np.floor(u)
            ok = (fl >= 0) & (fl <= f32(dims[a] - 2))  # (false for NaN and the infinities)
            cell &= ok
            fl = np.where(ok, fl, f32(0))
            idx.append(fl.astype(np.int64))
            t.append((u - fl).astype(f32))
        i, j, k = idx
        c = [[[vol[k + dk, j + dj, i + di] for di in (0, 1)] for dj in (0, 1)] for dk in (0, 1)]  # c[dk][dj][di]
        for dk in (0, 1):
            for dj in (0, 1):
                for di in (0, 1):
                    cell &= np.isfinite(c[dk][dj][di])
        tx, ty, tz = t
        e00, e10 = _lerp(c[0][0][0], c[0][0][1], tx), _lerp(c[0][1][0], c[0][1][1], tx)  # e[dj][dk]
        e01, e11 = _lerp(c[1][0][0], c[1][0][1], tx), _lerp(c[1][1][0], c[1][1][1], tx)
        f0, f1 = _lerp(e00, e10, ty), _lerp(e01, e11, ty)
        d = _lerp(f0, f1, tz)
        gz = (f1 - f0) / s[2]
        gy = (_lerp(e10, e11, tz) - _lerp(e00, e01, tz)) / s[1]
        x0 = _lerp(_lerp(c[0][0][0], c[0][1][0], ty), _lerp(c[1][0][0], c[1][1][0], ty), tz)
        x1 = _lerp(_lerp(c[0][0][1], c[0][1][1], ty), _lerp(c[1][0][1], c[1][1][1], ty), tz)
        gx = (x1 - x0) / s[0]
        mag = np.sqrt(_dot(gx, gy, gz, gx, gy, gz))
    g = np.stack([gx, gy, gz], axis=1).astype(f32)
    return cell, d.astype(f32), g, mag.astype(f32)


def collider_query(vol, origin, step, pos):
    """dsl_collider_volume_query: (dist (N,), normal (N, 3)); zeros where there is no cell, a zero normal where |g| is not > 0"""
    cell, d, g, mag = collider_eval(vol, origin, step, pos)
    with np.errstate(all="ignore"):
        n = g / mag[:, None]
    has_n = cell & (mag > 0)
    return np.where(cell, d, f32(0)).astype(f32), np.where(has_n[:, None], n, f32(0)).astype(f32)


def collider_pass(vol, origin, step, pos, vel, radius, restitution):
    """dsl_collide_pass against a volume: (pos', vel', hit (N,) bool)"""
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    vel = np.asarray(vel, dtype=f32).reshape(-1, 3)
    cell, d, g, mag = collider_eval(vol, origin, step, pos)
    with np.errstate(all="ignore"):
        hit = cell & (d < f32(radius)) & (mag > 0)
        n = (g / mag[:, None]).astype(f32)
        pen = f32(radius) - d
        new_pos = pos + pen[:, None] * n
        vn = _dot(vel[:, 0], vel[:, 1], vel[:, 2], n[:, 0], n[:, 1], n[:, 2])
        f = (f32(1) + f32(restitution)) * vn
        new_vel = vel - f[:, None] * n
    out_pos = np.where(hit[:, None], new_pos, pos).astype(f32)
    out_vel = np.where((hit & (vn < 0))[:, None], new_vel, vel).astype(f32)
    return out_pos, out_vel, hit
