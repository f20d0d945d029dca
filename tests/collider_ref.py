"""CPU reference of the triangle-mesh collider: Mesh.Collision (geom/mesh/mesh.go:41-57) through
Triangle.BarycentricCollision / Barycentric (geom/triangle/tri.go:37-101), for many particles at once.

numpy float32 with the rounding order written out: every binary operation below has float32 operands and numpy rounds
its float32 result once; a dot product is (x0*y0 + x1*y1) + x2*y2 (vector.go:268-276); Mag is the float32 sum of squares
followed by a float64 square root rounded to float32 (vector.go:301-308).  The loop over triangles is the reference's
own loop; the particles are the vector axis.
"""
import numpy as np

f32 = np.float32


def _dot(a, b):
    """(a0*b0 + a1*b1) + a2*b2 over the last axis, float32"""
    a = np.asarray(a, dtype=f32)
    b = np.asarray(b, dtype=f32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def mag(a):
    """vector.Mag: float32(sqrt(float64(sum of squares)))"""
    return np.sqrt(_dot(a, a).astype(np.float64)).astype(f32)


def triangle_terms(vertices):
    """per triangle: a, e0 = b - a, e1 = c - a, d00, d01, d11, denom = d00*d11 - d01*d01 (tri.go:81-89)"""
    v = np.asarray(vertices, dtype=f32).reshape(-1, 3, 3)
    a = v[:, 0]
    e0 = v[:, 1] - a
    e1 = v[:, 2] - a
    d00, d01, d11 = _dot(e0, e0), _dot(e0, e1), _dot(e1, e1)
    denom = d00 * d11 - d01 * d01
    return a, e0, e1, d00, d01, d11, denom


def collide(pos, vel, vertices, normals, dt, r):
    """Mesh.Collision(P, V, dt, r) for every particle: (tri, normal, coord, point, k).
    tri: index of the first triangle in list order that collides, -1: none; normal, coord = (u, v, w), point =
    P + V*(-dt) where tri >= 0, zeros elsewhere; k = ((a - P).n) / (n.V) of that triangle (the response's switch)."""
    P = np.ascontiguousarray(pos, dtype=f32).reshape(-1, 3)
    V = np.ascontiguousarray(vel, dtype=f32).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, dtype=f32).reshape(-1, 3)
    a, e0, e1, d00, d01, d11, denom = triangle_terms(vertices)
    n = P.shape[0]
    r = f32(r)
    tri = np.full(n, -1, dtype=np.int32)
    out_n = np.zeros((n, 3), dtype=f32)
    out_c = np.zeros((n, 3), dtype=f32)
    out_k = np.zeros(n, dtype=f32)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        todo = mag(V) != 0  # tri.go:39
        for t in range(a.shape[0]):
            if not todo.any():
                break
            nt = nrm[t][None, :]
            ndr = _dot(nt, V)
            ndr = np.where(ndr == 0, f32(0.0001), ndr).astype(f32)
            d = _dot(a[t][None, :] - P, nt)
            k = d / ndr
            p0 = P + V * k[:, None]
            dist = mag(P - p0)
            near = todo & (dist <= r)  # (False for NaN)
            v2 = P - a[t][None, :]
            d20, d21 = _dot(v2, e0[t][None, :]), _dot(v2, e1[t][None, :])
            u = (d11[t] * d20 - d01[t] * d21) / denom[t]
            v = (d00[t] * d21 - d01[t] * d20) / denom[t]
            w = (one - v) - u
            s = (u + v) + w
            inside = (u <= 1) & (v <= 1) & (w <= 1) & (s <= 1) & (u >= 0) & (v >= 0) & (w >= 0)
            hit = near & inside
            tri[hit] = t
            out_n[hit] = nrm[t]
            out_c[hit] = np.stack([u, v, w], axis=-1)[hit]
            out_k[hit] = k[hit]
            todo &= ~hit
        point = np.where((tri >= 0)[:, None], P + V * (-f32(dt)), f32(0.0)).astype(f32)
    return tri, out_n, out_c, point, out_k


def respond(pos, vel, vertices, normals, dt, r, e):
    """the build-defined response: (positions, velocities, moved).  A colliding particle with k >= 0 goes back to `point`
    and v <- v - n*((1 + e)*(v.n)); a receding one (k < 0) and everything else stays."""
    P = np.ascontiguousarray(pos, dtype=f32).reshape(-1, 3).copy()
    V = np.ascontiguousarray(vel, dtype=f32).reshape(-1, 3).copy()
    tri, nrm, _coord, point, k = collide(P, V, vertices, normals, dt, r)
    with np.errstate(all="ignore"):
        moved = (tri >= 0) & (k >= 0)
        f = (f32(1.0) + f32(e)) * _dot(V, nrm)
        V2 = V - nrm * f[:, None]
    P[moved] = point[moved]
    V[moved] = V2[moved]
    return P, V, moved


def dist_threshold(r):
    """largest float32 s with float32(sqrt(float64(s))) <= r (the host's replacement for Mag in `dist <= r`); -1: none"""
    r = f32(r)
    if not r >= 0:
        return f32(-1.0)
    m = lambda s: f32(np.sqrt(np.float64(s)))
    with np.errstate(over="ignore"):
        s = f32(r * r)
    if not s <= np.finfo(f32).max:
        s = np.finfo(f32).max
    while s > 0 and m(s) > r:
        s = np.nextafter(s, f32(0))
    while np.isfinite(s) and m(np.nextafter(s, f32(np.inf))) <= r:
        s = np.nextafter(s, f32(np.inf))
    return f32(s)


def init_mesh_normals(vertices):
    """mesh.InitMesh's normals (mesh.go:17-37): Norm(Cross(b - a, c - a)) per triangle -- except the LAST triangle, whose
    normal stays zero (the loop stops at i < len(vertices) - 3); the flip towards the origin is computed and dropped."""
    v = np.asarray(vertices, dtype=f32).reshape(-1, 3, 3)
    e0, e1 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    c = np.stack([e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1],
                  e0[:, 2] * e1[:, 0] - e1[:, 2] * e0[:, 0],
                  e0[:, 0] * e1[:, 1] - e1[:, 0] * e0[:, 1]], axis=-1).astype(f32)
    l = mag(c)
    with np.errstate(all="ignore"):
        n = np.where((l != 0)[:, None], c / l[:, None], f32(0.0)).astype(f32)
    if n.shape[0]:
        n[-1] = 0.0
    return n
