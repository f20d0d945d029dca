"""numpy restatement of dsl_surface_extract's rule (include/dslsph.h), vectorised over cubes: marching tetrahedra over the
Kuhn triangulation, float32 with one rounding per operation.  It does not read the product's table
(csrc/surface_table.hpp, tools/make_surface_table.py): the winding of every case is derived here, from float64 geometry --
the affine function that takes the vertex values of a tetrahedron has a gradient, and a triangle's normal has to point
against it, towards lower values.

    verts, norms = extract(volume, origin, step, dims, iso)      # (T, 3, 3) and (T, 3) float32, in the product's order:
                                                                 # bricks of 8 x 8 x 4 cubes, then cubes, tetrahedra, table
"""
import itertools

import numpy as np

TETS = [(0, 1 << a, (1 << a) | (1 << b), 7) for a, b, _c in itertools.permutations(range(3))]


def _offset(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def _case(tet, mask):
    """triangles of one tetrahedron under one 4-bit inside mask: a list of [(u, w)] * 3, cube corners u < w"""
    inside = [m for m in range(4) if (mask >> m) & 1]
    outside = [m for m in range(4) if not (mask >> m) & 1]
    if not inside or not outside:
        return []
    if len(inside) == 1 or len(outside) == 1:
        i = inside[0] if len(inside) == 1 else outside[0]
        tris = [[(i, j) for j in range(4) if j != i]]
    else:
        (a, b), (c, d) = inside, outside
        q = [(a, c), (a, d), (b, d), (b, c)]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    # gradient of the affine function with value 1 at the inside vertices and 0 at the outside ones
    corner = np.array([_offset(c) for c in tet])
    value = np.array([1.0 if m in inside else 0.0 for m in range(4)])
    grad = np.linalg.solve(corner[1:] - corner[0], value[1:] - value[0])
    out = []
    for tri in tris:
        # the surface at value 1/2 crosses every edge in its middle
        p = [0.5 * (corner[m] + corner[n]) for m, n in tri]
        s = float(np.dot(np.cross(p[1] - p[0], p[2] - p[0]), grad))
        assert abs(s) > 1e-9
        pairs = [tuple(sorted((tet[m], tet[n]))) for m, n in tri]
        if s > 0:  # the normal points towards higher values: turn the triangle round
            pairs[1], pairs[2] = pairs[2], pairs[1]
        out.append(pairs)
    return out


CASES = [[_case(tet, mask) for mask in range(16)] for tet in TETS]
NTRI = np.array([[len(CASES[t][m]) for m in range(16)] for t in range(6)], dtype=np.int64)
_EDGE_U = np.zeros((6, 16, 2, 3), dtype=np.int64)
_EDGE_W = np.zeros((6, 16, 2, 3), dtype=np.int64)
for _t in range(6):
    for _m in range(16):
        for _k, _tri in enumerate(CASES[_t][_m]):
            for _e, (_u, _w) in enumerate(_tri):
                _EDGE_U[_t, _m, _k, _e] = _u
                _EDGE_W[_t, _m, _k, _e] = _w


def cube_masks(volume, dims, iso):
    """per cube (x fastest): the 8-bit inside mask, 0 where a corner is not finite; and the corner values (cubes, 8)"""
    nx, ny, nz = (int(d) for d in dims)
    v = np.asarray(volume, dtype=np.float32).reshape(nz, ny, nx)
    if min(nx, ny, nz) < 2:
        return np.zeros(0, np.int64), np.zeros((0, 8), np.float32)
    corner = np.stack([v[(c >> 2) & 1:nz - 1 + ((c >> 2) & 1), (c >> 1) & 1:ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)].reshape(-1)
                       for c in range(8)], axis=1)
    mask = np.zeros(corner.shape[0], dtype=np.int64)
    for c in range(8):
        mask |= (corner[:, c] >= np.float32(iso)).astype(np.int64) << c
    mask[~np.isfinite(corner).all(axis=1)] = 0
    return mask, corner


def tet_masks(mask):
    """(cubes, 6) 4-bit masks of the six tetrahedra"""
    out = np.zeros((mask.shape[0], 6), dtype=np.int64)
    for t, tet in enumerate(TETS):
        for m in range(4):
            out[:, t] |= ((mask >> tet[m]) & 1) << m
    return out


def cube_counts(volume, dims, iso):
    mask, _ = cube_masks(volume, dims, iso)
    if mask.size == 0:
        return mask
    m4 = tet_masks(mask)
    return sum(NTRI[t][m4[:, t]] for t in range(6))


BRICK = (8, 8, 4)  # cubes along x, y, z


def emit_order(dims):
    """The cubes (numbered x fastest) in the order in which their triangles come out: bricks of 8 x 8 x 4 cubes ascending, x
    fastest, and inside a brick its cubes ascending, x fastest."""
    nx, ny, nz = (int(d) for d in dims)
    cube = np.arange((nx - 1) * (ny - 1) * (nz - 1), dtype=np.int64)
    ci, cj, ck = cube % (nx - 1), (cube // (nx - 1)) % (ny - 1), cube // ((nx - 1) * (ny - 1))
    nbx, nby = -(-(nx - 1) // BRICK[0]), -(-(ny - 1) // BRICK[1])
    brick = ((ck // BRICK[2]) * nby + cj // BRICK[1]) * nbx + ci // BRICK[0]
    lane = ((ck % BRICK[2]) * BRICK[1] + cj % BRICK[1]) * BRICK[0] + ci % BRICK[0]
    return np.argsort(brick * (BRICK[0] * BRICK[1] * BRICK[2]) + lane, kind="stable")


def cube_starts(volume, dims, iso):
    """(first triangle, triangles) of every cube, indexed by cube number"""
    counts = cube_counts(volume, dims, iso)
    order = emit_order(dims)
    start = np.zeros_like(counts)
    start[order] = np.cumsum(counts[order]) - counts[order]
    return start, counts


def extract(volume, origin, step, dims, iso):
    nx, ny, nz = (int(d) for d in dims)
    iso = np.float32(iso)
    o = np.asarray(origin, dtype=np.float32).reshape(3)
    s = np.broadcast_to(np.asarray(step, dtype=np.float32), (3,))
    mask, corner = cube_masks(volume, dims, iso)
    if mask.size == 0:
        return np.zeros((0, 3, 3), np.float32), np.zeros((0, 3), np.float32)
    m4_all = tet_masks(mask)
    per_tet_all = np.stack([NTRI[t][m4_all[:, t]] for t in range(6)], axis=1)
    total_all = per_tet_all.sum(axis=1)
    assert total_all.max(initial=0) <= 12
    order = emit_order(dims)
    start_all = np.zeros_like(total_all)
    start_all[order] = np.cumsum(total_all[order]) - total_all[order]
    T = int(total_all.sum())
    verts = np.zeros((T, 3, 3), dtype=np.float32)
    act = np.nonzero(total_all)[0]
    corner, m4, per_tet, start = corner[act], m4_all[act], per_tet_all[act], start_all[act]
    within = np.cumsum(per_tet, axis=1) - per_tet
    ci, cj, ck = act % (nx - 1), (act // (nx - 1)) % (ny - 1), act // ((nx - 1) * (ny - 1))
    idx = np.stack([ci, cj, ck], axis=1)
    # voxel coordinates origin + step * idx: a float32 product, then a float32 sum
    lo = o[None, :] + s[None, :] * idx.astype(np.float32)
    hi = o[None, :] + s[None, :] * (idx + 1).astype(np.float32)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    with np.errstate(all="ignore"):
        for t in range(6):
            for k in range(2):
                sel = np.nonzero(per_tet[:, t] > k)[0]
                if sel.size == 0:
                    continue
                at = start[sel] + within[sel, t] + k
                for e in range(3):
                    u = _EDGE_U[t, m4[sel, t], k, e]
                    w = _EDGE_W[t, m4[sel, t], k, e]
                    vu, vw = corner[sel, u], corner[sel, w]
                    f = (iso - vu) / (vw - vu)
                    for a in range(3):
                        xu = np.where((u >> a) & 1, hi[sel, a], lo[sel, a])
                        xw = np.where((w >> a) & 1, hi[sel, a], lo[sel, a])
                        p = xu + f * (xw - xu)
                        assert p.dtype == np.float32
                        verts[at, e, a] = p
    return verts, normals(verts)


def normals(verts):
    """n = (b - a) x (c - a), every difference and product rounded; / sqrt((nx^2 + ny^2) + nz^2), or 0 when that is not > 0"""
    with np.errstate(all="ignore"):
        a = verts[:, 1] - verts[:, 0]
        b = verts[:, 2] - verts[:, 0]
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]],
                     axis=1)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = ln > 0
        out = np.where(ok[:, None], n / np.where(ok, ln, np.float32(1))[:, None], np.float32(0))
    assert out.dtype == np.float32
    return out


def degenerate(verts):
    """zero area: two of the three vertices are the same bits"""
    b = np.ascontiguousarray(verts, dtype=np.float32).view(np.uint32)
    same = lambda p, q: (b[:, p] == b[:, q]).all(axis=1)
    return same(0, 1) | same(1, 2) | same(0, 2)


def canonical(verts):
    """every triangle rotated so that its byte-wise smallest vertex comes first; a zero-area triangle's vertices sorted (it
    is compared as a multiset).  Returns (T, 9) uint32."""
    b = np.ascontiguousarray(verts, dtype=np.float32).view(np.uint32).reshape(-1, 3, 3).astype(np.uint64)
    T = b.shape[0]
    first = np.zeros(T, dtype=np.int64)
    for cand in (1, 2):
        cur = b[np.arange(T), first]
        new = b[:, cand]
        less = np.zeros(T, dtype=bool)
        tie = np.ones(T, dtype=bool)
        for a in range(3):
            less |= tie & (new[:, a] < cur[:, a])
            tie &= new[:, a] == cur[:, a]
        first = np.where(less, cand, first)
    rot = (first[:, None] + np.arange(3)[None, :]) % 3
    out = b[np.arange(T)[:, None], rot]
    deg = degenerate(verts)
    if deg.any():
        d = out[deg]
        # sort the three vertices of each zero-area triangle lexicographically
        srt = np.empty_like(d)
        for r in range(d.shape[0]):
            srt[r] = np.array(sorted(map(tuple, d[r])), dtype=np.uint64)
        out[deg] = srt
    return out.reshape(T, 9).astype(np.uint32)


def same_triangles(got, want):
    """triangle by triangle, up to rotation (zero-area triangles: as vertex multisets)"""
    return got.shape == want.shape and np.array_equal(canonical(got), canonical(want))


def topology(verts):
    """welding by vertex bits, without the zero-area triangles: (V, E, F, every directed edge is used once and its reverse
    once, signed volume in float64)"""
    keep = ~degenerate(verts)
    v = np.ascontiguousarray(verts[keep], dtype=np.float32)
    F = v.shape[0]
    flat = v.reshape(-1, 3).view(np.uint32)
    uniq, ids = np.unique(flat, axis=0, return_inverse=True)
    ids = ids.reshape(F, 3)
    directed = np.concatenate([ids[:, [0, 1]], ids[:, [1, 2]], ids[:, [2, 0]]])
    code = directed[:, 0].astype(np.int64) * (uniq.shape[0] + 1) + directed[:, 1]
    rev = directed[:, 1].astype(np.int64) * (uniq.shape[0] + 1) + directed[:, 0]
    once = np.unique(code).size == code.size
    closed = bool(once and np.array_equal(np.sort(code), np.sort(rev)))
    E = np.unique(np.sort(directed, axis=1), axis=0).shape[0]
    d = v.astype(np.float64)
    volume = float(np.einsum("ij,ij->i", d[:, 0], np.cross(d[:, 1], d[:, 2])).sum() / 6.0)
    return uniq.shape[0], E, F, closed, volume
