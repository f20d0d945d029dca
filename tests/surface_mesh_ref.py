"""numpy restatement of dsl_surface_extract_indexed's rule (include/dslsph.h), on top of surface_ref (the
soup's rule): which lattice edges carry a vertex, the vertex order, the ids of every triangle corner, the positions and the
vertex normals, float32 with one rounding per operation.  It reads neither the product's table nor its code: the triangles'
edges come from surface_ref.CASES, which derives its windings from geometry.

    pos, nrm, idx = mesh(volume, origin, step, dims, iso)   # (V, 3) float32, (V, 3) float32, (T, 3) int32

An edge is (u, d): from voxel u to w = u + (d & 1, (d >> 1) & 1, d >> 2), d in 1..7.
"""
import numpy as np

import surface_ref as ref

VBRICK = (8, 8, 4)  # VOXELS along x, y, z


def _off(d):
    return d & 1, (d >> 1) & 1, d >> 2


def live_cubes(volume, dims):
    """(nz - 1, ny - 1, nx - 1) bool: the cube's 8 corners are finite"""
    nx, ny, nz = (int(d) for d in dims)
    fin = np.isfinite(np.asarray(volume, dtype=np.float32).reshape(nz, ny, nx))
    if min(nx, ny, nz) < 2:
        return np.zeros((max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)), dtype=bool)
    live = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    for c in range(8):
        cx, cy, cz = _off(c)
        live &= fin[cz:nz - 1 + cz, cy:ny - 1 + cy, cx:nx - 1 + cx]
    return live


def vertex_edges(volume, dims, iso):
    """(nz, ny, nx, 8) bool: edge (u, d) carries a vertex (entry d = 0 is unused).  w inside the lattice, exactly one of u, w
    inside the surface, and a live cube with corner 0 at u - s for some s with s & d == 0."""
    nx, ny, nz = (int(d) for d in dims)
    v = np.asarray(volume, dtype=np.float32).reshape(nz, ny, nx)
    with np.errstate(invalid="ignore"):
        inside = v >= np.float32(iso)
    live = live_cubes(volume, dims)
    # livep[k + 1, j + 1, i + 1] = live[k, j, i]: cubes at index -1 and n - 1 do not exist
    livep = np.zeros((nz + 1, ny + 1, nx + 1), dtype=bool)
    livep[1:nz, 1:ny, 1:nx] = live
    has = np.zeros((nz, ny, nx, 8), dtype=bool)
    for d in range(1, 8):
        dx, dy, dz = _off(d)
        held = np.zeros((nz, ny, nx), dtype=bool)
        for s in range(8):
            if s & d:
                continue
            sx, sy, sz = _off(s)
            held |= livep[1 - sz:1 - sz + nz, 1 - sy:1 - sy + ny, 1 - sx:1 - sx + nx]
        cross = np.zeros((nz, ny, nx), dtype=bool)
        cross[:nz - dz, :ny - dy, :nx - dx] = inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]
        has[..., d] = held & cross
    return has


def vertex_order(has, dims):
    """the edges that carry a vertex in the order of their ids: (V,) voxel (linear, x fastest) and (V,) d.  Bricks of 8 x 8 x 4
    voxels ascending, x fastest; inside a brick its voxels ascending, x fastest; inside a voxel d ascending."""
    nx, ny, nz = (int(d) for d in dims)
    k, j, i, d = np.nonzero(has)
    nvx, nvy = -(-nx // VBRICK[0]), -(-ny // VBRICK[1])
    brick = ((k // VBRICK[2]) * nvy + j // VBRICK[1]) * nvx + i // VBRICK[0]
    lane = ((k % VBRICK[2]) * VBRICK[1] + j % VBRICK[1]) * VBRICK[0] + i % VBRICK[0]
    order = np.argsort((brick * 256 + lane) * 8 + d, kind="stable")
    return ((k * ny + j) * nx + i)[order].astype(np.int64), d[order].astype(np.int64)


def gradient(volume, origin, step, dims):
    """(3, nz, ny, nx) float32: per voxel and axis the central difference where both neighbours are usable (inside the lattice
    and finite), the one-sided one where one is, 0 where none is"""
    nx, ny, nz = (int(d) for d in dims)
    v = np.asarray(volume, dtype=np.float32).reshape(nz, ny, nx)
    o = np.asarray(origin, dtype=np.float32).reshape(3)
    s = np.broadcast_to(np.asarray(step, dtype=np.float32), (3,))
    out = np.zeros((3, nz, ny, nx), dtype=np.float32)
    with np.errstate(all="ignore"):
        for a, n in enumerate((nx, ny, nz)):
            axis = 2 - a
            x = o[a] + s[a] * np.arange(-1, n + 1).astype(np.float32)  # x[i + 1] is the coordinate of index i
            assert x.dtype == np.float32
            shape = [1, 1, 1]
            shape[axis] = n
            xp, xm, xq = (x[1 + e:1 + e + n].reshape(shape) for e in (0, -1, 1))
            pad = [(0, 0)] * 3
            pad[axis] = (1, 1)
            vp = np.pad(v, pad, constant_values=np.float32(np.nan))
            sl = lambda e: tuple(slice(1 + e, 1 + e + n) if ax == axis else slice(None) for ax in range(3))
            vm, vq = vp[sl(-1)], vp[sl(1)]
            um, uq = np.isfinite(vm), np.isfinite(vq)
            hi, lo = np.where(uq, vq, v), np.where(um, vm, v)
            xhi, xlo = np.where(uq, xq, xp), np.where(um, xm, xp)
            g = (hi - lo) / (xhi - xlo)
            assert g.dtype == np.float32
            out[a] = np.where(um | uq, g, np.float32(0))
    return out


def triangle_edges(volume, dims, iso):
    """the soup's triangles in the soup's order, corner by corner, as lattice edges: (T, 3) voxel u (linear) and (T, 3) d"""
    nx, ny, nz = (int(d) for d in dims)
    mask, _corner = ref.cube_masks(volume, dims, iso)
    if mask.size == 0:
        return np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)
    m4 = ref.tet_masks(mask)
    per_tet = np.stack([ref.NTRI[t][m4[:, t]] for t in range(6)], axis=1)
    total = per_tet.sum(axis=1)
    order = ref.emit_order(dims)
    start = np.zeros_like(total)
    start[order] = np.cumsum(total[order]) - total[order]
    within = np.cumsum(per_tet, axis=1) - per_tet
    T = int(total.sum())
    eu, ed = np.zeros((T, 3), np.int64), np.zeros((T, 3), np.int64)
    cube = np.arange(mask.size)
    ci, cj, ck = cube % (nx - 1), (cube // (nx - 1)) % (ny - 1), cube // ((nx - 1) * (ny - 1))
    for t in range(6):
        for m in range(16):
            case = ref.CASES[t][m]
            if not case:
                continue
            sel = np.nonzero(m4[:, t] == m)[0]
            sel = sel[mask[sel] != 0]
            if sel.size == 0:
                continue
            for q, tri in enumerate(case):
                at = start[sel] + within[sel, t] + q
                for e, (u, w) in enumerate(tri):
                    assert u < w and (u & (w ^ u)) == 0
                    ux, uy, uz = _off(u)
                    eu[at, e] = ((ck[sel] + uz) * ny + cj[sel] + uy) * nx + ci[sel] + ux
                    ed[at, e] = w ^ u
    return eu, ed


def mesh(volume, origin, step, dims, iso):
    nx, ny, nz = (int(d) for d in dims)
    iso = np.float32(iso)
    v = np.asarray(volume, dtype=np.float32).reshape(-1)
    o = np.asarray(origin, dtype=np.float32).reshape(3)
    s = np.broadcast_to(np.asarray(step, dtype=np.float32), (3,))
    vu_lin, vd = vertex_order(vertex_edges(v, dims, iso), dims)
    V = vu_lin.size
    ids = np.full((nx * ny * nz, 8), -1, dtype=np.int64)
    ids[vu_lin, vd] = np.arange(V)
    dx, dy, dz = vd & 1, (vd >> 1) & 1, vd >> 2
    ui, uj, uk = vu_lin % nx, (vu_lin // nx) % ny, vu_lin // (nx * ny)
    vw_lin = ((uk + dz) * ny + uj + dy) * nx + ui + dx
    g = gradient(v, origin, step, dims).reshape(3, -1)
    pos, nrm = np.zeros((V, 3), np.float32), np.zeros((V, 3), np.float32)
    with np.errstate(all="ignore"):
        f = (iso - v[vu_lin]) / (v[vw_lin] - v[vu_lin])
        G = np.zeros((V, 3), np.float32)
        for a, (idx, dd) in enumerate(((ui, dx), (uj, dy), (uk, dz))):
            xu = o[a] + s[a] * idx.astype(np.float32)
            xw = o[a] + s[a] * (idx + dd).astype(np.float32)
            p = xu + f * (xw - xu)
            Ga = g[a][vu_lin] + f * (g[a][vw_lin] - g[a][vu_lin])
            assert p.dtype == np.float32 and Ga.dtype == np.float32
            pos[:, a], G[:, a] = p, Ga
        ln = np.sqrt((G[:, 0] * G[:, 0] + G[:, 1] * G[:, 1]) + G[:, 2] * G[:, 2])
        ok = ln > 0
        nrm = np.where(ok[:, None], (-G) / np.where(ok, ln, np.float32(1))[:, None], np.float32(0))
    assert nrm.dtype == np.float32
    eu, ed = triangle_edges(v, dims, iso)
    idx = ids[eu, ed]
    assert (idx >= 0).all(), "a triangle corner on an edge without a vertex"
    return pos, nrm, idx.astype(np.int32)


def soup_edge_set(volume, dims, iso):
    """the edges (voxel * 8 + d) that some triangle of the soup touches, sorted"""
    eu, ed = triangle_edges(np.asarray(volume, dtype=np.float32).reshape(-1), dims, iso)
    return np.unique(eu.reshape(-1) * 8 + ed.reshape(-1))


def vertex_edge_set(volume, dims, iso):
    u, d = vertex_order(vertex_edges(volume, dims, iso), dims)
    return np.sort(u * 8 + d)


def closed_by_id(idx):
    """welded by id, zero-area triangles kept: every directed edge occurs once and its reverse once; returns (closed, E)"""
    idx = np.asarray(idx, dtype=np.int64)
    directed = np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]])
    big = int(idx.max(initial=0)) + 1
    code = directed[:, 0] * big + directed[:, 1]
    rev = directed[:, 1] * big + directed[:, 0]
    once = np.unique(code).size == code.size
    closed = bool(once and np.array_equal(np.sort(code), np.sort(rev)))
    E = np.unique(np.sort(directed, axis=1), axis=0).shape[0]
    return closed, E
