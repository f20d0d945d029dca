"""Initial conditions and parameter sets (host side, numpy only).

* reference_scene: sph.Init's lattice on [-1,1)^3 (geom/grid/point-grid.go:33-63,
  model/field/sph_field.go:87-108) with the reference constants.
* dambreak_scene: the build's synthetic dam-break -- no reference
  counterpart; the oracle carries an independent C restatement of the same generator and
  tests/test_scenes.py checks the two agree bit for bit.
"""
from __future__ import annotations

import numpy as np

from ._lib import Params
from .engine import reference_params

f32 = np.float32


def lattice_positions(n3: int, origin=(0.0, 0.0, 0.0)) -> np.ndarray:
    """pos[id = k + n3*(i*n3 + j)] = min + step*(i,j,k); float32 operation order of
    BuildKernGrid / GridPosition (point-grid.go:26-28,39-40,60-63)."""
    origin = np.asarray(origin, dtype=f32)
    if origin.shape != (3,):  # V.Add length mismatch -> (0,0,0) (vector.go:171-173)
        minb = np.zeros(3, dtype=f32)
    else:
        minb = (f32(-1.0) * np.ones(3, dtype=f32) + origin).astype(f32)
    inv = f32(1.0) / f32(n3)
    step = (inv * (minb * f32(-2.0)).astype(f32)).astype(f32)
    i, j, k = np.meshgrid(np.arange(n3), np.arange(n3), np.arange(n3), indexing="ij")
    ijk = np.stack([i, j, k], axis=-1).reshape(-1, 3).astype(f32)  # id order = i-major, k fastest
    return (minb[None, :] + (step[None, :] * ijk).astype(f32)).astype(f32)


def volume_points(origin, step, dims) -> np.ndarray:
    """(nx * ny * nz, 3) float32: the voxel coordinates of SPHEngine.field_volume, in its output order (x fastest).  Voxel
    (i, j, k) lies at origin[a] + step[a] * float32(idx[a]) per axis: one float32 multiplication, one float32 addition
    (grid.Grid.GridPosition, point-grid.go:59-63) -- the library's rule, bit for bit.  `step` is one number or three."""
    o = np.broadcast_to(np.asarray(origin, dtype=f32), (3,))
    s = np.broadcast_to(np.asarray(step, dtype=f32), (3,))
    ax = [(o[a] + (s[a] * np.arange(int(dims[a])).astype(f32)).astype(f32)).astype(f32) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], axis=-1).reshape(-1, 3)


def reference_scene(n3: int, grid_half_extent: float = 4.0):
    """(params, positions) for sph.Init(1.0, {0,0,0}, nil, n3, pci) in grid mode."""
    p = reference_params(n3)
    for a in range(3):
        p.grid_min[a] = -grid_half_extent
        p.grid_max[a] = grid_half_extent
    return p, lattice_positions(n3)


def _splitmix64(seed: int, counters: np.ndarray) -> np.ndarray:
    """counter-based splitmix64: mix(seed + (c+1)*0x9E3779B97F4A7C15), vectorised."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (counters.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dambreak_positions(n3: int, dx: float, jitter: float = 0.05, seed: int = 1234) -> np.ndarray:
    """Fluid block of n3^3 particles at ((i,j,k)+0.5)*dx with +-jitter*dx uniform jitter
    from splitmix64(seed, 3*id + axis), id = k + n3*(i*n3 + j)."""
    n = n3 ** 3
    r = _splitmix64(seed, np.arange(3 * n, dtype=np.uint64))
    u = ((r >> np.uint64(40)).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)
    jit = ((u * f32(2.0) - f32(1.0)).astype(f32) * f32(f32(jitter) * f32(dx))).astype(f32)
    i, j, k = np.meshgrid(np.arange(n3), np.arange(n3), np.arange(n3), indexing="ij")
    ijk = np.stack([i, j, k], axis=-1).reshape(-1, 3).astype(f32)
    base = ((ijk + f32(0.5)).astype(f32) * f32(dx)).astype(f32)
    return (base + jit.reshape(-1, 3)).astype(f32)


def dambreak_slab_ids(n3: int, axis: int, l0: int, l1: int) -> np.ndarray:
    """ids (k + n3*(i*n3 + j)) of the lattice layers l0 <= index < l1 along `axis`
    (0: i/x, 1: j/y, 2: k/z), ascending."""
    rng = [np.arange(n3)] * 3
    rng = list(rng)
    rng[axis] = np.arange(l0, l1)
    i, j, k = np.meshgrid(rng[0], rng[1], rng[2], indexing="ij")
    ids = (k + n3 * (i * n3 + j)).reshape(-1)
    return np.sort(ids).astype(np.int32)


def dambreak_positions_ids(n3: int, dx: float, ids, jitter: float = 0.05, seed: int = 1234) -> np.ndarray:
    """dambreak_positions restricted to the given particle ids (same values bit for bit)."""
    ids = np.asarray(ids, dtype=np.int64)
    k = ids % n3
    j = (ids // n3) % n3
    i = ids // (n3 * n3)
    ctr = (3 * ids[:, None] + np.arange(3)[None, :]).reshape(-1).astype(np.uint64)
    r = _splitmix64(seed, ctr)
    u = ((r >> np.uint64(40)).astype(f32) * f32(1.0 / 16777216.0)).astype(f32)
    jit = ((u * f32(2.0) - f32(1.0)).astype(f32) * f32(f32(jitter) * f32(dx))).astype(f32)
    ijk = np.stack([i, j, k], axis=-1).astype(f32)
    base = ((ijk + f32(0.5)).astype(f32) * f32(dx)).astype(f32)
    return (base + jit.reshape(-1, 3)).astype(f32)


def lattice_rest_density(h_over_dx: float, mass: float, dx: float) -> float:
    """Density the reference kernel (kernel/std_kernel.go:33-39) gives an interior particle
    of a perfect cubic lattice, self term excluded as in SPHField.Density."""
    h = h_over_dx * dx
    A = 315.0 / (64.0 * 3.141592653589 * h ** 3)
    r = int(np.ceil(h_over_dx)) + 1
    o = np.arange(-r, r + 1)
    ox, oy, oz = np.meshgrid(o, o, o, indexing="ij")
    d2 = (ox * ox + oy * oy + oz * oz).astype(np.float64) * dx * dx
    mask = (d2 > 0) & (d2 < h * h)
    q = 1.0 - d2[mask] / (h * h)
    return float(mass * A * np.sum(q * q))


def dambreak_scene(n3: int, *, h_over_dx: float = 2.0, jitter: float = 0.05, seed: int = 1234, fluid_edge: float = 1.0,
                   rho_phys: float = 1000.0, cfl: float = 0.25, visc: float = 0.02, math_mode: int = 1,
                   positions: bool = True):
    """(params, positions) of the synthetic dam-break: fluid block [0,L]^3 in the corner of a
    4L x 2L x L box, h = h_over_dx*dx, gravity -y, wall box = clamp + reflect.  All force
    terms use the reference's formulas (kernel, Tait EOS, Gradient, LaplacianForce, Update);
    the switches that are unphysical for m != 1 are set to their physical values
    (pressure repels, viscosity without the running-mass product, single gravity)."""
    L = float(fluid_edge)
    dx = L / n3
    h = h_over_dx * dx
    mass = rho_phys * dx ** 3
    rho0 = lattice_rest_density(h_over_dx, mass, dx)
    g = 9.81
    c_s = 10.0 * np.sqrt(2.0 * g * L)
    dt = cfl * h / c_s
    p = reference_params(4)  # reference constants as the starting point
    p.n_particles = n3 ** 3
    p.lsh_bucket_size = int(np.float32(p.n_particles // 255) * np.float32(1.5))
    p.dt = dt
    p.mass = mass
    p.h = h
    p.ref_density = rho0
    p.eos_d0_grad = rho0
    # reference Gradient carries rho_i*m instead of m_i*m_j (sph_field.go:199): absorb the
    # extra rho/m into the stiffness so that the sound speed is c_s
    p.eos_w = c_s * c_s * mass
    p.mu = visc * mass * dx * c_s
    p.pressure_sign = -1.0
    p.visc_running_mass = 0
    p.force_reset[0], p.force_reset[1], p.force_reset[2] = 0.0, -g * mass, 0.0
    p.external[0] = p.external[1] = p.external[2] = 0.0
    p.wcsph_pressure_force = 1
    p.wcsph_viscosity = 1
    p.walls = 1
    box = (4.0 * L, 2.0 * L, 1.0 * L)
    for a in range(3):
        p.box_min[a] = 0.0
        p.box_max[a] = box[a]
        p.grid_min[a] = -h
        p.grid_max[a] = box[a] + h
    p.restitution = 0.0
    p.math_mode = math_mode
    pos = dambreak_positions(n3, dx, jitter, seed) if positions else None
    return p, pos


def quad_mesh(p0, p1, p2, p3, normal, subdiv: int = 1):
    """(vertices (T, 3, 3), normals (T, 3)), float32: the quad p0 p1 p2 p3 (corners in order around it) as 2 * subdiv^2
    triangles with `normal` on every one -- as supplied: a collider's normals are neither normalised nor checked
    (SPHEngine.set_collider_mesh)."""
    c = [np.asarray(q, dtype=np.float64) for q in (p0, p1, p2, p3)]
    s = int(subdiv)

    def at(i, j):  # bilinear
        u, v = i / s, j / s
        return (1 - u) * (1 - v) * c[0] + u * (1 - v) * c[1] + u * v * c[2] + (1 - u) * v * c[3]

    tris = []
    for i in range(s):
        for j in range(s):
            a, b, cc, d = at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)
            tris.append((a, b, cc))
            tris.append((a, cc, d))
    verts = np.asarray(tris, dtype=f32).reshape(-1, 3, 3)
    normals = np.tile(np.asarray(normal, dtype=f32).reshape(1, 3), (verts.shape[0], 1))
    return verts, normals


def box_mesh(center, size, subdiv: int = 1):
    """(vertices, normals) of an axis-aligned box obstacle: six faces of 2 * subdiv^2 triangles each (12, 192, 3072
    triangles for subdiv 1, 4, 16), unit outward normals."""
    ctr = np.asarray(center, dtype=np.float64)
    half = 0.5 * np.asarray(size, dtype=np.float64)
    vs, ns = [], []
    for axis in range(3):
        a1, a2 = (axis + 1) % 3, (axis + 2) % 3
        for sign in (-1.0, 1.0):
            corners = []
            for s1, s2 in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                q = ctr.copy()
                q[axis] += sign * half[axis]
                q[a1] += s1 * half[a1]
                q[a2] += s2 * half[a2]
                corners.append(q)
            nrm = np.zeros(3)
            nrm[axis] = sign
            v, n = quad_mesh(*corners, nrm, subdiv)
            vs.append(v)
            ns.append(n)
    return np.concatenate(vs), np.concatenate(ns)


def icosphere_mesh(center, radius: float, level: int = 0):
    """(vertices, normals) of a sphere obstacle: the icosahedron, every triangle split in four `level` times and the new
    vertices pushed out to the sphere -- 20 * 4^level triangles (20,480 at level 5), none of them thin (a latitude /
    longitude sphere ends in needles at its poles, which a collider's broad phase cannot skip).  The normals are the unit
    outward face normals, computed in float64 from the float32 vertices."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
                  (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)], dtype=np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    faces = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2),
                      (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11),
                      (6, 2, 10), (8, 6, 7), (9, 8, 1)], dtype=np.int64)
    tri = v[faces]  # (20, 3, 3), counter-clockwise seen from outside
    for _ in range(int(level)):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = a + b, b + c, c + a
        ab, bc, ca = (m / np.linalg.norm(m, axis=1, keepdims=True) for m in (ab, bc, ca))
        tri = np.stack([np.stack(q, axis=1) for q in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))], axis=1).reshape(-1, 3, 3)
    verts = (np.asarray(center, dtype=np.float64)[None, None, :] + float(radius) * tri).astype(f32)
    q = verts.astype(np.float64)
    n = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    outward = np.sum(n * (q.mean(axis=1) - np.asarray(center, dtype=np.float64)[None, :]), axis=1) > 0
    assert outward.all()
    return verts, n.astype(f32)
