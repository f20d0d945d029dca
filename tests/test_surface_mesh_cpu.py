"""The indexed fluid surface, the parts that need no GPU: the numpy reference of dsl_surface_extract_indexed's rule
(tests/surface_mesh_ref.py) against the soup's reference and against itself -- the vertex set is the set of edges the soup's
triangles touch, positions[index] is the soup bit for bit, ids keep a tie at iso a manifold, vertex normals point the way
the face normals do -- and the library exports the entry points."""
import functools

import numpy as np

import surface_mesh_ref as mref
import surface_ref as ref


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_volume(dims, seed, nan=0.03, tie=0.05, iso=0.25):
    """values around iso, about 3 % of the voxels NaN and 5 % exactly iso: shape (nz, ny, nx)"""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    v = rng.normal(iso, 1.0, (nz, ny, nx)).astype(np.float32)
    r = rng.random((nz, ny, nx))
    v[r < nan] = np.nan
    v[(r >= nan) & (r < nan + tie)] = np.float32(iso)
    return v


ORIGIN, STEP, ISO = (-0.4, 0.3, 0.05), (0.11, 0.07, 0.13), 0.25


def test_the_vertex_set_is_the_set_of_edges_the_soups_triangles_touch():
    for seed, dims in enumerate([(9, 7, 6), (10, 9, 5), (17, 9, 6), (2, 2, 2), (18, 17, 10), (3, 3, 9), (1, 5, 5), (2, 9, 2)]):
        for nan, tie in ((0.03, 0.05), (0.0, 0.0), (0.2, 0.2)):
            vol = random_volume(dims, seed, nan, tie, ISO)
            got, want = mref.vertex_edge_set(vol, dims, ISO), mref.soup_edge_set(vol, dims, ISO)
            assert np.array_equal(got, want), (dims, nan, tie)
    # every mask of one cube, with and without a tie
    for mask in range(256):
        for inside_value in (1.0, 0.0):
            vol = np.array([inside_value if (mask >> c) & 1 else -1.0 for c in range(8)], dtype=np.float32)
            assert np.array_equal(mref.vertex_edge_set(vol, (2, 2, 2), 0.0), mref.soup_edge_set(vol, (2, 2, 2), 0.0)), mask


def test_positions_through_the_indices_are_the_soup_bit_for_bit():
    for seed, dims in enumerate([(18, 17, 10), (9, 7, 6), (2, 2, 2)]):
        vol = random_volume(dims, 10 + seed, iso=ISO)
        pos, nrm, idx = mref.mesh(vol, ORIGIN, STEP, dims, ISO)
        soup, _ = ref.extract(vol.ravel(), ORIGIN, STEP, dims, ISO)
        assert idx.shape == (soup.shape[0], 3) and pos.shape == nrm.shape
        assert np.array_equal(_bits(pos[idx]), _bits(soup))
        assert np.array_equal(np.unique(idx), np.arange(pos.shape[0]))  # every vertex is referenced
        assert np.isfinite(pos).all() and np.isfinite(nrm).all()


def test_the_vertex_order_is_bricks_of_voxels_then_voxels_then_d():
    dims = (18, 17, 10)
    vol = random_volume(dims, 3, iso=ISO)
    u, d = mref.vertex_order(mref.vertex_edges(vol, dims, ISO), dims)
    i, j, k = u % 18, (u // 18) % 17, u // (18 * 17)
    brick = ((k // 4) * 3 + j // 8) * 3 + i // 8  # 3 x 3 x 3 bricks of voxels (the bricks of cubes: 3 x 2 x 3)
    assert np.all(np.diff(brick) >= 0) and brick.max() > 2 * 9 + 2 * 3  # (a vertex in the third layer of voxel bricks: z = 8, 9)
    lane = ((k % 4) * 8 + j % 8) * 8 + i % 8
    key = (brick * 256 + lane) * 8 + d
    assert np.all(np.diff(key) > 0)


# ---- a sphere with voxels exactly at iso -------------------------------------------------------------------------------
S_ORIGIN, S_STEP, S_DIMS, S_ISO = (-1.13, -0.97, -1.05), (0.19, 0.21, 0.2), (13, 11, 12), 0.2
S_CENTRE = (0.03, 0.05, -0.02)
AT_ISO = [(3, 4, 3), (4, 8, 5), (6, 7, 9), (7, 2, 8), (8, 5, 9)]  # inside voxels with an outside neighbour, as (k, j, i)


@functools.lru_cache(maxsize=None)
def _sphere(ties=True):
    o, s = np.asarray(S_ORIGIN, np.float32), np.asarray(S_STEP, np.float32)
    x, y, z = (o[a] + s[a] * np.arange(S_DIMS[a], dtype=np.float32) for a in range(3))
    Z, Y, X = np.meshgrid(z.astype(np.float64), y.astype(np.float64), x.astype(np.float64), indexing="ij")
    v = (1.0 - np.sqrt((X - S_CENTRE[0]) ** 2 + (Y - S_CENTRE[1]) ** 2 + (Z - S_CENTRE[2]) ** 2)).astype(np.float32)
    if ties:
        for q in AT_ISO:
            assert v[q] >= np.float32(S_ISO)
            v[q] = np.float32(S_ISO)
    v.setflags(write=False)
    return v


def test_a_sphere_with_ties_welded_by_id_is_closed_with_euler_characteristic_two():
    vol = _sphere()
    pos, nrm, idx = mref.mesh(vol, S_ORIGIN, S_STEP, S_DIMS, S_ISO)
    soup, _ = ref.extract(vol.ravel(), S_ORIGIN, S_STEP, S_DIMS, S_ISO)
    assert ref.degenerate(soup).sum() > 0  # the ties make zero-area triangles; they stay in
    closed, E = mref.closed_by_id(idx)
    V, F = pos.shape[0], idx.shape[0]
    print("sphere with ties: V, E, F =", V, E, F)
    assert closed and V - E + F == 2
    # distinct vertices share their position bits at a tie: welding by bits would merge them
    assert np.unique(_bits(pos), axis=0).shape[0] < V
    # ... and welded by bits WITH the zero-area triangles the surface is no manifold
    _u, inv = np.unique(_bits(soup.reshape(-1, 3)), axis=0, return_inverse=True)
    assert not mref.closed_by_id(inv.reshape(-1, 3))[0]


def test_vertex_normals_point_outwards_and_along_the_face_normals():
    low = []
    for ties in (False, True):
        vol = _sphere(ties)
        pos, nrm, idx = mref.mesh(vol, S_ORIGIN, S_STEP, S_DIMS, S_ISO)
        soup, face = ref.extract(vol.ravel(), S_ORIGIN, S_STEP, S_DIMS, S_ISO)
        n64 = nrm.astype(np.float64)
        assert np.allclose(np.linalg.norm(n64, axis=1), 1.0, atol=1e-6)
        radial = pos.astype(np.float64) - np.asarray(S_CENTRE)
        radial /= np.linalg.norm(radial, axis=1)[:, None]
        d_radial = np.einsum("ij,ij->i", n64, radial)
        keep = ~ref.degenerate(soup)
        d_face = np.einsum("tej,tj->te", n64[idx[keep]], face[keep].astype(np.float64))
        print("sphere, ties" if ties else "sphere", "smallest n . radial", d_radial.min(), "smallest n . face normal", d_face.min())
        assert d_radial.min() > 0 and d_face.min() > 0
        low.append((d_radial.min(), d_face.min()))


def test_one_sided_gradients_at_the_lattice_faces_and_next_to_nan():
    """a linear volume has the same gradient everywhere, one-sided or central: the normal is its direction at every vertex"""
    dims = (6, 5, 5)  # (the NaN voxel's six neighbours each keep one usable neighbour of their own along that axis)
    k, j, i = np.meshgrid(np.arange(5), np.arange(5), np.arange(6), indexing="ij")
    vol = (0.5 * i - 0.25 * j + 0.125 * k - 0.8125).astype(np.float32)  # (multiples of 1/16: every difference is exact)
    vol[2, 2, 3] = np.nan
    g = mref.gradient(vol, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims)
    fin = np.isfinite(vol)
    assert np.all(g[0][fin] == 0.5) and np.all(g[1][fin] == -0.25) and np.all(g[2][fin] == 0.125)
    pos, nrm, idx = mref.mesh(vol, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dims, 0.0)
    want = -np.array([0.5, -0.25, 0.125]) / np.linalg.norm([0.5, -0.25, 0.125])
    assert pos.shape[0] > 10 and np.allclose(nrm, want[None, :], atol=1e-6)
    lone = np.full((3, 3, 3), np.nan, dtype=np.float32)
    lone[1, 1, 1] = 1.0
    assert not mref.gradient(lone, (0.0,) * 3, (1.0,) * 3, (3, 3, 3))[:, 1, 1, 1].any()  # neither neighbour usable: 0


def test_the_library_exports_the_entry_points():
    import ctypes as C
    from dieselfluid_amd import _lib
    _lib.build_library()
    L = C.CDLL(_lib.library_path())
    assert hasattr(L, "dsl_surface_extract_indexed") and len(_lib.EXPORTS["dsl_surface_extract_indexed"][1]) == 13
    assert hasattr(L, "dsl_field_surface_indexed") and len(_lib.EXPORTS["dsl_field_surface_indexed"][1]) == 12
