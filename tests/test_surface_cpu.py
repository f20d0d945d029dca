"""Fluid surfaces, the parts that need no GPU: the committed table (csrc/surface_table.hpp) is what its generator makes and
agrees with the windings tests/surface_ref.py derives on its own; and the rule itself, run through the numpy reference,
gives a closed, consistently wound surface on a sphere -- with voxels exactly at iso, and with a NaN voxel, as stated."""
import functools
import os
import re
import sys

import numpy as np

import surface_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HEADER = os.path.join(ROOT, "dieselfluid_amd", "csrc", "surface_table.hpp")


def _header_array(name):
    text = open(HEADER).read()
    m = re.search(r"constexpr unsigned char %s((?:\[\d+\])+) = \{(.*?)\};" % name, text, re.S)
    assert m, name
    shape = [int(d) for d in re.findall(r"\[(\d+)\]", m.group(1))]
    return np.array([int(v) for v in re.findall(r"\d+", m.group(2))], dtype=np.int64).reshape(shape)


# ---- the table ---------------------------------------------------------------------------------------------------------
def test_the_committed_table_is_the_generators_output():
    import make_surface_table
    assert open(HEADER).read() == make_surface_table.render()


def test_the_cube_counts_are_the_per_mask_sums_and_never_exceed_twelve():
    corner, ntri, count = _header_array("kSurfTetCorner"), _header_array("kSurfTetTriangles"), _header_array("kSurfCubeTriangles")
    assert corner.shape == (6, 4) and ntri.shape == (6, 16) and count.shape == (256,)
    assert [tuple(t) for t in corner] == ref.TETS
    for cube in range(256):
        total = 0
        for t in range(6):
            m4 = sum(((cube >> int(corner[t][m])) & 1) << m for m in range(4))
            total += int(ntri[t][m4])
        assert count[cube] == total, cube
    assert count.max() == 12 and count[0] == 0 and count[255] == 0
    assert np.array_equal(count, count[::-1])  # (inside and outside exchanged: the same triangles, turned round)


def test_the_tables_winding_is_the_one_geometry_gives():
    """surface_ref derives every case from the gradient of the tetrahedron's affine interpolant; the generator from the
    centroids of the inside and the outside vertices, in rational arithmetic.  Same triangles, same order, same winding."""
    ntri, edge = _header_array("kSurfTetTriangles"), _header_array("kSurfTetEdge")
    assert edge.shape == (6, 16, 6)
    for t in range(6):
        for m in range(16):
            case = ref.CASES[t][m]
            assert len(case) == ntri[t][m]
            want = [u | (w << 3) for tri in case for (u, w) in tri]
            assert list(edge[t][m][:len(want)]) == want and not edge[t][m][len(want):].any(), (t, m)


# ---- the rule on a sphere ----------------------------------------------------------------------------------------------
ORIGIN, STEP, DIMS, ISO = (-1.13, -0.97, -1.05), (0.19, 0.21, 0.2), (13, 11, 12), 0.2
CENTRE = (0.03, 0.05, -0.02)


@functools.lru_cache(maxsize=None)
def _sphere():
    """1 - |x - c| on the lattice (the coordinates are the product's float32 ones), shape (nz, ny, nx)"""
    o, s = np.asarray(ORIGIN, np.float32), np.asarray(STEP, np.float32)
    x, y, z = (o[a] + s[a] * np.arange(DIMS[a], dtype=np.float32) for a in range(3))
    Z, Y, X = np.meshgrid(z.astype(np.float64), y.astype(np.float64), x.astype(np.float64), indexing="ij")
    v = (1.0 - np.sqrt((X - CENTRE[0]) ** 2 + (Y - CENTRE[1]) ** 2 + (Z - CENTRE[2]) ** 2)).astype(np.float32)
    v.setflags(write=False)
    return v


def test_a_sphere_gives_a_closed_consistently_wound_surface():
    verts, norms = ref.extract(_sphere().ravel(), ORIGIN, STEP, DIMS, ISO)
    assert verts.shape == (1788, 3, 3) and norms.shape == (1788, 3)
    assert not ref.degenerate(verts).any()
    V, E, F, closed, volume = ref.topology(verts)
    print("sphere: V, E, F =", V, E, F, "closed:", closed, "volume:", volume)
    assert closed          # every undirected edge twice, once in each direction, welding by vertex bits
    assert V - E + F == 2
    assert volume > 0      # outward normals; 2.078 against the analytic 4/3 pi 0.8^3 = 2.145 (the chords cut it short)
    assert abs(volume - 2.078) < 1e-3
    # the stored normals are the triangles' own, unit length, pointing away from the centre
    centroid = verts.astype(np.float64).mean(axis=1)
    assert np.all(np.einsum("ij,ij->i", norms.astype(np.float64), centroid - np.asarray(CENTRE)) > 0)
    assert np.allclose(np.linalg.norm(norms.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # the order: bricks of 8 x 8 x 4 cubes ascending, cubes ascending inside a brick -- every triangle lies in its cube
    start, counts = ref.cube_starts(_sphere().ravel(), DIMS, ISO)
    assert counts.sum() == 1788 and counts.max() <= 12
    o, s = np.asarray(ORIGIN, np.float64), np.asarray(STEP, np.float64)
    order = ref.emit_order(DIMS)
    assert order[:8].tolist() == list(range(8)) and order[8] == DIMS[0] - 1 and order[256] == 8  # (12 x 10 x 11 cubes: 2 x 2 x 3 bricks)
    for cube in np.nonzero(counts)[0]:
        idx = np.array([cube % 12, (cube // 12) % 10, cube // 120])
        tri = verts[start[cube]:start[cube] + counts[cube]].astype(np.float64)
        assert np.all(tri >= o + s * idx - 1e-6) and np.all(tri <= o + s * (idx + 1) + 1e-6), cube


# five inside voxels with an outside neighbour across a face, as (k, j, i)
AT_ISO = [(3, 4, 3), (4, 8, 5), (6, 7, 9), (7, 2, 8), (8, 5, 9)]


def _collapsed_triangles(volume, iso):
    """Triangles that the rule makes degenerate, from the masks alone: an edge point lies ON its inside voxel when that
    voxel's value is iso (t is 0 or 1 there), so a triangle with two edge points on edges out of the same such voxel has
    two equal vertices."""
    mask, corner = ref.cube_masks(volume.ravel(), DIMS, iso)
    m4 = ref.tet_masks(mask)
    n = 0
    for cube in np.nonzero(mask)[0]:
        for t in range(6):
            for tri in ref.CASES[t][m4[cube, t]]:
                ends = []
                for u, w in tri:
                    inside = u if (mask[cube] >> u) & 1 else w
                    ends.append(inside if corner[cube, inside] == np.float32(iso) else -1 - len(ends))
                n += len(set(ends)) < 3
    return n


def test_voxels_exactly_at_iso_give_zero_area_triangles_that_are_kept():
    v = _sphere().copy()
    iso = np.float32(ISO)
    for q in AT_ISO:
        assert v[q] >= iso and min(v[q[0], q[1], q[2] - 1], v[q[0], q[1], q[2] + 1], v[q[0], q[1] - 1, q[2]], v[q[0], q[1] + 1, q[2]],
                                   v[q[0] - 1, q[1], q[2]], v[q[0] + 1, q[1], q[2]]) < iso
        v[q] = iso
    verts, _norms = ref.extract(v.ravel(), ORIGIN, STEP, DIMS, ISO)
    # still inside (>=): the masks, and with them the count, are the sphere's
    assert verts.shape[0] == 1788
    deg = int(ref.degenerate(verts).sum())
    print("five voxels at iso: zero-area triangles:", deg)
    assert deg == _collapsed_triangles(v, ISO) == 64  # (which five voxels decides the number: 28 to 66 over 400 random choices on this sphere)
    V, E, F, closed, volume = ref.topology(verts)  # (without the zero-area triangles)
    assert F == 1788 - deg and closed and V - E + F == 2 and volume > 0
    _v, norms = ref.extract(v.ravel(), ORIGIN, STEP, DIMS, ISO)
    assert np.all(norms[ref.degenerate(verts)] == 0)


def test_a_nan_voxel_opens_a_hole_of_exactly_the_cubes_that_touch_it():
    v = _sphere().copy()
    k, j, i = 6, 5, 2  # on the surface: its cubes emit triangles
    v[k, j, i] = np.nan
    base = ref.cube_counts(_sphere().ravel(), DIMS, ISO).reshape(DIMS[2] - 1, DIMS[1] - 1, DIMS[0] - 1)
    got = ref.cube_counts(v.ravel(), DIMS, ISO).reshape(base.shape)
    touch = np.zeros(base.shape, dtype=bool)
    touch[k - 1:k + 1, j - 1:j + 1, i - 1:i + 1] = True
    assert touch.sum() == 8 and base[touch].sum() > 0
    assert np.all(got[touch] == 0) and np.array_equal(got[~touch], base[~touch])
    verts, _ = ref.extract(v.ravel(), ORIGIN, STEP, DIMS, ISO)
    assert verts.shape[0] == 1788 - base[touch].sum() and np.isfinite(verts).all()
    _V, _E, _F, closed, _vol = ref.topology(verts)
    assert not closed  # the hole has a rim
    # the triangles of the other cubes are the sphere's own, bit for bit and in order
    full, _ = ref.extract(_sphere().ravel(), ORIGIN, STEP, DIMS, ISO)
    start, _counts = ref.cube_starts(_sphere().ravel(), DIMS, ISO)
    keep = np.ones(1788, dtype=bool)
    for c in np.nonzero(touch.ravel())[0]:
        keep[start[c]:start[c] + base.ravel()[c]] = False
    assert np.array_equal(verts.view(np.uint32), full[keep].view(np.uint32))


def test_the_library_exports_the_entry_points():
    import ctypes as C
    from dieselfluid_amd import _lib
    _lib.build_library()
    L = C.CDLL(_lib.library_path())
    assert hasattr(L, "dsl_surface_extract") and len(_lib.EXPORTS["dsl_surface_extract"][1]) == 11
    assert hasattr(L, "dsl_field_surface") and len(_lib.EXPORTS["dsl_field_surface"][1]) == 10
