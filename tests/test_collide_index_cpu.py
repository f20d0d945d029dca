"""The collider's cell index, what can be checked without a GPU: the new DSL_OPT_* values of include/dslsph.h are the
ones engine.OPTIONS and the Go binding name; scenes.icosphere_mesh gives 20 * 4^level triangles, every one of them
REGULAR under k_collide_prep's float32 formula (csrc/kernels_collide.hpp), restated here in numpy -- so the whole sphere
goes into the cell lists and nothing onto the always-list."""
import os
import re

import numpy as np
import pytest

import collider_ref as cr

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"collide_index": ("DSL_OPT_COLLIDE_INDEX", "OptCollideIndex", 35),
       "collide_index_edge": ("DSL_OPT_COLLIDE_INDEX_EDGE", "OptCollideIndexEdge", 36),
       "collide_index_cells": ("DSL_OPT_COLLIDE_INDEX_CELLS", "OptCollideIndexCells", 37),
       "collide_index_entries": ("DSL_OPT_COLLIDE_INDEX_ENTRIES", "OptCollideIndexEntries", 38),
       "collide_visits": ("DSL_OPT_COLLIDE_VISITS", "OptCollideVisits", 39),
       "collide_full_waves": ("DSL_OPT_COLLIDE_FULL_WAVES", "OptCollideFullWaves", 40)}


def test_header_engine_and_go_binding_agree_on_the_new_options():
    from dieselfluid_amd.engine import SPHEngine
    header = open(os.path.join(ROOT, "include", "dslsph.h")).read()
    go = open(os.path.join(ROOT, "bindings", "go", "dslsph", "dslsph.go")).read()
    in_header = {k: int(v) for k, v in re.findall(r"\b(DSL_OPT_\w+)\s*=\s*(\d+)", header)}
    assert len(set(in_header.values())) == len(in_header)  # no value twice
    for name, (c_name, go_name, value) in NEW.items():
        assert in_header[c_name] == value and SPHEngine.OPTIONS[name] == value, name
        assert re.search(rf"\b{go_name}\s*=\s*int\(C\.{c_name}\)", go), go_name
    # ... and on every other one: each name of the engine's table is a value of the header
    assert set(SPHEngine.OPTIONS.values()) <= set(in_header.values())


def regular(verts, normals, r):
    """k_collide_prep's `regular` flag and padded box, float32, operation for operation"""
    a, e0, e1, d00, d01, d11, denom = cr.triangle_terms(verts)
    v = np.asarray(verts, dtype=f32).reshape(-1, 3, 3)
    n = np.asarray(normals, dtype=f32).reshape(-1, 3)
    lo, hi = v.min(axis=1), v.max(axis=1)
    ext = np.zeros(v.shape[0], dtype=f32)
    big = np.zeros(v.shape[0], dtype=f32)
    for k in range(3):
        ext = ext + (hi[:, k] - lo[:, k])
        big = np.maximum(big, np.maximum(np.abs(lo[:, k]), np.abs(hi[:, k])))
    pad = f32(2.1) * f32(r) + f32(0.01) * ext + f32(1.0e-5) * big
    p0 = d00 * d11
    n2, ne0, ne1 = cr._dot(n, n), cr._dot(n, e0), cr._dot(n, e1)
    reg = (n2 >= f32(0.25)) & (n2 <= f32(1.002001))
    reg &= (d00 > 0) & (d11 > 0) & (denom >= f32(0.01) * p0) & (p0 < f32(1.0e30))
    reg &= (ne0 * ne0 <= f32(1.0e-6) * (n2 * d00)) & (ne1 * ne1 <= f32(1.0e-6) * (n2 * d11))
    reg &= (pad >= 0) & (pad < f32(1.0e30)) & (big < f32(1.0e30))
    return reg, lo - pad[:, None], hi + pad[:, None]


@pytest.mark.parametrize("level", [0, 1, 2, 3, 5])
def test_icosphere_has_20_times_4_to_the_level_regular_triangles(level):
    from dieselfluid_amd import scenes
    verts, normals = scenes.icosphere_mesh((0.05, -0.1, 0.0), 0.7, level)
    assert verts.shape == (20 * 4 ** level, 3, 3) and normals.shape == (20 * 4 ** level, 3)
    assert verts.dtype == f32 and normals.dtype == f32
    reg, _lo, _hi = regular(verts, normals, 0.1)
    assert reg.all()
    # unit outward face normals; the vertices lie on the sphere
    q = verts.astype(np.float64)
    c = np.array([0.05, -0.1, 0.0])
    assert np.allclose(np.linalg.norm(q - c, axis=2), 0.7, atol=1e-6)
    assert np.allclose(np.linalg.norm(normals.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert np.all(np.sum(normals * (q.mean(axis=1) - c), axis=1) > 0)
    # no thin triangle: every angle is far above the 5.7 degrees at which a triangle stops being regular
    e0, e1 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
    sin2 = 1 - np.sum(e0 * e1, axis=1) ** 2 / (np.sum(e0 * e0, axis=1) * np.sum(e1 * e1, axis=1))
    assert sin2.min() > 0.5


def test_the_irregular_kinds_of_the_collider_tests_are_not_regular():
    """the formula above is not vacuous: test_gpu_collider's _mesh(300) edits come out irregular, the rest regular"""
    from dieselfluid_amd import scenes
    v, n = scenes.box_mesh((0.05, -0.1, 0.0), (1.3, 1.1, 1.2), 5)
    v, n = v.copy(), n.copy()
    v[150, 1] = v[150, 0]
    n[200:210] *= f32(3.0)
    n[210:220] = n[210:220][:, [1, 2, 0]]
    n[299] = 0
    reg, _lo, _hi = regular(v, n, 0.15)
    want = np.ones(300, dtype=bool)
    want[150] = want[299] = False
    want[200:220] = False
    assert np.array_equal(reg, want)
