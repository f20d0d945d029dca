"""Implicit colliders, the parts that need no GPU: tests/sdf_ref.py -- the numpy float32 restatement of the two build-defined
rules of csrc/sdf.hip (include/dslsph.h) -- against float64: the distance by the same seven regions in float64,
the sign against an inside test that shares nothing with the rule (coordinates for the box, the solid angle for the
spheres), the collider rule on a plane, which the trilinear form reproduces; and the new names in the header, the ctypes
table, the engine's option table and the Go binding."""
import os
import re

import numpy as np
import pytest

import sdf_cases as sc
import sdf_ref

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTENT = 1.7  # the lattice's largest extent (sdf_cases.DIMS at step 0.1)
# |float32 - float64| of the distance, measured by test_distance_against_float64 on its six cases: at most 8.3e-8 of the
# extent (triangle 6.9e-8, box 3.9e-8, ico0 7.0e-8, ico1 7.1e-8, ico2 8.2e-8, degenerate 7.0e-8).  Four times that.
DIST_TOL = 4 * 8.3e-8


def _distance64(name, dims=sc.DIMS, x0=0.0):
    p = sc.points64(dims, x0).reshape(-1, 3)
    best = np.full(p.shape[0], np.inf)
    for tri in sc.mesh(name).astype(np.float64):
        d2 = sdf_ref.tri_dist2(p[:, 0], p[:, 1], p[:, 2], tri, dtype=np.float64)
        best = np.where(d2 < best, d2, best)
    return np.sqrt(best).reshape(dims[2], dims[1], dims[0])


def _inside_by_solid_angle(name):
    """float64: the triangles' signed solid angles (Van Oosterom and Strackee) sum to +-4 pi inside, 0 outside"""
    p = sc.points64().reshape(-1, 3)
    total = np.zeros(p.shape[0])
    for tri in sc.mesh(name).astype(np.float64):
        a, b, c = tri[0] - p, tri[1] - p, tri[2] - p
        la, lb, lc = (np.linalg.norm(v, axis=1) for v in (a, b, c))
        num = np.einsum("ij,ij->i", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("ij,ij->i", a, b) * lc + np.einsum("ij,ij->i", b, c) * la + np.einsum("ij,ij->i", c, a) * lb
        total += 2 * np.arctan2(num, den)
    return (np.abs(total) > 2 * np.pi).reshape(sc.DIMS[2], sc.DIMS[1], sc.DIMS[0])


def test_one_triangle_has_voxels_in_all_seven_regions():
    a, b, c = sc.mesh("triangle")[0].astype(np.float64)
    p = sc.points64().reshape(-1, 3)
    ab, ac = b - a, c - a
    d1, d2 = (p - a) @ ab, (p - a) @ ac
    d3, d4 = (p - b) @ ab, (p - b) @ ac
    d5, d6 = (p - c) @ ab, (p - c) @ ac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6), (vc <= 0) & (d1 >= 0) & (d3 <= 0),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    region = np.select(conds, list(range(6)), 6)
    assert sorted(set(region.tolist())) == list(range(7))


@pytest.mark.parametrize("name", ["triangle", "box", "ico0", "ico1", "ico2", "degenerate"])
def test_distance_against_float64(name):
    d, want = sc.distance(name), _distance64(name)
    assert d.dtype == f32 and np.isfinite(d).all()
    err = float(np.abs(d.astype(np.float64) - want).max()) / EXTENT
    print(f"{name}: |float32 - float64| / extent = {err:.2e}")
    assert err <= DIST_TOL
    if name == "degenerate":
        # the zero-area triangle and the repeated vertex change nothing the sphere has not decided ... except where one of
        # their points is the closest: both are real points of the mesh
        assert np.all(d <= sc.distance("ico0")) and np.any(d < sc.distance("ico0"))


@pytest.mark.parametrize("x0", [0.0, 0.03])
def test_sign_of_the_lattice_aligned_box(x0):
    """x0 = 0: rays run through edges and vertices of the subdivided faces, and the four faces along x project to nothing"""
    p = sc.points64(x0=x0)
    v = sc.mesh("box").astype(np.float64).reshape(-1, 3)
    want = np.all((p > v.min(axis=0)) & (p < v.max(axis=0)), axis=-1)
    keep = _distance64("box", x0=x0) >= 1e-6 * EXTENT
    left_out = int((~keep).sum())
    print(f"x0 = {x0}: {left_out} of {keep.size} voxels lie on the surface")  # 306 and 240 of 3060
    assert left_out <= 0.10 * keep.size
    got = sc.inside("box", x0=x0)
    assert want[keep].sum() >= 100 and np.array_equal(got[keep], want[keep])


@pytest.mark.parametrize("level", [0, 1, 2])
def test_sign_of_the_icospheres(level):
    name = f"ico{level}"
    want = _inside_by_solid_angle(name)
    keep = _distance64(name) >= 1e-6 * EXTENT
    assert int((~keep).sum()) <= 0.10 * keep.size  # (none)
    got = sc.inside(name)
    assert want[keep].sum() >= 100 and np.array_equal(got[keep], want[keep])


def test_the_degenerate_triangles_are_skipped_by_the_sign():
    assert np.array_equal(sc.inside("degenerate"), sc.inside("ico0"))


def test_an_open_quad_unsigned_is_the_closed_box_where_the_quad_is_nearest():
    quad = sdf_ref.volume(sc.mesh("quad"), sc.origin(), sc.STEP, sc.DIMS, flags=sdf_ref.UNSIGNED)
    rest = sc.distance("rest")
    box = sc.volume("box")
    both = quad <= rest  # the nearest point of the box lies on the quad: both volumes measure the same distance
    assert 100 <= both.sum() < both.size
    assert np.array_equal(np.abs(box)[both].view(np.uint32), quad[both].view(np.uint32))
    assert np.all(quad >= 0) and np.any(box < 0)
    # the open quad, signed: whatever the parity gives, without error -- the voxels below it, inside its footprint
    signed = sdf_ref.volume(sc.mesh("quad"), sc.origin(), sc.STEP, sc.DIMS)
    assert np.array_equal(np.abs(signed).view(np.uint32), quad.view(np.uint32))


@pytest.mark.parametrize("name,band", [("box", 0.3), ("ico1", 0.05), ("ico1", 0.3)])
def test_a_finite_band_cuts_the_full_volume_off(name, band):
    full = sc.volume(name)
    got = sdf_ref.volume(sc.mesh(name), sc.origin(), sc.STEP, sc.DIMS, band=band)
    want = np.where(full < 0, -np.minimum(-full, f32(band)), np.minimum(full, f32(band))).astype(f32)
    neg_zero = sc.inside(name) & (sc.distance(name) == 0)  # (-0.0 < 0 is false: its sign comes from the parity)
    want = np.where(neg_zero, -f32(0), want).astype(f32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.any(np.abs(got) == f32(band)) and np.any(np.abs(got) < f32(band))


# ---- the collider rule on a plane ----
PLANE_N = np.array([0.36, 0.48, 0.8])  # unit
PLANE_C = 0.9
VORIGIN, VSTEP, VDIMS = (-0.2, -0.1, 0.0), (0.1, 0.125, 0.15), (12, 11, 9)
RADIUS = 0.07
# |n.x' - c - radius| after the response, measured here against float64: 1.73e-7 with coordinates up to 1.2 (the float32
# volume, the interpolation, the normalisation and the push each round).  Four times that.
PLANE_TOL = 4 * 1.8e-7


def _plane_volume():
    x, y, z = (a.astype(np.float64) for a in sdf_ref.axes(VORIGIN, VSTEP, VDIMS))
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return (PLANE_N[0] * xx + PLANE_N[1] * yy + PLANE_N[2] * zz - PLANE_C).astype(f32)


def _cloud(n=4000, seed=5):
    rng = np.random.default_rng(seed)
    lo = np.array(VORIGIN) - 0.05
    hi = np.array(VORIGIN) + np.array(VSTEP) * (np.array(VDIMS) - 1) + 0.05
    pos = rng.uniform(lo, hi, (n, 3)).astype(f32)
    vel = rng.uniform(-1, 1, (n, 3)).astype(f32)
    return pos, vel


def test_collider_rule_on_a_plane():
    vol = _plane_volume()
    pos, vel = _cloud()
    cell, d, g, mag = sdf_ref.collider_eval(vol, VORIGIN, VSTEP, pos)
    d64 = pos.astype(np.float64) @ PLANE_N - PLANE_C
    assert 0.5 < cell.mean() < 1.0  # (some of the cloud lies outside the lattice)
    assert np.abs(d[cell] - d64[cell]).max() < 1e-6 and np.abs(g[cell] - PLANE_N).max() < 1e-5
    for rest in (0.0, 0.5):
        x1, v1, hit = sdf_ref.collider_pass(vol, VORIGIN, VSTEP, pos, vel, RADIUS, rest)
        assert np.array_equal(hit, cell & (d < f32(RADIUS))) and 100 < hit.sum() < cell.sum()
        after = x1.astype(np.float64) @ PLANE_N - PLANE_C
        err = float(np.abs(after[hit] - RADIUS).max())
        print(f"restitution {rest}: |distance after the response - radius| = {err:.2e}")
        assert err <= PLANE_TOL
        # v' is the reflection formula where the particle approaches, v where it recedes
        n = (g / mag[:, None]).astype(np.float64)
        vn = np.einsum("ij,ij->i", vel.astype(np.float64), n)
        want = vel.astype(np.float64) - ((1 + rest) * vn)[:, None] * n
        approaching = hit & (vn < -1e-6)
        receding = hit & (vn > 1e-6)
        assert approaching.sum() > 20 and receding.sum() > 20
        assert np.abs(v1[approaching] - want[approaching]).max() < 1e-6
        assert np.array_equal(v1[receding].view(np.uint32), vel[receding].view(np.uint32))
        # nobody else moves
        assert np.array_equal(x1[~hit].view(np.uint32), pos[~hit].view(np.uint32))
        assert np.array_equal(v1[~hit].view(np.uint32), vel[~hit].view(np.uint32))


def test_collider_rule_at_the_edges_of_the_lattice():
    vol = np.full((4, 4, 4), -1.0, dtype=f32)  # everything is deep inside ...
    vol[:, :, 2:] = f32(-0.5)                  # ... with a gradient along x between i = 1 and 2 only
    o, s = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    pos = np.array([[1.5, 1.5, 1.5],    # a cell with a gradient: collides
                    [2.5, 2.5, 2.5],    # the last cell (index n - 2), |g| = 0: no collision
                    [0.5, 0.5, 0.5],    # |g| = 0
                    [3.0, 1.5, 1.5],    # index n - 1: one outside
                    [3.5, 1.5, 1.5], [-0.5, 1.5, 1.5], [1.5, 1.5, np.nan], [np.inf, 1.5, 1.5],
                    [1.5, 2.5, 2.999]], dtype=f32)  # the last cell along y and z, with the gradient: collides
    vel = np.zeros_like(pos)
    x1, _v1, hit = sdf_ref.collider_pass(vol, o, s, pos, vel, 0.0, 0.0)
    assert hit.tolist() == [True, False, False, False, False, False, False, False, True]
    assert x1[0].tolist() == [2.25, 1.5, 1.5]  # d = -0.75, n = +x: out by 0.75
    dist, nrm = sdf_ref.collider_query(vol, o, s, pos)
    assert dist.tolist() == [-0.75, -0.5, -1.0, 0, 0, 0, 0, 0, -0.75] and nrm[1].tolist() == [0, 0, 0] and nrm[0].tolist() == [1, 0, 0]
    vol2 = vol.copy()
    vol2[1, 1, 1] = np.nan  # a corner of the first particle's cell, not of the last one's
    _x, _v, hit2 = sdf_ref.collider_pass(vol2, o, s, pos, vel, 0.0, 0.0)
    assert hit2.tolist() == [False] * 8 + [True]


# ---- names ----
NEW_OPTIONS = {"sdf_active_bricks": ("DSL_OPT_SDF_ACTIVE_BRICKS", "OptSdfActiveBricks", 72),
               "sdf_visits": ("DSL_OPT_SDF_VISITS", "OptSdfVisits", 73),
               "sdf_distance_ms": ("DSL_OPT_SDF_DISTANCE_MS", "OptSdfDistanceMs", 74),
               "sdf_sign_ms": ("DSL_OPT_SDF_SIGN_MS", "OptSdfSignMs", 75),
               "collider_volume": ("DSL_OPT_COLLIDER_VOLUME", "OptColliderVolume", 76)}


def test_header_engine_and_go_binding_agree_on_the_new_names():
    from dieselfluid_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "dslsph.h")).read()
    go = open(os.path.join(ROOT, "bindings", "go", "dslsph", "dslsph.go")).read()
    in_header = {k: int(v) for k, v in re.findall(r"\b(DSL_OPT_\w+)\s*=\s*(\d+)", header)}
    for name, (c_name, go_name, value) in NEW_OPTIONS.items():
        assert in_header[c_name] == value and engine.SPHEngine.OPTIONS[name] == value, name
        assert re.search(rf"\b{go_name}\s*=\s*int\(C\.{c_name}\)", go), go_name
    assert re.search(r"\bDSL_K_SDF\s*=\s*18\b", header) and re.search(r"\bDSL_K_COUNT\s*=\s*19\b", header)
    assert engine.KERNEL_IDS["sdf"] == 18 and re.search(r"\bKSdf\s*=\s*int\(C\.DSL_K_SDF\)", go)
    assert re.search(r"#define\s+DSL_SDF_UNSIGNED\s+1\b", header) and engine.SDF_UNSIGNED == sdf_ref.UNSIGNED == 1
    assert re.search(r"\bSdfUnsigned\s*=\s*int\(C\.DSL_SDF_UNSIGNED\)", go)
    for name, arity in (("dsl_mesh_distance_volume", 10), ("dsl_collider_set_volume", 9), ("dsl_collider_volume_query", 3)):
        assert len(_lib.EXPORTS[name][1]) == arity
    L = _lib.load_library()
    assert all(hasattr(L, name) for name in ("dsl_mesh_distance_volume", "dsl_collider_set_volume", "dsl_collider_volume_query"))
    assert "sdf.hip" in _lib.UNITS
