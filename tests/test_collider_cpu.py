"""tests/collider_ref.py -- the numpy float32 restatement of Mesh.Collision (geom/mesh/mesh.go:41-57,
geom/triangle/tri.go:37-101) the GPU collider tests compare against -- checked against values worked out by hand, and
the C++ host mirror's mesh::InitMesh / Mesh::Collision (dieselfluid_amd/host/dieselfluid.hpp) checked against it bit for
bit.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import collider_ref as cr

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the unit right triangle in the plane y = 0: a = (0,0,0), b = (1,0,0), c = (0,0,1); e0 = x, e1 = z, so that
# d00 = d11 = 1, d01 = 0, denom = 1 and (u, v, w) = (P.x, P.z, 1 - P.z - P.x)
TRI = np.array([[[0, 0, 0], [1, 0, 0], [0, 0, 1]]], dtype=f32)
UP = np.array([[0, 1, 0]], dtype=f32)
DT, R = 0.01, 0.125  # r = 2^-3: its square and the squares of the heights below are exact


def _one(P, V, verts=TRI, normals=UP, dt=DT, r=R):
    tri, n, c, p, k = cr.collide(np.array([P], dtype=f32), np.array([V], dtype=f32), verts, normals, dt, r)
    return int(tri[0]), n[0], c[0], p[0], k[0]


def test_falling_straight_at_a_horizontal_triangle_collides_iff_within_r():
    # V = (0,-1,0): n.V = -1, d = (a - P).n = -y, k = y, p0 = (x, 0, z), dist = |y|
    above = np.nextafter(f32(0.125), f32(1))
    for y, hit in ((0.0625, True), (0.125, True), (above, False), (0.5, False), (-0.125, True), (-above, False)):
        tri, n, c, p, k = _one([0.25, y, 0.25], [0, -1, 0])
        assert (tri == 0) == hit, y
        if hit:
            assert k == f32(y)
            assert n.tolist() == [0, 1, 0] and c.tolist() == [0.25, 0.25, 0.5]
            assert p.tolist() == [0.25, float(f32(y) + f32(-1) * -f32(DT)), 0.25]  # P + V * (-dt)
        else:
            assert not n.any() and not c.any() and not p.any()


def test_the_substitute_is_used_when_the_normal_and_the_velocity_are_exactly_perpendicular():
    # V = (1,0,0): n.V == 0 -> 0.0001; k = -y / 0.0001, p0 = P + V k, dist = |k|: collides iff |y| / 0.0001 <= r
    for y, hit in ((2.0 ** -17, True), (2.0 ** -16, False)):  # 0.0763 <= 0.125 < 0.1526
        tri, _n, _c, _p, k = _one([0.25, y, 0.25], [1, 0, 0])
        assert (tri == 0) == hit
        if hit:
            assert k == f32(-f32(y)) / f32(0.0001)
    # with any other divisor in place of 0 the particle 2^-17 above the plane would be missed or NaN
    assert abs(float(f32(2.0 ** -17) / f32(0.0001)) - 0.0762939) < 1e-6


def test_a_particle_at_rest_never_collides():
    assert _one([0.25, 0.0, 0.25], [0, 0, 0])[0] == -1
    assert _one([0.25, 0.0, 0.25], [0, -1e-30, 0])[0] == -1  # |V|^2 underflows to 0 in float32: Mag(V) == 0
    assert _one([0.25, 0.0, 0.25], [0, -1e-18, 0])[0] == 0


def test_a_zero_normal_collides_anywhere_inside_the_prism():
    zero = np.zeros((1, 3), dtype=f32)
    # n = 0: n.V -> 0.0001, d = 0, k = 0, dist = 0 <= r whatever the height; only the barycentric test decides
    for P, hit in (([0.25, 100.0, 0.25], True), ([0.25, -7.0, 0.5], True), ([0.75, 100.0, 0.5], False),
                   ([-0.01, 100.0, 0.25], False)):
        tri, _n, c, _p, k = _one(P, [0.3, -2.0, 0.1], normals=zero)
        assert (tri == 0) == hit, P
        if hit:
            assert k == 0 and c[0] == f32(P[0]) and c[1] == f32(P[2])


def test_a_degenerate_triangle_never_collides():
    flat = np.array([[[0, 0, 0], [0, 0, 0], [0, 0, 1]]], dtype=f32)     # b == a: e0 = 0, denom = 0
    line = np.array([[[0, 0, 0], [1, 0, 0], [2, 0, 0]]], dtype=f32)     # collinear: d00 d11 == d01^2
    for verts in (flat, line):
        assert cr.triangle_terms(verts)[6][0] == 0
        for P in ([0.0, 0.0, 0.0], [0.25, 0.01, 0.0], [0.0, 0.0, 0.5]):
            assert _one(P, [0, -1, 0], verts=verts)[0] == -1


def test_of_two_stacked_triangles_the_lower_index_wins():
    two = np.concatenate([TRI + f32([0, 0.03125, 0]), TRI])  # triangle 0 in the plane y = 1/32, triangle 1 in y = 0
    nn = np.concatenate([UP, UP])
    tri, *_ = _one([0.25, 0.0625, 0.25], [0, -1, 0], verts=two, normals=nn)
    assert tri == 0
    assert _one([0.25, 0.0625, 0.25], [0, -1, 0], verts=two[::-1].copy(), normals=nn)[3][1] == f32(0.0625) + f32(0.01)
    # ... and alone each of them collides: both qualify
    assert _one([0.25, 0.0625, 0.25], [0, -1, 0], verts=two[1:], normals=UP)[0] == 0


def test_a_triangle_that_passes_the_distance_but_fails_the_barycentric_test_does_not_stop_the_loop():
    far = TRI + f32([10, 0, 0])  # same plane, ten units along x: dist <= r holds, (u, v, w) = (-9.75, ...) does not
    two = np.concatenate([far, TRI])
    nn = np.concatenate([UP, UP])
    tri, n, c, _p, _k = _one([0.25, 0.0625, 0.25], [0, -1, 0], verts=two, normals=nn)
    assert tri == 1 and c.tolist() == [0.25, 0.25, 0.5] and n.tolist() == [0, 1, 0]
    assert _one([0.25, 0.0625, 0.25], [0, -1, 0], verts=far)[0] == -1


def test_the_response_reflects_an_approaching_particle_and_leaves_a_receding_one():
    P = np.array([[0.25, 0.0625, 0.25], [0.25, 0.0625, 0.25], [0.25, 0.5, 0.25]], dtype=f32)
    V = np.array([[0.5, -1, 0], [0.5, 1, 0], [0.5, -1, 0]], dtype=f32)  # approaching, receding (k < 0), out of reach
    P2, V2, moved = cr.respond(P, V, TRI, UP, DT, R, 0.5)
    assert moved.tolist() == [True, False, False]
    assert P2[0].tolist() == [float(f32(0.25) + f32(0.5) * -f32(DT)), float(f32(0.0625) + f32(-1) * -f32(DT)), 0.25]
    assert V2[0].tolist() == [0.5, 0.5, 0.0]  # v - n (1.5 (v.n)) = -1 + 1.5
    assert np.array_equal(P2[1:], P[1:]) and np.array_equal(V2[1:], V[1:])
    # the sign of n means nothing to either formula
    P3, V3, moved3 = cr.respond(P, V, TRI, -UP, DT, R, 0.5)
    assert np.array_equal(P3, P2) and np.array_equal(V3, V2) and np.array_equal(moved3, moved)


def test_the_distance_threshold_is_the_monotone_inverse_of_mag():
    for r in (0.125, 0.1, 1e-3, 3.0, 0.0, 1e-20):
        s = cr.dist_threshold(r)
        m = lambda x: f32(np.sqrt(np.float64(x)))
        assert m(s) <= f32(r) and m(np.nextafter(s, f32(np.inf))) > f32(r)
    assert cr.dist_threshold(-1.0) == -1 and cr.dist_threshold(float("nan")) == -1


# ---- the C++ host mirror ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tests/collider_host_check.cpp built against dieselfluid.hpp with the host layer's flags (no device code, no
    library: the mesh functions are plain host arithmetic)"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("collider_host") / "collider_host_check")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "collider_host_check.cpp")])

    def run(verts, normals, P, V, dt, r, origin=None):
        verts = np.ascontiguousarray(verts, dtype=f32).reshape(-1, 3, 3)
        T, N = verts.shape[0], len(P)
        nrm = np.zeros((T, 3), dtype=f32) if normals is None else np.ascontiguousarray(normals, dtype=f32)
        src, dst = exe + ".in", exe + ".out"
        with open(src, "wb") as f:
            f.write(struct.pack("<iiifffff", T, N, 1 if normals is None else 0, dt, r, *(origin or (0.0, 0.0, 0.0))))
            for a in (verts, nrm, P, V):
                f.write(np.ascontiguousarray(a, dtype=f32).tobytes())
        subprocess.check_call([exe, src, dst])
        raw = np.fromfile(dst, dtype=f32)
        used = raw[:3 * T].reshape(T, 3)
        rec = raw[3 * T:].reshape(N, 10)
        return used, rec[:, 0].copy().view(np.int32), rec[:, 1:4], rec[:, 4:7], rec[:, 7:10]

    return run


def _hand_cases():
    """the particles of the tests above, as one batch against one mesh that holds every triangle they use"""
    verts = np.concatenate([TRI + f32([10, 0, 0]), TRI + f32([0, 0.03125, 0]), TRI,
                            np.array([[[0, 0, 0], [0, 0, 0], [0, 0, 1]]], dtype=f32), TRI + f32([0, 0, 5])])
    normals = np.array([[0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 0, 0]], dtype=f32)
    above = float(np.nextafter(f32(0.125), f32(1)))
    P = [[0.25, 0.0625, 0.25], [0.25, 0.125, 0.25], [0.25, above, 0.25], [0.25, -0.125, 0.25], [0.25, 2.0 ** -17, 0.25],
         [0.25, 2.0 ** -16, 0.25], [0.25, 0.0, 0.25], [0.25, 100.0, 5.25], [0.75, 100.0, 5.5], [10.25, 0.0625, 0.25],
         [0.25, 0.14, 0.25], [0.25, 0.0625, 0.25]]
    V = [[0, -1, 0], [0, -1, 0], [0, -1, 0], [0, -1, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0], [0.3, -2, 0.1], [0.3, -2, 0.1],
         [0, -1, 0], [0, -1, 0], [0.5, 1, 0]]
    return verts, normals, np.array(P, dtype=f32), np.array(V, dtype=f32)


def _random_cases(seed=7, n=400, T=40):
    rng = np.random.default_rng(seed)
    verts = rng.uniform(-1, 1, (T, 3, 3)).astype(f32)
    P = rng.uniform(-1, 1, (n, 3)).astype(f32)
    V = rng.normal(0, 1, (n, 3)).astype(f32)
    V[::10] = 0
    V[1::10, 1] = 0
    return verts, P, V


def test_host_mirror_collision_agrees_with_the_reference_on_the_hand_cases(host_check):
    verts, normals, P, V = _hand_cases()
    tri, n, c, p, _k = cr.collide(P, V, verts, normals, DT, R)
    # by hand: triangle 0 lies ten units away (never inside), 1 in the plane y = 1/32, 2 in y = 0, 3 is degenerate, 4 has a
    # zero normal and sits at z + 5.  Heights up to 1/32 + r reach triangle 1 first; y = -1/8 is 5/32 from it and exactly r
    # from triangle 2; the perpendicular mover at 2^-17 reaches only triangle 2, at 2^-16 nothing
    assert tri.tolist() == [1, 1, 1, 2, 2, -1, -1, 4, -1, 0, 1, 1]
    used, htri, hn, hc, hp = host_check(verts, normals, P, V, DT, R)
    assert np.array_equal(used, normals)
    assert np.array_equal(htri, tri)
    for got, want in ((hn, n), (hc, c), (hp, p)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_host_mirror_init_mesh_and_collision_agree_with_the_reference_on_random_meshes(host_check):
    verts, P, V = _random_cases()
    normals = cr.init_mesh_normals(verts)
    assert not normals[-1].any() and np.all(np.abs(cr.mag(normals[:-1]) - 1) < 1e-6)  # the last one stays zero
    r = 0.25
    tri, n, c, p, _k = cr.collide(P, V, verts, normals, DT, r)
    frac = np.mean(tri >= 0)
    assert 0.05 < frac < 0.95, frac
    assert np.all(tri[::10] == -1)  # Mag(V) == 0
    used, htri, hn, hc, hp = host_check(verts, None, P, V, DT, r, origin=(0.0, 0.0, 0.0))
    assert np.array_equal(used.view(np.uint32), normals.view(np.uint32))  # InitMesh, both quirks included
    assert np.array_equal(htri, tri)
    for got, want in ((hn, n), (hc, c), (hp, p)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the flip is dropped: normals that point away from the origin stay as they are
    a = verts[:, 0]
    assert np.any(np.einsum("ij,ij->i", normals[:-1], a[:-1]) > 0)
