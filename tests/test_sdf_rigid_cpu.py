"""CPU: the rule of the volume collider in rigid motion (include/dslsph.h: dsl_collider_volume_motion) as tests/sdf_rigid_ref.py
restates it -- the identity motion is the static rule bit for bit, a rotated and translated plane is met at the radius and
reflected against the body's velocity, the impulse is the momentum the particles lost, the two-level sum is a sum -- and
the names the header, the Python binding and the Go binding give to the new calls."""
import math
import os
import re

import numpy as np

import sdf_ref
import sdf_rigid_ref as rr
import test_gpu_sdf_collider as static_case  # its volume (a sphere with a NaN voxel) and its seeded cloud of 1000

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_the_identity_motion_is_the_static_rule_bit_for_bit():
    vol, (pos, vel) = static_case._volume(), static_case._particles()
    o, s, radius = static_case.ORIGIN, static_case.STEP, static_case.RADIUS
    for kw in (dict(), dict(rot=np.eye(3), trans=(0, 0, 0), lin_vel=(0, 0, 0), ang_vel=(0, 0, 0))):
        for rest in (0.0, 0.5):
            want_x, want_v, want_hit = sdf_ref.collider_pass(vol, o, s, pos, vel, radius, rest)
            x, v, hit, responded, J, tau = rr.rigid_pass(vol, o, s, pos, vel, radius, rest, 1.0, **kw)
            assert np.array_equal(_bits(x), _bits(want_x)) and np.array_equal(_bits(v), _bits(want_v))
            assert np.array_equal(hit, want_hit) and hit.sum() > 100
            assert 20 < responded.sum() < hit.sum() and not (responded & ~hit).any()
            assert not J[~responded].any() and not tau[~responded].any() and J[responded].any(axis=1).all()
        want_d, want_n = sdf_ref.collider_query(vol, o, s, pos)
        d, n = rr.rigid_query(vol, o, s, pos, kw.get("rot"), kw.get("trans"))
        assert np.array_equal(_bits(d), _bits(want_d)) and np.array_equal(_bits(n), _bits(want_n))


# ---- a plane, rotated about a skew axis and translated ----
PLANE_N = np.array([0.36, 0.48, 0.8])  # unit, in the body's frame
PLANE_C = 0.9
VORIGIN, VSTEP, VDIMS = (-0.2, -0.1, 0.0), (0.1, 0.125, 0.15), (12, 11, 9)
RADIUS = 0.07
ROT = rr.rotation((2.0, -1.0, 3.0), 0.9)
TRANS = np.array([0.15, -0.25, 0.1], dtype=f32)
LIN, ANG = np.array([0.3, 0.4, 0.9], dtype=f32), np.array([0.2, -0.3, 0.1], dtype=f32)
# Measured here, the reference against float64, coordinates up to 1.91: |distance to the moved plane after the response -
# radius| is at most 2.02e-7 (the static rule's 1.73e-7 and the two rotations), and |(v' - u).n + restitution (v - u).n| at
# most 8.09e-7 (5.40e-7 with restitution 0) at relative speeds up to 1.27: the float32 normal, u and the three products of
# the response each round.  Each asserted at four times the measured value.
PLANE_TOL = 4 * 2.02e-7
REFLECT_TOL = 4 * 8.09e-7


def _plane_volume():
    x, y, z = (a.astype(np.float64) for a in sdf_ref.axes(VORIGIN, VSTEP, VDIMS))
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return (PLANE_N[0] * xx + PLANE_N[1] * yy + PLANE_N[2] * zz - PLANE_C).astype(f32)


def _world_cloud(n=4000, seed=5):
    """a cloud over the lattice and a margin around it in the body's frame, taken to world coordinates"""
    rng = np.random.default_rng(seed)
    lo = np.array(VORIGIN) - 0.05
    hi = np.array(VORIGIN) + np.array(VSTEP) * (np.array(VDIMS) - 1) + 0.05
    local = rng.uniform(lo, hi, (n, 3))
    return (local @ ROT.astype(np.float64).T + TRANS.astype(np.float64)).astype(f32)


def _plane_distance64(x):
    """float64 distance of world points to the moved plane { t + R y : N.y = c }, R taken as supplied"""
    R = ROT.astype(np.float64)
    return ((x.astype(np.float64) - TRANS.astype(np.float64)) @ R) @ PLANE_N - PLANE_C


def test_a_rotated_plane_is_met_at_the_radius_and_reflects_against_the_bodys_velocity():
    vol, pos = _plane_volume(), _world_cloud()
    vel = np.zeros_like(pos)  # particles at rest: the body runs into them
    n64 = ROT.astype(np.float64) @ PLANE_N
    n64 /= np.linalg.norm(n64)
    q64 = pos.astype(np.float64) - TRANS.astype(np.float64)
    u64 = LIN.astype(np.float64) + np.cross(ANG.astype(np.float64), q64)
    for rest in (0.0, 0.5):
        x1, v1, hit, responded, J, tau = rr.rigid_pass(vol, VORIGIN, VSTEP, pos, vel, RADIUS, rest, 1.0, ROT, TRANS, LIN, ANG)
        assert 100 < hit.sum() < len(pos) // 2
        err = float(np.abs(_plane_distance64(x1)[hit] - RADIUS).max())
        vn_before = np.einsum("ij,j->i", -u64, n64)
        clear = hit & (vn_before < -1e-3)  # (the body approaches the particle, beyond any rounding of the sign)
        assert clear.sum() > 100 and responded[clear].all()
        vn_after = np.einsum("ij,j->i", v1.astype(np.float64) - u64, n64)
        rerr = float(np.abs(vn_after[clear] + rest * vn_before[clear]).max())
        print(f"restitution {rest}: |distance after - radius| = {err:.3e}, |(v' - u).n + e (v - u).n| = {rerr:.3e}, "
              f"|x| <= {np.abs(pos).max():.2f}, |v - u| <= {np.linalg.norm(u64[hit], axis=1).max():.2f}")
        assert err <= PLANE_TOL
        assert rerr <= REFLECT_TOL
        # a particle the body recedes from is pushed out and keeps its velocity; nobody else moves
        away = hit & (vn_before > 1e-3)
        assert np.array_equal(_bits(v1[away]), _bits(vel[away])) and not responded[away].any()
        assert np.array_equal(_bits(x1[~hit]), _bits(pos[~hit])) and np.array_equal(_bits(v1[~hit]), _bits(vel[~hit]))


def test_the_impulse_is_the_momentum_the_particles_lost():
    vol, (pos, vel) = static_case._volume(), static_case._particles()
    mass = 0.37
    R = rr.rotation((1, 2, 3), 0.7)
    x, v, hit, responded, J, tau = rr.rigid_pass(vol, static_case.ORIGIN, static_case.STEP, pos, vel, static_case.RADIUS, 0.5, mass, R,
                                                 (0.07, -0.04, 0.05), (0.3, -0.2, 0.1), (0.5, -1.0, 0.8))
    assert responded.sum() >= 30
    dv = v.astype(np.float64) - vel.astype(np.float64)
    assert not dv[~responded].any()
    got = J.astype(np.float64).sum(axis=0)
    want = -float(f32(mass)) * dv.sum(axis=0)
    # per particle and component J = fl(fl(m f) n) against m (v - fl(v - fl(f n))): two roundings of |m f n| on the left, one of
    # |f n| and one of |v'| (at most ulp(|v| + |f n|)) times m on the right -- four half-ulps of m (|v| + |f n|), summed
    fn = np.abs(dv)
    bound = (4 * 2.0 ** -24 * float(f32(mass)) * (np.abs(vel.astype(np.float64)) + fn)[responded]).sum(axis=0)
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)
    assert (np.abs(got) > 100 * bound).any()  # (the bound is no loophole: the sum is far above it)
    # the torque impulse is q x J
    q = pos.astype(np.float64) - np.array([0.07, -0.04, 0.05], dtype=f32).astype(np.float64)
    assert np.abs(tau.astype(np.float64) - np.cross(q, J.astype(np.float64))).max() < 1e-6 * np.abs(J).max()


def test_fold_is_a_sum_in_a_fixed_order():
    rng = np.random.default_rng(3)
    for n_slots in (1, 255, 256, 257, 1000, 65536, 65537, 70001):
        c = (rng.standard_normal((n_slots, 6)) * rng.uniform(0.0, 3.0, (n_slots, 1))).astype(f32)
        c[rng.uniform(size=n_slots) < 0.7] = 0  # most slots do not respond
        got = rr.fold(c)
        assert got.dtype == f32 and got.shape == (6,)
        for k in range(6):
            want = math.fsum(float(t) for t in c[:, k])
            bound = n_slots * 2.0 ** -24 * math.fsum(abs(float(t)) for t in c[:, k])
            assert abs(float(got[k]) - want) <= bound, (n_slots, k, float(got[k]), want, bound)
        # the same terms in another slot order: another float32 sum, inside the same bound
        other = rr.fold(c[::-1])
        for k in range(6):
            assert abs(float(other[k]) - math.fsum(float(t) for t in c[:, k])) <= n_slots * 2.0 ** -24 * math.fsum(abs(float(t)) for t in c[:, k])
    # every level written out, on a case small enough to do by hand: slots 0 and 300 hold 1 and 2^-24, the rest +0
    c = np.zeros((600, 1), dtype=f32)
    c[0], c[300] = 1.0, 2.0 ** -24
    assert rr.partials(c).reshape(-1).tolist() == [1.0, 2.0 ** -24, 0.0] and rr.fold(c)[0] == f32(1.0)  # (ties to even)
    c[301] = 2.0 ** -24  # lane 44 and 45 of workgroup 1 meet in its tree before they meet the 1
    assert rr.fold(c)[0] == f32(1.0) + f32(2.0 ** -23)


def test_fold_of_nothing_is_plus_zero():
    for n_slots in (1, 256, 1000, 70001):
        z = rr.fold(np.zeros((n_slots, 6), dtype=f32))
        assert z.shape == (6,) and not _bits(z).any()  # +0: not a bit set
    # a -0 contribution does not survive the +0 the lane sums start from
    c = np.zeros((300, 6), dtype=f32)
    c[7] = -0.0
    assert not _bits(rr.fold(c)).any()


def test_the_bindings_agree_on_the_new_names():
    from dieselfluid_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "dslsph.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(dsl_collider_volume_(?:motion|impulse))\s*\(([^)]*)\)", code)}
    assert {k: len(v.split(",")) for k, v in decl.items()} == {"dsl_collider_volume_motion": 5, "dsl_collider_volume_impulse": 4}
    assert len(_lib.EXPORTS["dsl_collider_volume_motion"][1]) == 5 and len(_lib.EXPORTS["dsl_collider_volume_impulse"][1]) == 4
    assert re.search(r"\bDSL_OPT_COLLIDER_VOLUME_MOVING\s*=\s*77\b", code)
    assert re.search(r"\bDSL_K_COUNT\s*=\s*19\b", code)  # the new launches are timed under DSL_K_COLLIDE
    assert engine.SPHEngine.OPTIONS["collider_volume_moving"] == 77
    for name in ("set_collider_volume_motion", "clear_collider_volume_motion", "collider_volume_impulse"):
        assert callable(getattr(engine.SPHEngine, name))
    assert "sdf_rigid.hip" in _lib.UNITS
    go = open(os.path.join(ROOT, "bindings", "go", "dslsph", "dslsph.go")).read()
    for name in ("C.dsl_collider_volume_motion(", "C.dsl_collider_volume_impulse(", "C.DSL_OPT_COLLIDER_VOLUME_MOVING",
                 "func (e *Engine) SetColliderVolumeMotion(", "func (e *Engine) ClearColliderVolumeMotion(",
                 "func (e *Engine) ColliderVolumeImpulse("):
        assert name in go, name
    hpp = open(os.path.join(ROOT, "dieselfluid_amd", "host", "dieselfluid.hpp")).read()
    for name in ("struct Motion", "Impulse(", "UpdateOrigin(", "IsStatic(", "dsl_collider_volume_motion(", "dsl_collider_volume_impulse("):
        assert name in hpp, name
