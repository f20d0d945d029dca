"""The pinned inputs of the contact tests (tests/test_contact_cpu.py asserts what they cover on the reference,
tests/test_gpu_contact.py runs them on the device): analytic sphere and cube volumes centred on their lattices, and the scenes
built from them."""
import functools

import numpy as np

import bodies_ref as br

f32 = np.float32
STEP = 0.02
BOX_MIN, BOX_MAX = (0.0, 0.0, 0.0), (4.0, 4.0, 4.0)
GRAVITY = (0.0, -9.81, 0.0)
DT = 0.002


def lattice(n, step=STEP):
    """(origin, step) of n^3 voxels centred on 0"""
    o = -0.5 * (n - 1) * step
    return (o, o, o), (step, step, step)


def _grid(n, step):
    c = (np.arange(n) - 0.5 * (n - 1)) * step
    return np.meshgrid(c, c, c, indexing="ij")  # z, y, x


@functools.lru_cache(maxsize=None)
def sphere(n=24, radius_steps=8.3, step=STEP):
    """the distance to a sphere of radius_steps voxel steps, float64 rounded to float32"""
    z, y, x = _grid(n, step)
    vol = (np.sqrt(x * x + y * y + z * z) - radius_steps * step).astype(f32)
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def cube(n=24, half_steps=7.3, step=STEP):
    """the distance to an axis-aligned cube of half-side half_steps voxel steps"""
    z, y, x = (np.abs(a) - half_steps * step for a in _grid(n, step))
    out = np.sqrt(np.maximum(x, 0) ** 2 + np.maximum(y, 0) ** 2 + np.maximum(z, 0) ** 2)
    vol = (out + np.minimum(np.maximum(x, np.maximum(y, z)), 0)).astype(f32)
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def sphere_nan():
    """the sphere with one voxel of its innermost shell NaN"""
    vol = sphere().copy()
    assert vol[12, 12, 4] <= 0 < vol[12, 12, 3]
    vol[12, 12, 4] = np.nan
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def sphere_unsigned():
    vol = np.abs(sphere())
    vol.setflags(write=False)
    return vol


def body(vol, props, state=None, step=STEP):
    o, s = lattice(vol.shape[0], step)
    return br.body(vol, o, s, br.props(**props), br.state(**state) if state else None)


BALL = dict(inv_mass=1.0, inv_inertia=(90.0, 90.0, 90.0), accel=GRAVITY, radius=0.01, restitution=0.3)
REST_HEIGHT = 7.5 * STEP  # the sphere's innermost shell reaches 7.5 steps below its centre


def dropped_sphere():
    return [body(sphere(), BALL, dict(trans=(1.0, 0.5, 1.0)))]


def sunk_sphere():
    """the sphere a third under the floor, turned, with both velocities: 656 points in three workgroups"""
    return [body(sphere(), BALL, dict(quat=br.axis_angle((1, 2, 3), 0.7), trans=(1.0, 0.1, 1.0), lin_vel=(0.3, -1.0, 0.2),
                                      ang_vel=(0.5, -1.0, 0.8)))]


def corner_cube():
    """a rotated cube in the corner of the box, touching three walls"""
    p = dict(inv_mass=0.8, inv_inertia=(60.0, 70.0, 80.0), accel=GRAVITY, radius=0.01, restitution=0.1)
    return [body(cube(), p, dict(quat=br.axis_angle((1, -1, 0.5), 0.5), trans=(0.12, 0.1, 0.13), lin_vel=(-0.5, -0.8, -0.3),
                                 ang_vel=(0.2, 0.1, -0.4)))]


def big_cube():
    """66,152 points in 259 workgroups, half under the floor: the fold's second lane-strided trip"""
    p = dict(inv_mass=0.5, inv_inertia=(1.0, 1.0, 1.0), radius=0.01, restitution=0.0)
    return [body(cube(116, 53.3), p, dict(quat=br.axis_angle((0, 0, 1), 0.1), trans=(2.0, 0.0, 2.0)))]


def glancing_pair():
    """two spheres of unequal mass on a glancing course, restitution 1, no gravity"""
    a = dict(inv_mass=1.0, inv_inertia=(90.0, 90.0, 90.0), radius=0.01, restitution=1.0)
    b = dict(inv_mass=0.5, inv_inertia=(45.0, 45.0, 45.0), radius=0.01, restitution=1.0)
    return [body(sphere(), a, dict(trans=(1.0, 2.0, 1.0), lin_vel=(1.0, 0.0, 0.0))),
            body(sphere(), b, dict(trans=(1.6, 2.05, 1.0), lin_vel=(-1.0, 0.0, 0.0)))]


def overlapping_pair():
    """two turned spheres that overlap by a few voxels, approaching"""
    a = dict(inv_mass=1.0, inv_inertia=(90.0, 80.0, 70.0), radius=0.01, restitution=0.5)
    b = dict(inv_mass=0.5, inv_inertia=(45.0, 40.0, 50.0), radius=0.01, restitution=0.8)
    return [body(sphere(), a, dict(quat=br.axis_angle((1, 2, 3), 0.7), trans=(1.0, 2.0, 1.0), lin_vel=(0.6, 0.1, 0.0), ang_vel=(0.0, 0.5, 1.0))),
            body(sphere(), b, dict(quat=br.axis_angle((-2, 1, 0.5), 1.1), trans=(1.27, 2.08, 1.05), lin_vel=(-0.4, 0.0, 0.1),
                                   ang_vel=(0.3, 0.0, -0.2)))]


def three_bodies():
    """the overlapping pair and a cube that overlaps the second sphere alone"""
    c = dict(inv_mass=0.7, inv_inertia=(60.0, 70.0, 80.0), accel=GRAVITY, radius=0.01, restitution=0.2)
    return overlapping_pair() + [body(cube(), c, dict(quat=br.axis_angle((0, 1, 0), 0.3), trans=(1.45, 1.9, 1.2), lin_vel=(0.0, 0.3, -0.2)))]
