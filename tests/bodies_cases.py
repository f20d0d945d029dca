"""The pinned inputs of the rigid-body tests (tests/test_bodies_cpu.py asserts what they cover, tests/test_gpu_bodies.py runs
them on the device): bodies built from the sphere volume with its NaN voxel, over the seeded cloud of 1000 of
test_gpu_sdf_collider."""
import functools

import numpy as np

import bodies_ref as br
import test_gpu_sdf_collider as static_case

f32 = np.float32
ORIGIN, STEP, RADIUS, N = static_case.ORIGIN, static_case.STEP, static_case.RADIUS, static_case.N
# the general pose of the issue: 0.7 rad about (1, 2, 3), translated, with both velocities
GENERAL = dict(quat=br.axis_angle((1, 2, 3), 0.7), trans=(0.07, -0.04, 0.05), lin_vel=(0.3, -0.2, 0.1), ang_vel=(0.5, -1.0, 0.8))


def sphere_body(props, state=None):
    return br.body(static_case._volume(), ORIGIN, STEP, br.props(**props), br.state(**state) if state else None)


def three_bodies():
    """Three bodies with different radius and restitution.  Bodies 0 and 1 are the same sphere at two poses about its
    radius apart, so that their bands -- and their insides: a particle inside is moved as well -- overlap; body 2 stands apart
    at the cloud's corner.  All three move, so that particles at rest respond too."""
    return [
        sphere_body(dict(radius=RADIUS, restitution=0.5), GENERAL),
        sphere_body(dict(radius=0.12, restitution=0.0),
                    dict(quat=br.axis_angle((-2, 1, 0.5), 1.1), trans=(0.2, 0.2, 0.0), lin_vel=(-0.4, 0.1, 0.3), ang_vel=(1.0, 0.4, -0.6))),
        sphere_body(dict(radius=0.03, restitution=0.9),
                    dict(quat=br.axis_angle((0, 1, 1), 2.0), trans=(0.45, 0.4, 0.3), lin_vel=(-0.5, -0.5, -0.4), ang_vel=(0.0, 0.7, 0.2))),
    ]


@functools.lru_cache(maxsize=None)
def three_bodies_pass(order=(0, 1, 2)):
    """the reference pass of three_bodies() in the given order over the cloud, mass 1: read-only arrays"""
    pos, vel = static_case._particles()
    bodies = three_bodies()
    out = br.bodies_pass([bodies[b] for b in order], pos, vel, 1.0)
    for a in out:
        a.setflags(write=False)
    return out
