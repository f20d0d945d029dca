"""The meshes, lattices and reference volumes the distance-volume tests share (CPU and GPU): each reference is computed once
by tests/sdf_ref.py and handed out read-only."""
import functools

import numpy as np

import sdf_ref

f32 = np.float32
STEP = 0.1
DIMS = (18, 17, 10)  # extent 1.7 x 1.6 x 0.9: more than one brick of 8 x 8 x 4 along every axis, none of them whole


def origin(x0=0.0):
    return (x0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(T, 3, 3) float32 vertices.  box: faces on lattice planes of the x0 = 0 lattice (x = 0.3, 1.3, y = 0.4, 1.2,
    z = 0.2, 0.6; subdiv 2 puts edges and vertices on lattice rows too).  triangle: one oblique triangle.  ico<level>.
    degenerate: ico0 plus a zero-area triangle (three points of a line) and a triangle with a repeated vertex.  quad: the
    box's +z face alone (open); rest: the box without it."""
    from dieselfluid_amd import scenes
    if name == "box":
        v = scenes.box_mesh((0.8, 0.8, 0.4), (1.0, 0.8, 0.4), 2)[0]
    elif name == "quad":
        v = mesh("box")[40:48]  # box_mesh: axis-major, -face then +face, 8 triangles each: z+ is the last
    elif name == "rest":
        v = mesh("box")[:40]
    elif name == "triangle":
        v = np.array([[[0.31, 0.22, 0.13], [1.42, 0.47, 0.38], [0.66, 1.33, 0.71]]], dtype=f32)
    elif name.startswith("ico"):
        v = scenes.icosphere_mesh((0.85, 0.8, 0.45), 0.4, int(name[3:]))[0]
    elif name == "degenerate":
        extra = np.array([[[0.25, 0.25, 0.25], [0.5, 0.25, 0.25], [0.75, 0.25, 0.25]],
                          [[0.5, 0.5, 0.25], [0.5, 0.5, 0.25], [0.75, 0.5, 0.5]]], dtype=f32)
        v = np.concatenate([mesh("ico0"), extra])
    else:
        raise KeyError(name)
    v = np.ascontiguousarray(v, dtype=f32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def distance(name, dims=DIMS, x0=0.0):
    """the unsigned, unbanded distance volume"""
    d = sdf_ref.distance(mesh(name), origin(x0), STEP, dims)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inside(name, dims=DIMS, x0=0.0):
    m = sdf_ref.inside(mesh(name), origin(x0), STEP, dims)
    m.setflags(write=False)
    return m


def volume(name, dims=DIMS, x0=0.0, band=np.inf, unsigned=False):
    """sdf_ref.volume from the two cached halves: min(d, band), negated inside"""
    d = np.minimum(distance(name, dims, x0), f32(band)).astype(f32)
    return d if unsigned else np.where(inside(name, dims, x0), -d, d).astype(f32)


def points64(dims=DIMS, x0=0.0):
    """(nz, ny, nx, 3) float64: the float32 lattice coordinates, exactly"""
    x, y, z = (a.astype(np.float64) for a in sdf_ref.axes(origin(x0), STEP, dims))
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([xx, yy, zz], axis=-1)
