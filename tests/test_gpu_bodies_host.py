"""GPU: the C++ host mirror's rigid bodies (dieselfluid_amd/host/dieselfluid.hpp: SPH::Body, SPH::Bodies) -- one run of
tests/bodies_host_check.cpp on sph.Init's lattice, held bit for bit to the Python binding on a handle with the same history
and, for the pass, to tests/bodies_ref.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bodies_ref as br
import test_gpu_sdf_collider as static_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N3 = 12
ORIGIN, STEP, DIMS = (-0.6, -0.6, -0.6), (0.1, 0.1, 0.1), (13, 13, 13)
KEYS = ("quat", "trans", "lin_vel", "ang_vel")


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _bodies():
    vol = static_case._sphere_volume(ORIGIN, STEP, DIMS, np.zeros(3), 0.45)  # centred on its own frame's origin
    return [
        br.body(vol, ORIGIN, STEP, br.props(inv_mass=0.5, inv_inertia=(1.0, 2.0, 3.0), accel=(0.0, -1.0, 0.0), radius=0.05, restitution=0.5),
                br.state(quat=br.axis_angle((3, -1, 2), 0.5), trans=(0.1, 0.05, -0.1), lin_vel=(0.4, 0.3, -0.2), ang_vel=(0.3, 0.6, -0.9))),
        br.body(vol, ORIGIN, STEP, br.props(radius=0.08, restitution=0.0),
                br.state(quat=(2.0, 0.0, 0.5, 0.0), trans=(-0.25, 0.2, 0.3), lin_vel=(-0.3, 0.0, 0.1), ang_vel=(0.0, 1.0, 0.0))),
    ]


def _reading(fl):
    return {k: a for k, a in zip(KEYS, np.split(fl[:13], [4, 7, 10]))}, fl[13:19]


def test_the_host_mirrors_bodies_are_the_python_bindings(tmp_path):
    from dieselfluid_amd import SPHEngine, _lib, engine
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, src, out = str(tmp_path / "bodies_host_check"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    libdir = os.path.dirname(_lib.library_path())
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "bodies_host_check.cpp"), "-L" + libdir, "-ldslsph",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    bodies = _bodies()
    with open(src, "wb") as f:
        f.write(np.array(DIMS, dtype=np.int32).tobytes())
        f.write(np.array(ORIGIN, dtype=f32).tobytes() + np.array(STEP, dtype=f32).tobytes())
        for bd in bodies:
            p, s = br.api_props(bd["props"]), br.api_state(bd["state"])
            f.write(np.array([p["inv_mass"], *p["inv_inertia"], *p["accel"], p["radius"], p["restitution"]], dtype=f32).tobytes())
            f.write(np.array([*s["quat"], *s["trans"], *s["lin_vel"], *s["ang_vel"]], dtype=f32).tobytes())
        f.write(np.ascontiguousarray(bodies[0]["vol"], dtype=f32).tobytes())
    run = subprocess.run([exe, src, out, str(N3)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "bodies_host_check ok" in run.stdout, run.stdout + run.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    n = int(raw[:8].view(np.int64)[0])
    assert n == N3 ** 3
    fl = raw[8:].view(f32)
    assert fl.size == 16 * n + 4 * 19
    before, dist, normal, after, vel, r0, r1, stepped, s0, s1 = np.split(fl, np.cumsum([3 * n, n, 3 * n, 3 * n, 3 * n, 19, 19, 3 * n, 19]))
    before, normal, after, vel, stepped = (a.reshape(n, 3) for a in (before, normal, after, vel, stepped))
    # the Python binding on a handle with the same history: sph.Init's parameters, its lattice, the same calls
    eng = SPHEngine(engine.reference_params(N3), device=0)
    eng.upload("positions", before)
    eng.nn()  # sph.Init's own passes (fluid.go:72-75), so that the steps below start from the same forces
    eng.density_all()
    eng.external_all(np.array([0.0, f32(-9.81) * f32(eng.params.mass), 0.0], dtype=f32))
    eng.viscous_all()
    for b, bd in enumerate(bodies):
        assert eng.add_body(bd["vol"], ORIGIN, STEP, br.api_props(bd["props"]), br.api_state(bd["state"])) == b
    py_d, py_n = eng.body_query(1)
    assert _same(dist, py_d) and _same(normal, py_n)
    ids = eng.download_ids()
    eng.collide()
    assert _same(after, eng.download("positions")) and _same(vel, eng.download("velocities"))
    x, v, hit, responded, contrib = br.bodies_pass(bodies, before, np.zeros_like(before), float(eng.params.mass))
    assert (hit.sum(axis=1) > 40).all() and (responded.sum(axis=1) > 20).all()
    assert _same(after, x) and _same(vel, v)
    want = br.totals(contrib, ids)
    for b, r in enumerate((r0, r1)):
        state, acc = _reading(r)
        py_state, imp, trq = eng.body_state(b)
        assert all(_same(state[k], py_state[k]) and _same(state[k], bodies[b]["state"][k]) for k in KEYS), b
        assert _same(acc, np.concatenate([imp, trq])) and _same(acc, want[b]) and acc.any(), b
    eng.wcsph_step(2)
    assert _same(stepped, eng.download("positions"))
    for b, r in enumerate((s0, s1)):
        state, acc = _reading(r)
        py_state, imp, trq = eng.body_state(b)
        assert all(_same(state[k], py_state[k]) for k in KEYS) and _same(acc, np.concatenate([imp, trq])), b
        assert not _same(state["trans"], bodies[b]["state"]["trans"])  # (the steps integrated the poses)
    eng.close()
