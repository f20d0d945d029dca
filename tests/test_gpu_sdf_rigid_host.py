"""GPU: the C++ host mirror's moving volume collider (dieselfluid_amd/host/dieselfluid.hpp: SPH::VolumeCollider::Motion,
SPH::UpdateMotion / UpdateOrigin / ClearMotion / IsStatic, SPH::Impulse) -- one run of tests/sdf_rigid_host_check.cpp on
sph.Init's lattice, held bit for bit to the Python binding on a handle with the same history and to tests/sdf_rigid_ref.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sdf_rigid_ref as rr
import test_gpu_sdf_collider as static_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N3 = 12
ORIGIN, STEP, DIMS = (-0.8, -0.75, -0.85), (0.1, 0.1, 0.1), (17, 16, 18)
RADIUS, REST = 0.05, 0.5
POSE = dict(rot=rr.rotation((3, -1, 2), 0.5), trans=(0.05, -0.03, 0.04), lin_vel=(0.4, 0.3, -0.2), ang_vel=(0.3, 0.6, -0.9))


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_the_host_mirrors_motion_and_impulse_are_the_python_bindings(tmp_path):
    from dieselfluid_amd import SPHEngine, _lib, engine
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, src, out = str(tmp_path / "sdf_rigid_host_check"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    libdir = os.path.dirname(_lib.library_path())
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "sdf_rigid_host_check.cpp"), "-L" + libdir, "-ldslsph",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    vol = static_case._sphere_volume(ORIGIN, STEP, DIMS, np.array([0.0, 0.05, -0.05]), 0.45)  # inside sph.Init's lattice [-1, 1)^3
    R, t, lv, av = rr.motion(**POSE)
    with open(src, "wb") as f:
        f.write(np.array(DIMS, dtype=np.int32).tobytes())
        for a in (np.array(ORIGIN, dtype=f32), np.array(STEP, dtype=f32), R, t, lv, av, vol):
            f.write(np.ascontiguousarray(a, dtype=f32).tobytes())
    run = subprocess.run([exe, src, out, str(N3), repr(RADIUS), repr(REST)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sdf_rigid_host_check ok" in run.stdout, run.stdout + run.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    n = int(raw[:8].view(np.int64)[0])
    assert n == N3 ** 3
    fl = raw[8:].view(f32)
    assert fl.size == 13 * n + 18
    before, dist, normal, after, vel, kept, taken, left = np.split(fl, np.cumsum([3 * n, n, 3 * n, 3 * n, 3 * n, 6, 6]))
    before, normal, after, vel = (a.reshape(n, 3) for a in (before, normal, after, vel))
    # the Python binding on a handle with the same history: sph.Init's parameters, its lattice, one neighbour build
    eng = SPHEngine(engine.reference_params(N3), device=0)
    eng.upload("positions", before)
    eng.nn()
    eng.set_collider_volume(vol, ORIGIN, STEP, radius=RADIUS, restitution=REST)
    eng.set_collider_volume_motion(**POSE)
    py_d, py_n = eng.collider_volume_query()
    ids = eng.download_ids()
    eng.collide()
    py_imp = np.concatenate(eng.collider_volume_impulse())
    assert _same(dist, py_d) and _same(normal, py_n)
    assert _same(after, eng.download("positions")) and _same(vel, eng.download("velocities"))
    assert _same(kept, py_imp) and _same(taken, py_imp) and not left.view(np.uint32).any()
    # ... and the reference
    x, v, hit, responded, J, tau = rr.rigid_pass(vol, ORIGIN, STEP, before, np.zeros_like(before), RADIUS, REST, float(eng.params.mass), **POSE)
    assert hit.sum() > 40 and responded.sum() > 20
    assert _same(after, x) and _same(vel, v) and _same(kept, rr.fold(np.concatenate([J, tau], axis=1)[ids])) and kept.any()
    eng.close()
