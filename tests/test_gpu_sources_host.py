"""GPU: the C++ host mirror's sources and sinks (dieselfluid_amd/host/dieselfluid.hpp: SPH::Emitter, SPH::Sink and their calls)
-- one run of tests/sources_host_check.cpp fills and drains a small tank on sph.Init's lattice, held bit for bit to the Python
binding on a handle with the same history, and its counts to tests/sources_ref.py's schedule."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sources_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N3, ROOM = 6, 808
FACE = dict(origin=(-0.7, 1.25, -0.5), u=(0.33, 0.0, 0.02), v=(0.01, 0.0, 0.34), nu=5, nv=4, velocity=(0.0, -20.0, 0.0))
INF = float("inf")
OUTLET = ((-INF, -INF, -INF), (INF, -0.9, INF))
EXTRA = np.array([[2.5, -0.95, 0.0], [2.5, 0.5, 0.0], [2.5, 0.0, 0.5]], dtype=f32)
EXTRA_V = np.array([[0, 1, 0], [0, 2, 0], [0, 3, 0]], dtype=f32)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_host_mirrors_tank_is_the_python_bindings(tmp_path):
    from dieselfluid_amd import SPHEngine, _lib, engine, scenes
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, out = str(tmp_path / "sources_host_check"), str(tmp_path / "out.bin")
    libdir = os.path.dirname(_lib.library_path())
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "sources_host_check.cpp"), "-L" + libdir, "-ldslsph",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    run = subprocess.run([exe, out, str(N3), str(ROOM)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sources_host_check ok" in run.stdout, run.stdout + run.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    counts = [int(c) for c in raw[:80].view(np.int64)]
    n = counts[8]
    fl = raw[80:].view(f32)
    assert fl.size == 6 * n
    pos, vel = fl[:3 * n].reshape(n, 3), fl[3 * n:].reshape(n, 3)
    # the Python binding on a handle with the same history: sph.Init's parameters, its lattice and passes, the same calls
    p = engine.reference_params(N3)
    p.capacity = p.n_particles + ROOM
    eng = SPHEngine(p, device=0)
    eng.upload("positions", scenes.lattice_positions(N3))
    eng.nn()
    eng.density_all()
    eng.external_all(np.array([0.0, f32(-9.81) * f32(eng.params.mass), 0.0], dtype=f32))
    eng.viscous_all()
    assert eng.add_emitter(**FACE) == 0 and eng.add_sink(*OUTLET) == 0
    eng.set_option("sink_every", 2)
    got = []
    for _ in range(6):
        eng.wcsph_step(1)
        got.append(eng.n)
    eng.emit(0)
    got.append(eng.n)
    eng.append_particles(EXTRA, EXTRA_V)
    got.append(eng.n)
    gone = eng.remove_particles()
    got += [eng.n, gone]
    print("counts:", got)
    assert got == counts
    # the tank filled and drained: a layer of 20 every step, the lowest lattice layer gone at the first look
    assert got[0] == N3 ** 3 - N3 ** 2 + 20 and got[6] == got[5] + 20 and got[7] == got[6] + 3 and got[8] == got[7] - gone and gone >= 1  # (one of the three sits in the outlet)
    assert eng.get_option("emitted") == 7 * 20 and eng.get_option("removed") == N3 ** 3 + 7 * 20 + 3 - n
    sched = sr.Schedule(N3 ** 3, N3 ** 3 + ROOM, [sr.Emitter(FACE["origin"], FACE["u"], FACE["v"], 5, 4, FACE["velocity"])], every=2)
    assert [s for s in range(6) if sched.looks(s)] == [0, 2, 4]
    eng.clear_emitters()
    eng.clear_sinks()
    eng.wcsph_step(1)
    assert eng.n == n and _same(pos, eng.download("positions")) and _same(vel, eng.download("velocities"))
    assert np.isfinite(pos).all()
    eng.close()
