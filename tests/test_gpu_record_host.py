"""GPU: the C++ host mirror's frame recorder (dieselfluid_amd/host/dieselfluid.hpp: SPH::Recorder, SetRecorder, RecordNow,
PollFrames, NextFrame, WriteAnimation) -- one run of tests/record_host_check.cpp records on sph.Init's lattice; its frames and
the animation file it writes are byte for byte the Python binding's on a handle with the same history."""
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N3 = 6


def test_the_host_mirrors_frames_and_file_are_the_python_bindings(tmp_path):
    from dieselfluid_amd import SPHEngine, _lib, animation, engine, scenes
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, frame0, anim = str(tmp_path / "record_host_check"), str(tmp_path / "frame0.bin"), str(tmp_path / "host.dslanim")
    libdir = os.path.dirname(_lib.library_path())
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "record_host_check.cpp"), "-L" + libdir, "-ldslsph",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    run = subprocess.run([exe, frame0, anim, str(N3)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "record_host_check ok" in run.stdout, run.stdout + run.stderr
    # the Python binding on a handle with the same history: sph.Init's parameters, its lattice and passes, the same calls
    p = engine.reference_params(N3)
    eng = SPHEngine(p, device=0)
    eng.upload("positions", scenes.lattice_positions(N3))
    eng.nn()
    eng.density_all()
    eng.external_all(np.array([0.0, f32(-9.81) * f32(eng.params.mass), 0.0], dtype=f32))
    eng.viscous_all()
    eng.set_recorder(every=2, fields=("velocities", "densities"), slots=8)
    eng.wcsph_step(6)
    eng.record_now()
    frames = [eng.read_frame() for _ in range(4)]
    eng.set_recorder(stride=3, fields=("velocities",), encoding="q16", first_step=6, slots=2)
    eng.wcsph_step(2)
    frames += [eng.read_frame() for _ in range(2)]
    assert eng.record_poll() == (2, 0, 0)
    eng.close()
    assert [animation.decode_frame(f)["step"] for f in frames] == [0, 2, 4, 6, 6, 7]
    assert open(frame0, "rb").read() == frames[0]
    mine = str(tmp_path / "python.dslanim")
    with animation.AnimationWriter(mine) as w:
        for f in frames[1:]:
            w.append(f)
    assert open(anim, "rb").read() == open(mine, "rb").read()
    back = animation.read_animation(anim)
    assert back == frames[1:]
    last = animation.decode_frame(back[-1])
    assert last["encoding"] == 1 and last["auto_box"] == 1 and last["count"] == -(-N3 ** 3 // 3) and np.isfinite(last["positions"]).all()
    assert last["velocities"].shape == (last["count"], 3) and "densities" not in last
