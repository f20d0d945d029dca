"""GPU: the C++ host mirror's SPH::SurfaceIndexed (dieselfluid_amd/host/dieselfluid.hpp) returns the fluid's iso-surface as
positions, vertex normals and indices -- one call of it, through tests/surface_mesh_host_check.cpp, held to the numpy
reference on the volume the same program downloads."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import surface_mesh_ref as mref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_mirror_returns_the_surface_as_an_indexed_mesh(tmp_path):
    from dieselfluid_amd import _lib
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, out = str(tmp_path / "surface_mesh_host_check"), str(tmp_path / "mesh.bin")
    libdir = os.path.dirname(_lib.library_path())
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "surface_mesh_host_check.cpp"), "-L" + libdir, "-ldslsph",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    # lattice A of test_gpu_volume.py over the reference's 12^3 scene; iso = rho0 / 2
    origin, step, dims = (-2.3, -2.1, -1.9), (0.37, 0.41, 0.43), (13, 11, 9)
    args = [exe, out, "12", "0.5"] + [repr(v) for v in origin + step] + [str(d) for d in dims]
    run = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "surface_mesh_host_check ok" in run.stdout, run.stdout + run.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    V, T, nvox = (int(v) for v in raw[:24].view(np.int64))
    assert nvox == dims[0] * dims[1] * dims[2] and V > 50 and T > 100
    body = raw[24:]
    assert body.size == 4 * (nvox + 6 * V + 3 * T)
    fl = body[:4 * (nvox + 6 * V)].view(np.float32)
    vol, pos, nrm = fl[:nvox], fl[nvox:nvox + 3 * V].reshape(V, 3), fl[nvox + 3 * V:].reshape(V, 3)
    idx = body[4 * (nvox + 6 * V):].view(np.int32).reshape(T, 3)
    from dieselfluid_amd.engine import reference_params
    iso = np.float32(0.5) * np.float32(reference_params(12).ref_density)
    wp, wn, wi = mref.mesh(vol, origin, step, dims, iso)
    assert (V, T) == (wp.shape[0], wi.shape[0]) and np.array_equal(idx, wi)
    assert np.array_equal(pos.view(np.uint32), wp.view(np.uint32)) and np.array_equal(nrm.view(np.uint32), wn.view(np.uint32))
