"""GPU: the C++ host mirror's implicit colliders (dieselfluid_amd/host/dieselfluid.hpp: SPH::MeshDistance, SPH::Collider of a
VolumeCollider, SPH::ColliderDistances) -- one run of tests/sdf_host_check.cpp on sph.Init's lattice, held to tests/sdf_ref.py
bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sdf_cases as sc
import sdf_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_the_host_mirror_builds_a_distance_volume_and_collides_with_it(tmp_path):
    from dieselfluid_amd import _lib
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, mesh, out = str(tmp_path / "sdf_host_check"), str(tmp_path / "mesh.bin"), str(tmp_path / "sdf.bin")
    libdir = os.path.dirname(_lib.library_path())
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "sdf_host_check.cpp"), "-L" + libdir, "-ldslsph",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    # the shared icosphere, moved to the middle of sph.Init's lattice [-1, 1)^3
    origin, step, dims = (-0.85, -0.8, -0.45), (sc.STEP,) * 3, sc.DIMS
    shift = np.array(origin, dtype=f32) - np.array(sc.origin(), dtype=f32)
    verts = (sc.mesh("ico1") + shift[None, None, :]).astype(f32)
    with open(mesh, "wb") as f:
        f.write(np.int32(verts.shape[0]).tobytes())
        f.write(verts.tobytes())
    band, radius, rest = 0.25, 0.05, 0.5
    args = [exe, mesh, out, "12", repr(band), repr(radius), repr(rest)] + [repr(v) for v in origin + step] + [str(d) for d in dims]
    run = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sdf_host_check ok" in run.stdout, run.stdout + run.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    nvox, n = (int(v) for v in raw[:16].view(np.int64))
    assert nvox == dims[0] * dims[1] * dims[2] and n == 12 ** 3
    fl = raw[16:].view(f32)
    assert fl.size == nvox + 13 * n
    cuts = np.cumsum([nvox, 3 * n, n, 3 * n, 3 * n])
    vol, before, dist, normal, after, vel = np.split(fl, cuts)
    want_vol = sdf_ref.volume(verts, origin, sc.STEP, dims, band=band)
    assert np.array_equal(vol.view(np.uint32), want_vol.reshape(-1).view(np.uint32))
    before = before.reshape(n, 3)
    want_d, want_n = sdf_ref.collider_query(want_vol, origin, sc.STEP, before)
    assert np.array_equal(dist.view(np.uint32), want_d.view(np.uint32))
    assert np.array_equal(normal.reshape(n, 3).view(np.uint32), want_n.view(np.uint32))
    want_x, want_v, hit = sdf_ref.collider_pass(want_vol, origin, sc.STEP, before, np.zeros((n, 3), dtype=f32), radius, rest)
    assert hit.sum() > 20
    assert np.array_equal(after.reshape(n, 3).view(np.uint32), want_x.view(np.uint32))
    assert np.array_equal(vel.reshape(n, 3).view(np.uint32), want_v.view(np.uint32))
