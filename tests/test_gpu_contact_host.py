"""GPU: the C++ host mirror's contact stage (dieselfluid_amd/host/dieselfluid.hpp: SPH::Bodies::ContactPoints, ContactPass,
ContactTable, Contact, Contacts) -- one run of tests/contact_host_check.cpp on sph.Init's lattice, held bit for bit to the
Python binding on a handle with the same history and, for the points, the table and the solve, to tests/contact_ref.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bodies_ref as br
import contact_cases as cc
import contact_ref as cr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
N3 = 12
KEYS = ("quat", "trans", "lin_vel", "ang_vel")


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _states(eng):
    return np.stack([np.concatenate([eng.body_state(b)[0][k] for k in KEYS]) for b in range(2)])


def test_the_host_mirrors_contact_stage_is_the_python_bindings(tmp_path):
    from dieselfluid_amd import SPHEngine, _lib, engine, scenes
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe, src, out = str(tmp_path / "contact_host_check"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    libdir = os.path.dirname(_lib.library_path())
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "contact_host_check.cpp"), "-L" + libdir, "-ldslsph",
                           "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    # the overlapping pair, far above sph.Init's particles
    bodies = cc.overlapping_pair()
    for bd in bodies:
        bd["state"] = br.state(quat=bd["state"]["quat_given"], trans=bd["state"]["trans"] + f32(20), lin_vel=bd["state"]["lin_vel"],
                               ang_vel=bd["state"]["ang_vel"])
    vol = bodies[0]["vol"]
    with open(src, "wb") as f:
        f.write(np.array(vol.shape[::-1], dtype=np.int32).tobytes())
        f.write(np.array(bodies[0]["origin"], dtype=f32).tobytes() + np.array(bodies[0]["step"], dtype=f32).tobytes())
        for bd in bodies:
            p, s = br.api_props(bd["props"]), br.api_state(bd["state"])
            f.write(np.array([p["inv_mass"], *p["inv_inertia"], *p["accel"], p["radius"], p["restitution"]], dtype=f32).tobytes())
            f.write(np.array([*s["quat"], *s["trans"], *s["lin_vel"], *s["ang_vel"]], dtype=f32).tobytes())
        f.write(np.ascontiguousarray(vol, dtype=f32).tobytes())
    run = subprocess.run([exe, src, out, str(N3)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "contact_host_check ok" in run.stdout, run.stdout + run.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    n, m = (int(t) for t in raw[:16].view(np.int64))
    assert n == N3 ** 3 and m == 656
    points = raw[16:16 + 4 * m].view(np.int32)
    rest = raw[16 + 4 * m:]
    assert rest.size == 4 * 2 * (144 + 26 + 1)
    t1, s1, c1, t2, s2, c2 = np.split(rest, np.cumsum([4 * 144, 4 * 26, 4, 4 * 144, 4 * 26]))
    t1, t2 = (a.view(f32).reshape(2, 8, 9) for a in (t1, t2))
    s1, s2 = (a.view(f32).reshape(2, 13) for a in (s1, s2))
    c1, c2 = int(c1.view(np.int32)[0]), int(c2.view(np.int32)[0])
    # the reference
    assert np.array_equal(points, cr.points(vol))
    p = engine.reference_params(N3)
    E = cr.detect(bodies, 3, int(p.walls), tuple(p.box_min[:]), tuple(p.box_max[:]))
    solved = cr.clone(bodies)
    assert cr.solve(solved, E) == c1 >= 2 and _same(t1, E) and _same(s1, cr.state_words(solved))
    # the Python binding on a handle with the same history
    eng = SPHEngine(p, device=0)
    eng.upload("positions", scenes.lattice_positions(N3))  # (sph.Init's lattice; no particle comes near the bodies)
    for b, bd in enumerate(bodies):
        assert eng.add_body(bd["vol"], bd["origin"], bd["step"], br.api_props(bd["props"]), br.api_state(bd["state"])) == b
    assert np.array_equal(eng.contact_points(0)[0], points)
    eng.contact_pass(3, solve=True)
    assert _same(eng.contact_table(), t1) and _same(_states(eng), s1) and eng.get_option("bodies_contacts") == c1
    eng.set_option("bodies_contact", 2)
    eng.wcsph_step(2)
    assert _same(eng.contact_table(), t2) and _same(_states(eng), s2) and eng.get_option("bodies_contacts") == c2
    assert not _same(s2, s1)  # (the steps integrated the poses)
    eng.close()
