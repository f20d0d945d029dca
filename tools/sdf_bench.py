#!/usr/bin/env python3
"""What an implicit collider costs next to the explicit one: the 16M FAST dam-break of bench.py after 20 steps with an
icosphere of level 5 (20,480 triangles) standing in the flow.  Three steps alternate in this one process, ten timed steps
each after a warm-up, every one on a fresh handle brought to the same state:

  plain    no collider (DSL_OPT_SKIN = 0: the step a handle with a collider runs -- no skin step is taken with either kind)
  index    the mesh collider over the cell index (DSL_OPT_COLLIDE_INDEX = 1): the numbers of profiles/collide_index_16m.jsonl,
           measured again here
  volume   the volume collider over a lattice of step dx around the sphere's box (dsl_mesh_distance_volume's output, band 4 dx)

Per run one JSON line: the wall-clock step, DSL_K_COLLIDE per launch (device events), the particles the last pass moved.
Then the volume build itself on that lattice, band = 4 dx and band = +inf, ten timed calls each after a warm-up: DSL_K_SDF
summed over the call's launches, the distance and sign phases, the bricks with a list and the triangle visits.

  python tools/sdf_bench.py [--n3 252] [--out profiles/sdf_16m.jsonl]

--rigid: what a pose costs.  Two steps alternate instead, on fresh handles in this one process:

  volume   as above: the static pass, k_collide_volume
  rigid    the same volume with a motion set (dsl_collider_volume_motion): the sphere turned about its own centre, so that it
           stands where the static one stands, with a linear and an angular velocity -- k_collide_volume_rigid and the fold of
           its partial sums, two launches per step under DSL_K_COLLIDE (collide_ms_per_step is their sum)

  python tools/sdf_bench.py --rigid [--n3 252] [--out profiles/sdf_rigid_16m.jsonl]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n3", type=int, default=252)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--level", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rigid", action="store_true", help="the static volume pass against the pass in rigid motion")
    args = ap.parse_args()
    import numpy as np
    import torch
    from dieselfluid_amd import SPHEngine, scenes

    p, pos = scenes.dambreak_scene(args.n3)
    n = args.n3 ** 3
    dx = 1.0 / args.n3
    radius = 0.5 * float(p.h)
    center, sphere_r = (0.5, 0.4, 0.5), 0.3
    verts, normals = scenes.icosphere_mesh(center, sphere_r, args.level)
    band = 4 * dx
    # the sphere's box, a band and a cell more on every side
    origin = tuple(float(c - sphere_r - band - 2 * dx) for c in center)
    dims = (int(np.ceil((2 * (sphere_r + band + 2 * dx)) / dx)) + 1,) * 3
    nvox = dims[0] * dims[1] * dims[2]
    lines = []

    def emit(rec):
        rec = {"n_particles": n, "triangles": int(verts.shape[0]), **rec}
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def fresh():
        eng = SPHEngine(p, device=0)
        eng.upload("positions", pos)
        eng.reset_forces()
        eng.set_option("skin", 0.0)
        eng.wcsph_step(args.warmup)
        return eng

    def timed_steps(eng):
        eng.wcsph_step(2)
        eng.timing_enable(1)
        eng.timing_reset()
        eng.sync()
        t0 = time.perf_counter()
        eng.wcsph_step(args.steps)
        eng.sync()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        col_ms, launches = eng.timing("collide")
        return ms, col_ms, launches

    def rigid_pose():
        """0.7 rad about (1, 2, 3) through the sphere's centre: x = R (xl - c) + c"""
        a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = (np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)).astype(np.float32)
        c = np.array(center)
        return dict(rot=R, trans=c - R.astype(np.float64) @ c, lin_vel=(0.3, -0.2, 0.1), ang_vel=(0.5, -1.0, 0.8))

    for rnd in range(args.rounds):
        for kind in (("volume", "rigid") if args.rigid else ("plain", "index", "volume")):
            eng = fresh()
            extra = {}
            if kind == "index":
                eng.set_option("collide_index", 1)
                eng.set_collider_mesh(verts, normals, radius, 0.0)
            elif kind in ("volume", "rigid"):
                dvol = torch.empty(nvox, dtype=torch.float32, device="cuda")
                eng.sync()
                t0 = time.perf_counter()
                eng.mesh_distance_volume(verts, origin, dx, dims, band=band, dev_out=dvol.data_ptr())
                eng.set_collider_volume(None, origin, dx, dims=dims, radius=radius, restitution=0.0, dev_volume=dvol.data_ptr())
                extra = {"build_and_set_ms": round((time.perf_counter() - t0) * 1e3, 3), "dims": list(dims), "voxels": nvox,
                         "volume_bytes": 4 * nvox}
                if kind == "rigid":
                    eng.set_collider_volume_motion(**rigid_pose())
            ms, col_ms, launches = timed_steps(eng)
            per_step = {"plain": 0, "rigid": 2}.get(kind, 1)  # (the rigid pass and its fold)
            assert launches == per_step * args.steps
            rec = {"config": kind, "round": rnd, "step_ms": round(ms, 4), "collide_ms_per_launch": round(col_ms, 4),
                   "hits_last_pass": eng.get_option("collide_hits"), **extra}
            if args.rigid:
                rec["collide_ms_per_step"] = round(col_ms * per_step, 4)
            if kind == "rigid":
                imp, trq = eng.collider_volume_impulse()
                rec["impulse"], rec["torque"] = [float(v) for v in imp], [float(v) for v in trq]
            if kind == "index":
                rec["visits_last_pass"] = eng.get_option("collide_visits")
            emit(rec)
            eng.close()

    if args.rigid:
        if args.out:
            with open(args.out, "w") as f:
                for rec in lines:
                    f.write(json.dumps(rec) + "\n")
        return

    # the build alone
    eng = fresh()
    dvol = torch.empty(nvox, dtype=torch.float32, device="cuda")
    eng.timing_enable(1)
    for label, b in (("band 4 dx", band), ("band +inf", float("inf"))):
        runs = []
        for k in range(1 + 10):
            eng.timing_reset()
            eng.sync()
            t0 = time.perf_counter()
            eng.mesh_distance_volume(verts, origin, dx, dims, band=b, dev_out=dvol.data_ptr())
            eng.sync()
            wall = (time.perf_counter() - t0) * 1e3
            ms, launches = eng.timing("sdf")
            if k:  # (the first call allocates)
                runs.append({"wall_ms": round(wall, 4), "kernels_ms": round(ms * launches, 4), "launches": launches,
                             "distance_ms": round(eng.get_option("sdf_distance_ms"), 4), "sign_ms": round(eng.get_option("sdf_sign_ms"), 4)})
        emit({"config": "build, " + label, "dims": list(dims), "voxels": nvox, "active_bricks": eng.get_option("sdf_active_bricks"),
              "visits": eng.get_option("sdf_visits"), "device_bytes": eng.get_option("device_bytes"), "runs": runs})
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
