#!/usr/bin/env python3
"""What rigid bodies cost a step: the 16M FAST dam-break of bench.py after 20 steps with icospheres (level 3, radius 0.1)
standing on the dry floor downstream of the block -- not inside it: DESIGN 4.6 records that a sphere inside the block makes
this scene's step a thousand times slower.  Their distance volumes are dsl_mesh_distance_volume's (band 4 dx, step dx), built
once per handle in the sphere's own frame.  Five steps alternate in this one process, on fresh handles brought to the same
state, `--rounds` rounds of `--steps` timed steps each after a warm-up:

  plain     no collider (DSL_OPT_SKIN = 0: the step a handle with a collider runs)
  rigid     the single volume collider with a motion set (dsl_collider_volume_motion): the parent's code, the baseline
  bodies1   one body (dsl_body_add) where the baseline's sphere stands
  bodies4   four bodies
  bodies16  sixteen bodies

Per run one JSON line: the wall-clock step, DSL_K_COLLIDE per step from device events (two launches per step for every
collider line), the (particle, body) pairs the last pass moved.  Only ratios inside one run count.

  python tools/bodies_bench.py [--n3 252] [--out profiles/bodies_16m.jsonl]
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
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from dieselfluid_amd import SPHEngine, scenes

    p, pos = scenes.dambreak_scene(args.n3)
    n = args.n3 ** 3
    dx = 1.0 / args.n3
    radius = 0.5 * float(p.h)
    sphere_r = 0.1
    verts, _normals = scenes.icosphere_mesh((0.0, 0.0, 0.0), sphere_r, args.level)  # in the body's frame: its centre is the origin
    band = 4 * dx
    half = sphere_r + band + 2 * dx
    origin = (-half,) * 3
    dims = (int(np.ceil(2 * half / dx)) + 1,) * 3
    nvox = dims[0] * dims[1] * dims[2]
    # sixteen places on the floor (gravity is -y) of the box 4 x 2 x 1, downstream of the block [0, 1]^3
    places = [(1.3 + 0.32 * (k // 2), sphere_r + radius, 0.25 + 0.5 * (k % 2)) for k in range(16)]
    lines = []

    def emit(rec):
        rec = {"n_particles": n, "triangles": int(verts.shape[0]), "voxels_per_body": nvox, **rec}
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

    for rnd in range(args.rounds):
        for kind, count in (("plain", 0), ("rigid", 1), ("bodies1", 1), ("bodies4", 4), ("bodies16", 16)):
            eng = fresh()
            if count:
                dvol = torch.empty(nvox, dtype=torch.float32, device="cuda")
                eng.mesh_distance_volume(verts, origin, dx, dims, band=band, dev_out=dvol.data_ptr())
                eng.sync()
            if kind == "rigid":
                eng.set_collider_volume(None, origin, dx, dims=dims, radius=radius, restitution=0.0, dev_volume=dvol.data_ptr())
                eng.set_collider_volume_motion(trans=places[0])
            elif count:
                for k in range(count):
                    eng.add_body(None, origin, dx, dict(radius=radius, restitution=0.0), dict(trans=places[k]), dims=dims,
                                 dev_volume=dvol.data_ptr())
            ms, col_ms, launches = timed_steps(eng)
            assert launches == (2 if count else 0) * args.steps
            emit({"config": kind, "bodies": count if kind != "rigid" else 0, "round": rnd, "step_ms": round(ms, 4),
                  "collide_ms_per_step": round(col_ms * 2, 4) if count else 0.0, "hits_last_pass": eng.get_option("collide_hits"),
                  "device_bytes": eng.get_option("device_bytes")})
            eng.close()

    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
