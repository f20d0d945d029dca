#!/usr/bin/env python3
"""What the bodies' contact stage costs a step: tools/bodies_bench.py's scene -- the 16M FAST dam-break of bench.py after 20
steps, icospheres (level 3, radius 0.1) on the dry floor downstream of the block, their distance volumes
dsl_mesh_distance_volume's (the full distance, step dx), built once per handle in the sphere's own frame -- with the spheres
dynamic under gravity, so that they lie on the floor by their contact with it.  For the body counts of `--counts` (1, 4 and
16), DSL_OPT_BODIES_CONTACT = 0 and = 3 alternate in this one process on fresh handles brought to the same state, `--rounds`
rounds of `--steps` timed steps each after a warm-up.  With the option 0 nothing holds the spheres: they go on falling
through the floor (by micrometres in these few steps of this scene's dt), and the line is the bodies' own two launches.

Per run one JSON line: the wall-clock step, DSL_K_COLLIDE per step from device events (two launches per step without the
stage, five with it), the contact points per body, the entries the last solve got past k > 0, the height of body 0.  Only
ratios inside one run count.  Every run (one handle: its warm-up, its bodies, its timed steps) has `--limit` seconds: a
watchdog ends the whole process with exit status 124 when a run overstays, so nothing more is started on a device that may
have hung.  The lines so far are written to `--out` after every run.

  timeout -k 10 900 python tools/contact_bench.py [--n3 252] [--counts 1,4,16] [--limit 120] [--out profiles/contacts_16m.jsonl]
"""
import argparse
import json
import os
import sys
import threading
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
    ap.add_argument("--counts", default="1,4,16")
    ap.add_argument("--limit", type=float, default=120.0, help="seconds one run may take before the process is ended")
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
    half = sphere_r + 6 * dx
    origin = (-half,) * 3
    dims = (int(np.ceil(2 * half / dx)) + 1,) * 3
    nvox = dims[0] * dims[1] * dims[2]
    # sixteen places on the floor (gravity is -y) of the box 4 x 2 x 1, downstream of the block [0, 1]^3, two voxels deep in
    # it: the first solve lifts each sphere until its innermost shell stands on the floor, and every later step meets it there
    places = [(1.3 + 0.32 * (k // 2), sphere_r - 2 * dx, 0.25 + 0.5 * (k % 2)) for k in range(16)]
    mass = 1000.0 * 4.0 / 3.0 * np.pi * sphere_r ** 3  # a sphere of the fluid's density
    props = dict(inv_mass=1.0 / mass, inv_inertia=(1.0 / (0.4 * mass * sphere_r ** 2),) * 3, accel=(0.0, -9.81, 0.0), radius=radius,
                 restitution=0.0)
    lines = []

    def emit(rec):
        rec = {"n_particles": n, "triangles": int(verts.shape[0]), "voxels_per_body": nvox, **rec}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                for r in lines:
                    f.write(json.dumps(r) + "\n")

    def overstayed(what):  # (the watchdog's thread: the run's own thread may be stuck in a device call)
        sys.stderr.write(f"contact_bench: {what} took more than {args.limit} s; ending the process\n")
        sys.stderr.flush()
        os._exit(124)

    for rnd in range(args.rounds):
        for count in (int(c) for c in args.counts.split(",")):
            for option in (0, 3):
                guard = threading.Timer(args.limit, overstayed, (f"bodies{count}_contact{option}, round {rnd}",))
                guard.daemon = True
                guard.start()
                eng = SPHEngine(p, device=0)
                eng.upload("positions", pos)
                eng.reset_forces()
                eng.set_option("skin", 0.0)
                eng.wcsph_step(args.warmup)
                dvol = torch.empty(nvox, dtype=torch.float32, device="cuda")
                eng.mesh_distance_volume(verts, origin, dx, dims, dev_out=dvol.data_ptr())  # (no band: the whole inside is signed)
                eng.sync()
                eng.set_option("bodies_contact", option)
                for k in range(count):
                    eng.add_body(None, origin, dx, props, dict(trans=places[k]), dims=dims, dev_volume=dvol.data_ptr())
                eng.wcsph_step(2)
                eng.timing_enable(1)
                eng.timing_reset()
                eng.sync()
                t0 = time.perf_counter()
                eng.wcsph_step(args.steps)
                eng.sync()
                ms = (time.perf_counter() - t0) * 1e3 / args.steps
                col_ms, launches = eng.timing("collide")
                assert launches == (5 if option else 2) * args.steps, launches
                emit({"config": f"bodies{count}_contact{option}", "bodies": count, "contact": option, "round": rnd,
                      "step_ms": round(ms, 4), "collide_ms_per_step": round(col_ms * launches / args.steps, 4),
                      "launches_per_step": launches // args.steps,
                      "points_per_body": eng.contact_points(0, cap=0)[1] if option else 0,
                      "contacts_last_solve": eng.get_option("bodies_contacts"),
                      "height_of_body_0": float(eng.body_state(0)[0]["trans"][1]), "hits_last_pass": eng.get_option("collide_hits"),
                      "device_bytes": eng.get_option("device_bytes")})
                eng.close()
                guard.cancel()


if __name__ == "__main__":
    main()
