#!/usr/bin/env python3
"""What a triangle-mesh collider costs: the 16M dam-break of bench.py with a box_mesh pillar standing in the fluid block,
T = 12, 192 and 3072 triangles, broad phase on (DSL_OPT_COLLIDE_CULL = 1) and off.

Per configuration one JSON line: DSL_K_COLLIDE's device time per launch (HIP events around the launch), the particles
the last pass moved, and the wall-clock step next to it; first the plain step without a mesh -- with the skin step the
bench's default takes, and without it (DSL_OPT_SKIN = 0), which is the step a handle with a mesh runs: the skin step is
not taken while a mesh is set.  Without the cull the pass tests N * T pairs.

  python tools/collide_bench.py [--n3 252] [--steps 20] [--out profiles/collide_16m.jsonl]

--index: the cell index over the triangles (DSL_OPT_COLLIDE_INDEX) against the list walk instead.  The pillars again, an
icosphere of 20,480 triangles standing in the block, and a concave case with the fluid inside the mesh -- an open box of
five quad_mesh faces around the block, 2,560 triangles.  Per configuration one JSON line with four runs, index 0, 1, 0, 1,
each on a fresh handle in this one process (the same GPU: the spread of the repeats is the noise): DSL_K_COLLIDE per
launch, the wall-clock step, the visits of the last pass, the index's cells, entries and edge, and what the blocking
dsl_collider_set_mesh took with the build in it.

  python tools/collide_bench.py --index [--out profiles/collide_index_16m.jsonl]
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--subdiv", type=int, nargs="*", default=[1, 4, 16])
    ap.add_argument("--out", default=None)
    ap.add_argument("--index", action="store_true")
    args = ap.parse_args()
    import numpy as np
    from dieselfluid_amd import SPHEngine, scenes

    p, pos = scenes.dambreak_scene(args.n3)
    n = args.n3 ** 3
    lines = []

    def emit(rec):
        rec = {"n_particles": n, **rec}
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def timed_steps(eng, steps):
        eng.sync()
        t0 = time.perf_counter()
        eng.wcsph_step(steps)
        eng.sync()
        return (time.perf_counter() - t0) * 1e3 / steps

    def fresh(skin):
        eng = SPHEngine(p, device=0)
        eng.upload("positions", pos)
        eng.reset_forces()
        if skin is not None:
            eng.set_option("skin", skin)
        return eng

    radius = 0.5 * float(p.h)

    def index_runs():
        half = 0.52  # the open box: faces 0.02 outside the block [0, 1]^3 (and the wall box), no lid
        c = [(0.5 + sx * half, 0.5 + sy * half, 0.5 + sz * half) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
        faces = [((0, 1, 3, 2), (1, 0, 0)), ((4, 5, 7, 6), (-1, 0, 0)), ((0, 1, 5, 4), (0, 1, 0)), ((0, 2, 6, 4), (0, 0, 1)),
                 ((1, 3, 7, 5), (0, 0, -1))]
        quads = [scenes.quad_mesh(*(c[k] for k in corners), nrm, 16) for corners, nrm in faces]
        configs = [("pillar in the fluid", scenes.box_mesh((0.5, 0.6, 0.5), (0.25, 1.2, 0.25), s)) for s in args.subdiv]
        configs.append(("icosphere in the fluid", scenes.icosphere_mesh((0.5, 0.4, 0.5), 0.3, 5)))
        configs.append(("open box around the fluid", (np.concatenate([q[0] for q in quads]), np.concatenate([q[1] for q in quads]))))
        for label, (verts, normals) in configs:
            runs = []
            for index in (0, 1, 0, 1):
                eng = fresh(None)
                eng.wcsph_step(args.warmup)
                eng.set_option("collide_index", index)
                eng.sync()
                t0 = time.perf_counter()
                eng.set_collider_mesh(verts, normals, radius, 0.0)
                set_mesh_ms = (time.perf_counter() - t0) * 1e3
                eng.wcsph_step(2)
                eng.timing_enable(1)
                eng.timing_reset()
                ms = timed_steps(eng, args.steps)
                col_ms, launches = eng.timing("collide")
                assert launches == args.steps
                runs.append({"index": index, "collide_ms_per_launch": round(col_ms, 4), "step_ms": round(ms, 4),
                             "visits_last_pass": eng.get_option("collide_visits"),
                             "full_waves_last_pass": eng.get_option("collide_full_waves"),
                             "hits_last_pass": eng.get_option("collide_hits"),
                             "cells": eng.get_option("collide_index_cells"), "entries": eng.get_option("collide_index_entries"),
                             "edge": eng.get_option("collide_index_edge"), "set_mesh_ms": round(set_mesh_ms, 3)})
                eng.close()
            emit({"config": label, "triangles": int(verts.shape[0]), "radius": radius, "steps": args.steps, "cull": 1,
                  "waves": (n + 63) // 64, "runs": runs})

    if args.index:
        index_runs()
        if args.out:
            with open(args.out, "w") as f:
                for rec in lines:
                    f.write(json.dumps(rec) + "\n")
        return

    for label, skin in (("plain step, default skin", None), ("plain step, skin 0", 0.0)):
        eng = fresh(skin)
        eng.wcsph_step(args.warmup)
        eng.timing_enable(1)
        eng.timing_reset()
        ms = timed_steps(eng, args.steps)
        assert eng.timing("collide")[1] == 0  # no mesh: no collide kernel
        emit({"config": label, "triangles": 0, "step_ms": round(ms, 4), "skin_steps": eng.get_option("skin_steps"),
              "density_ms": round(eng.timing("density")[0], 4), "force_integrate_ms": round(eng.timing("force_integrate")[0], 4)})
        eng.close()

    # a pillar inside the fluid block [0, 1]^3, floor to above the surface; query radius h / 2
    for subdiv in args.subdiv:
        verts, normals = scenes.box_mesh((0.5, 0.6, 0.5), (0.25, 1.2, 0.25), subdiv)
        for cull in (1, 0):
            eng = fresh(None)
            eng.wcsph_step(args.warmup)
            eng.set_collider_mesh(verts, normals, radius, 0.0)
            eng.set_option("collide_cull", cull)
            eng.wcsph_step(2)
            skin_before = eng.get_option("skin_steps")  # (the warm-up without a mesh took skin steps)
            eng.timing_enable(1)
            eng.timing_reset()
            pairs = n * verts.shape[0]
            steps = args.steps if (cull or pairs < 4e9) else max(2, min(args.steps, int(2e11 / pairs)))
            ms = timed_steps(eng, steps)
            col_ms, launches = eng.timing("collide")
            assert launches == steps and eng.get_option("skin_steps") == skin_before  # no skin step with a mesh
            emit({"config": "pillar in the fluid", "triangles": int(verts.shape[0]), "cull": cull, "radius": radius,
                  "steps": steps, "collide_ms_per_launch": round(col_ms, 4), "step_ms": round(ms, 4),
                  "pair_tests_without_cull": pairs, "hits_last_pass": eng.get_option("collide_hits"),
                  "density_ms": round(eng.timing("density")[0], 4),
                  "force_integrate_ms": round(eng.timing("force_integrate")[0], 4)})
            eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
