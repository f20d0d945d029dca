#!/usr/bin/env python3
"""What a field volume costs: dsl_field_volume of the densities over the wall box of bench.py's 16M DSL_MATH_FAST dam-break
after 20 steps, at step = dx (1008 x 504 x 252 = 128M voxels, 512 MB) and at step = h = 2 dx (16M voxels), written to
device memory (dev_out), in both kernel forms.

Per lattice one JSON line.  After one warm-up call per form, forms 0 (per-voxel sweep) and 1 (LDS bricks) ALTERNATE in this
one process on one handle; every call is timed by DSL_K_VOLUME's device events (reset, one call, read).  Recorded per form:
the calls' ms (mean, min, max, standard deviation, the list), the voxels, the bricks that swept out of LDS / fell back to
the global sweep / were empty, the records the LDS bricks staged, the algorithmic bytes -- 4 per voxel written plus 20 per
staged record -- and the GB/s they give; whether the two forms' volumes are the same bits; and first, for scale, the plain
step's wall-clock ms on the same scene.

  python tools/volume_bench.py [--n3 252] [--calls 10] [--out profiles/volume_16m.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECORD_BYTES = 20  # (x, y, z, m / rho_j) and f_j


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n3", type=int, default=252)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from dieselfluid_amd import SPHEngine, scenes

    p, pos = scenes.dambreak_scene(args.n3)  # DSL_MATH_FAST, h = 2 dx
    n = args.n3 ** 3
    dx = 1.0 / args.n3
    lines = []

    def emit(rec):
        rec = {"n_particles": n, **rec}
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.reset_forces()
    eng.wcsph_step(10)
    eng.sync()
    t0 = time.perf_counter()
    eng.wcsph_step(10)
    eng.sync()
    emit({"config": "plain step, default skin", "step_ms": round((time.perf_counter() - t0) * 1e3 / 10, 4),
          "steps_before_the_volumes": 20, "skin_steps": eng.get_option("skin_steps")})

    box = [float(p.box_max[a]) for a in range(3)]
    eng.timing_enable(1)
    for label, step in (("step = dx", dx), ("step = h", float(p.h))):
        dims = [int(round(box[a] / step)) for a in range(3)]
        origin = [0.5 * step] * 3  # voxel centres tile the wall box
        nvox = dims[0] * dims[1] * dims[2]
        out = [torch.empty(nvox, dtype=torch.float32, device="cuda") for _ in range(2)]
        ms = {0: [], 1: []}
        counts = {}
        for rep in range(args.calls + 1):  # (rep 0: the warm-up call of each form -- the first one also sorts)
            for form in (0, 1):
                eng.set_option("volume_bricks", form)
                eng.timing_reset()
                eng.field_volume(origin, step, dims, "densities", dev_out=out[form].data_ptr())
                t, launches = eng.timing("volume")
                assert launches == 1
                if rep > 0:
                    ms[form].append(t)
                counts[form] = {k: int(eng.get_option("volume_" + k)) for k in ("lds_bricks", "fallback_bricks", "empty_bricks",
                                                                                "staged_records")}
        same = bool(torch.equal(out[0].view(torch.int32), out[1].view(torch.int32)))
        nonzero = int(torch.count_nonzero(out[0]).item())
        forms = []
        for form in (0, 1):
            staged = counts[form]["staged_records"]
            nbytes = 4 * nvox + RECORD_BYTES * staged
            mean = statistics.fmean(ms[form])
            forms.append({"volume_bricks": form, "ms_mean": round(mean, 4), "ms_min": round(min(ms[form]), 4),
                          "ms_max": round(max(ms[form]), 4), "ms_stdev": round(statistics.pstdev(ms[form]), 4),
                          "ms": [round(t, 4) for t in ms[form]], **counts[form], "algorithmic_bytes": nbytes,
                          "algorithmic_gb_per_s": round(nbytes / (mean * 1e-3) / 1e9, 2)})
        emit({"config": label, "scalar": "densities", "origin": origin, "step": step, "dims": dims, "voxels": nvox,
              "nonzero_voxels": nonzero, "bricks": ((dims[0] + 7) // 8) * ((dims[1] + 7) // 8) * ((dims[2] + 3) // 4),
              "timed_calls_per_form": args.calls, "forms_same_bits": same, "forms": forms})
        del out
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
