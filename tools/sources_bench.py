#!/usr/bin/env python3
"""What sources and sinks cost a step: the 16M FAST dam-break of bench.py (n3 = 252), in configurations that alternate inside
one call, `--rounds` times, each run in a fresh child process under its own time limit (`--limit` seconds; a child that
overstays is killed and the whole call ends with exit status 124, so nothing more is started on a device that may have hung):

  plain          the step as bench.py runs it (the library's default skin step); no new call is made
  plain_noskin   DSL_OPT_SKIN = 0: sort and sweep every step -- what a handle with an emitter or a sink steps with, since
                 the skin step is not taken while one exists; the base line of the three configurations below
  sink_every8    one sink that catches nothing, DSL_OPT_SINK_EVERY = 8 (the default): a look every eighth step
  sink_every1    the same sink, a look every step: per launch, DSL_K_SOURCES is then the count kernel alone
  tap            a 64 x 64 emitter of period 4 above the column, its layers dx apart, and an outlet box in the stream, as
                 deep as the stream travels between two looks, which removes about as much as the face emits; afterwards
                 one dsl_particles_remove that catches part of the column: a look and a full compaction at 16M
  parent         `--parent-lib`: the plain step of another build of the library (the parent commit's), loaded through DSL_LIB

Per run one JSON line: ms per step by the wall clock over `--steps` steps in calls of 8 (no events recorded), then from a
16-step segment with events DSL_K_SOURCES per launch and its launches, the particle count after every 8 steps, and for `tap`
the launches, the device milliseconds and the wall-clock milliseconds of the one explicit removal.  Only ratios inside one
call count.  The lines so far are written to `--out` after every run.

  timeout -k 10 1100 python tools/sources_bench.py [--n3 252] [--parent-lib PATH] [--out profiles/sources_16m.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("plain", "plain_noskin", "sink_every8", "sink_every1", "tap", "parent")
NEW_CALLS = ("dsl_particles_append", "dsl_emitter_add", "dsl_emitters_clear", "dsl_emit", "dsl_sink_add", "dsl_sinks_clear",
             "dsl_particles_remove")
INF = float("inf")


def child(args):
    from dieselfluid_amd import _lib
    if args.child == "parent":  # (a build from before these calls existed: bind what it has)
        for name in NEW_CALLS:
            _lib.EXPORTS.pop(name, None)
    from dieselfluid_amd import SPHEngine, scenes
    n3 = args.n3
    n = n3 ** 3
    dx = 1.0 / n3
    p, pos = scenes.dambreak_scene(n3)
    room = 1 << 20 if args.child == "tap" else 0
    if room:
        p.capacity = n + room
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.reset_forces()
    del pos
    new = args.child not in ("plain", "parent")
    if args.child != "plain" and args.child != "parent":
        eng.set_option("skin", 0.0)
    if args.child.startswith("sink_every"):
        eng.set_option("sink_every", int(args.child[len("sink_every"):]))
        eng.add_sink((10.0, 10.0, 10.0), (11.0, 11.0, 11.0))  # (outside the box: it never catches anything)
    if args.child == "tap":
        period, every = 4, 8
        speed = dx / (period * float(p.dt))  # the layers come out dx apart
        eng.add_emitter(origin=(0.3, 1.6, 0.3), u=(dx, 0.0, 0.0), v=(0.0, 0.0, dx), nu=64, nv=64, velocity=(0.0, -speed, 0.0),
                        period=period)
        depth = every * float(p.dt) * speed  # what the stream travels between two looks
        top = 1.6 - 2.0 * dx  # (two layers under the face: the stream is there after 8 steps)
        eng.add_sink((0.25, top - depth, 0.25), (0.3 + 64 * dx + 0.05, top, 0.3 + 64 * dx + 0.05))
    eng.wcsph_step(args.warmup)
    eng.sync()
    counts = []
    t0 = time.perf_counter()
    for _ in range(args.steps // 8):
        eng.wcsph_step(8)
        counts.append(eng.n)
    eng.sync()
    ms = (time.perf_counter() - t0) * 1e3 / (8 * (args.steps // 8))
    rec = {"config": args.child, "n_particles": n, "capacity": n + room, "steps": 8 * (args.steps // 8), "warmup": args.warmup,
           "step_ms": round(ms, 4), "count_every_8_steps": counts, "library": "DSL_LIB" if os.environ.get("DSL_LIB") else "built"}
    eng.timing_enable(1)
    eng.timing_reset()
    eng.wcsph_step(16)
    eng.sync()
    rec["density_ms"] = round(eng.timing("density")[0], 4)
    if new:
        src_ms, launches = eng.timing("sources")
        rec.update({"sources_ms_per_launch": round(src_ms, 5), "sources_launches_in_16_steps": launches,
                    "emitted": eng.get_option("emitted"), "removed": eng.get_option("removed"),
                    "emit_skipped": eng.get_option("emit_skipped"), "skin_steps": eng.get_option("skin_steps")})
    if args.child == "tap":
        # one explicit removal that has work to do: the column's first 20 lattice layers in x (about 8 % of the particles)
        eng.clear_emitters()
        eng.clear_sinks()
        eng.add_sink((-INF, -INF, -INF), (20.0 * dx, INF, INF))
        eng.timing_reset()
        eng.sync()
        before = eng.n
        t0 = time.perf_counter()
        gone = eng.remove_particles()
        wall = (time.perf_counter() - t0) * 1e3
        src_ms, launches = eng.timing("sources")
        rec.update({"removal": {"n_before": before, "removed": gone, "launches": launches,
                                "device_ms_all_launches": round(src_ms * launches, 4), "wall_ms": round(wall, 4)}})
        eng.clear_sinks()
        eng.wcsph_step(2)  # (the handle steps on)
        eng.sync()
    rec["device_bytes"] = eng.get_option("device_bytes")
    eng.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n3", type=int, default=252)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=float, default=150.0, help="seconds one run may take before the call is ended")
    ap.add_argument("--parent-lib", default=None, help="libdslsph.so of the parent commit, for the `parent` configuration")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=CONFIGS, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = []
    for rnd in range(args.rounds):
        for config in CONFIGS:
            if config == "parent" and not args.parent_lib:
                continue
            env = dict(os.environ)
            if config == "parent":
                env["DSL_LIB"] = os.path.abspath(args.parent_lib)
            else:
                env.pop("DSL_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", config, "--n3", str(args.n3), "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            try:
                run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                sys.stderr.write(f"sources_bench: {config}, round {rnd}, took more than {args.limit} s; ending the call\n")
                return 124
            if run.returncode != 0:  # (a fault or an abort: nothing more is started)
                sys.stderr.write(f"sources_bench: {config}, round {rnd}, ended with status {run.returncode}\n{run.stdout}{run.stderr}")
                return run.returncode if run.returncode > 0 else 1
            rec = json.loads(run.stdout.strip().splitlines()[-1])
            rec["round"] = rnd
            lines.append(rec)
            print(json.dumps(rec), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    for r in lines:
                        f.write(json.dumps(r) + "\n")
    # the spread between the repeats of a configuration, and every configuration against its base line
    by = {}
    for r in lines:
        by.setdefault(r["config"], []).append(r["step_ms"])
    for config, v in by.items():
        print(f"# {config}: step_ms {v}, spread {100.0 * (max(v) - min(v)) / min(v):.2f} %", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
