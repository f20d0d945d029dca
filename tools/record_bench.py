#!/usr/bin/env python3
"""What the frame recorder costs a run: the 16M FAST dam-break of bench.py (n3 = 252), in configurations that alternate inside
one call, `--rounds` times, each run in a fresh child process under its own time limit (`--limit` seconds; a child that
overstays is killed and the whole call ends with exit status 124, so nothing more is started on a device that may have hung):

  off            no recorder: the step as bench.py runs it (the library's default skin step); no new call is made
  q16_every8     Q16 positions (96 MB a frame at 16M), a frame every 8th step
  f32_all_every8 float32 positions, velocities and densities (448 MB a frame), a frame every 8th step
  q16_every1     Q16 positions, a frame every step
  parent         `--parent-lib`: the step of another build of the library (the parent commit's), loaded through DSL_LIB

The host steps in calls of 8 and, behind each call, reads every frame that call recorded (peek waits for that frame's copy
only; the steps already queued run on), so no frame is dropped and the skin episode is never settled.  Per run one JSON line:
ms per step by the wall clock over `--steps` steps (no events recorded), frames recorded and dropped, the skin steps, and from
a 16-step segment with events DSL_OPT_RECORD_PACK_MS and DSL_OPT_RECORD_COPY_MS of its last frame and the copy's GB/s.  Only
ratios inside one call count; a configuration's cost per frame is (its step_ms - off's) * every.  The lines so far are written
to `--out` after every run.

  timeout -k 10 1100 python tools/record_bench.py [--n3 252] [--parent-lib PATH] [--out profiles/record_16m.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# config -> recorder_spec's arguments (None: no recorder)
CONFIGS = {
    "off": None,
    "q16_every8": dict(every=8, encoding="q16", slots=2),
    "f32_all_every8": dict(every=8, fields=("velocities", "densities"), slots=2),
    "q16_every1": dict(every=1, encoding="q16", slots=8),
    "parent": None,
}
NEW_CALLS = ("dsl_recorder_set", "dsl_record_frame_bytes", "dsl_record_now", "dsl_record_poll", "dsl_record_peek",
             "dsl_record_release", "dsl_record_read")


def child(args):
    from dieselfluid_amd import _lib
    if args.child == "parent":  # (a build from before these calls existed: bind what it has)
        for name in NEW_CALLS:
            _lib.EXPORTS.pop(name, None)
    from dieselfluid_amd import SPHEngine, scenes
    n3 = args.n3
    p, pos = scenes.dambreak_scene(n3)
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.reset_forces()
    del pos
    kw = CONFIGS[args.child]
    eng.wcsph_step(args.warmup)
    eng.sync()
    frame_bytes = 0
    if kw:
        spec = eng.set_recorder(first_step=args.warmup, **kw)
        frame_bytes = eng.record_frame_bytes(spec, n3 ** 3)

    def drain():
        got = 0
        while kw and eng.record_poll()[0] > drain.read:
            eng.peek_frame()
            eng.release_frame()
            drain.read += 1
            got += 1
        return got
    drain.read = 0

    calls = args.steps // 8
    t0 = time.perf_counter()
    for _ in range(calls):
        eng.wcsph_step(8)
        drain()
    eng.sync()
    ms = (time.perf_counter() - t0) * 1e3 / (8 * calls)
    rec = {"config": args.child, "n_particles": n3 ** 3, "steps": 8 * calls, "warmup": args.warmup, "step_ms": round(ms, 4),
           "library": "DSL_LIB" if os.environ.get("DSL_LIB") else "built", "skin_steps": eng.get_option("skin_steps"),
           "skin_rebuilds": eng.get_option("skin_rebuilds")}
    if kw:
        recorded, _, dropped = eng.record_poll()
        rec.update({"every": kw["every"], "frame_bytes": frame_bytes, "frames": recorded, "dropped": dropped})
        eng.timing_enable(1)
        for _ in range(2):
            eng.wcsph_step(8)
            drain()
        rec["pack_ms"] = round(eng.get_option("record_pack_ms"), 4)
        rec["copy_ms"] = round(eng.get_option("record_copy_ms"), 4)
        rec["copy_gb_per_s"] = round(frame_bytes / (rec["copy_ms"] * 1e6), 2) if rec["copy_ms"] > 0 else None
        eng.timing_enable(0)
        eng.set_recorder(None)
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
    ap.add_argument("--child", choices=tuple(CONFIGS), default=None, help=argparse.SUPPRESS)
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
                sys.stderr.write(f"record_bench: {config}, round {rnd}, took more than {args.limit} s; ending the call\n")
                return 124
            if run.returncode != 0:  # (a fault or an abort: nothing more is started)
                sys.stderr.write(f"record_bench: {config}, round {rnd}, ended with status {run.returncode}\n{run.stdout}{run.stderr}")
                return run.returncode if run.returncode > 0 else 1
            rec = json.loads(run.stdout.strip().splitlines()[-1])
            rec["round"] = rnd
            lines.append(rec)
            print(json.dumps(rec), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    for r in lines:
                        f.write(json.dumps(r) + "\n")
    # the spread between the repeats of a configuration, and every configuration's cost per frame against `off`
    by = {}
    for r in lines:
        by.setdefault(r["config"], []).append(r)
    off = min(r["step_ms"] for r in by["off"]) if "off" in by else None
    for config, rs in by.items():
        v = [r["step_ms"] for r in rs]
        note = f"# {config}: step_ms {v}, spread {100.0 * (max(v) - min(v)) / min(v):.2f} %"
        if off is not None and rs[0].get("every"):
            note += f", per frame {(min(v) - off) * rs[0]['every']:.3f} ms over off"
        print(note, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
