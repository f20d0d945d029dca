"""What the collide pass costs a slab rank (tools only, not part of the product).

A MIDDLE rank of the dam-break split along z, emulated on one GPU as tools/slab_periodic_bench.py does it: the rank's two
neighbours are periodic images of the rank itself, the transfer is a device copy, everything else a real middle rank
does per step runs unchanged -- pack, append, ghost sort, ghost densities, the split force pass, and, with a mesh, the
collide pass behind every integrate (the Python protocol of SlabDriver.wcsph_step: band integrate, band collide, band
pack, inner integrate, inner collide, append).  Default: rank 3 of 8 of the 16M scene (n3 = 252: two million particles
and their ghosts), the pillar of tools/collide_bench.py, which crosses that rank's slab, with T = 12 and 3072 triangles,
list walk and cell index, split and unsplit.

In one call, alternating, `--repeats` times over: the step without a mesh, then with each mesh and walk.  Per run one
JSON line: wall-clock ms per step, DSL_K_COLLIDE per launch and launches per step, the hits of the last step.  The
repeats of the same configuration give the call-to-call spread; a last line per split mode sums them up.

  python tools/slab_collide_run.py [--n3 252] [--world 8] [--rank 3] [--steps 30] [--repeats 2]
                                   [--plain-only] [--label this] [--out profiles/slab_collide.jsonl] [--append]

--plain-only: only the step without a mesh.  With DSL_LIB pointing at another build of the library (--label names it)
this is the A/B of the no-mesh step between two builds: alternate the two in one job and compare with the spread."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n3", type=int, default=252)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--subdiv", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    import torch
    import torch.distributed as dist
    from dieselfluid_amd import scenes
    from slab_periodic_bench import PeriodicDriver

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29578")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    torch.cuda.set_stream(torch.cuda.Stream())
    p, _ = scenes.dambreak_scene(a.n3, positions=False)
    radius = 0.5 * float(p.h)
    configs = [(0, 0)]  # (triangles' subdivision or 0: no mesh, index)
    if not a.plain_only:
        configs += [(s, ix) for s in a.subdiv for ix in (0, 1)]
    lines = []

    def emit(rec):
        rec = dict(build=a.label, n3=a.n3, world=a.world, rank=a.rank, **rec)
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def one(overlap, subdiv, index):
        mesh = None
        if subdiv:
            v, n = scenes.box_mesh((0.5, 0.6, 0.5), (0.25, 1.2, 0.25), subdiv)
            mesh = (v, n, radius, 0.0)
        drv = PeriodicDriver.dambreak(a.n3, math_mode=1, device=0, rank=a.rank, world=a.world, overlap=overlap, native=False,
                                      collider=mesh, collide_index=bool(index))
        drv.comm_dev, drv.use_nccl = torch.device("cpu"), False
        PeriodicDriver.REPLAN_EVERY = 10 ** 9  # no host synchronisation inside the timed loop
        eng = drv.engine_core
        drv.wcsph_step(a.warmup)
        eng.timing_reset()
        eng.timing_enable(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        drv.wcsph_step(a.steps)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        eng.timing_enable(False)
        col_ms, launches = eng.timing("collide")
        st = drv.engine.status()
        emit(dict(kind="run", split=bool(drv.overlap), triangles=0 if mesh is None else int(mesh[0].shape[0]), index=index,
                  steps=a.steps, ms_per_step=round(ms, 4), collide_ms_per_launch=round(col_ms, 4),
                  collide_launches_per_step=launches / a.steps, hits_last_step=eng.get_option("collide_hits"),
                  visits_last_step=eng.get_option("collide_visits"), owned=eng.n_owned(), live_with_ghosts=eng.n,
                  force_integrate_ms_per_launch=round(eng.timing("force_integrate")[0], 4),
                  overflow=st[0], margin_missed=st[1]))
        eng.close()
        return ms

    seen = {}
    for _rep in range(a.repeats):
        for overlap in (True, False):
            for subdiv, index in configs:
                seen.setdefault((overlap, subdiv, index), []).append(one(overlap, subdiv, index))
    for overlap in (True, False):
        plain = seen[(overlap, 0, 0)]
        rec = dict(kind="summary", split=overlap, plain_ms_per_step=[round(v, 4) for v in plain],
                   plain_spread_ms=round(max(plain) - min(plain), 4))
        for (ov, subdiv, index), v in seen.items():
            if ov == overlap and subdiv:
                rec[f"added_ms_T{12 * subdiv * subdiv}_index{index}"] = round(sum(v) / len(v) - sum(plain) / len(plain), 4)
        emit(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
