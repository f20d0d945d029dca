"""What moving the slab planes buys and costs (tools only, not part of the product).

The dam-break split along x -- the long axis of the box, where the block fills a quarter of the length -- on several
slab ranks of ONE GPU: the library's own step driver (dsl_slab_wcsph_step) with its transport calls staged through
the host (engine.HostStagedComm), once with dsl_slab_rebalance off and once on, in one call.  Several ranks on one card
share its CUs and pay the host staging for every message: the step times say NOTHING ABOUT SCALING.  What the run shows
is the balance ratio (max owned / mean owned over the ranks: hardware-independent) and what the looks add to a step,
against the same run with every = 0.

  python tools/slab_rebalance_run.py [--world 4] [--n3 64] [--steps 300] [--every 10] [--layers 0,8,16,24,64]
                                     [--out profiles/slab_rebalance.jsonl]

One JSON line per sample (every `every` steps, both runs: the planes in layers and the ranks' owned counts), one per
run (ms per step), one comparing the two."""
import argparse
import json
import os
import pickle
import socket
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, args, every, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from dieselfluid_amd.slab import SlabDriver
    # both runs are set up for moving planes (the same grids, capacities and messages); only `every` differs
    drv = SlabDriver.dambreak(args.n3, math_mode=1, device=0, axis=0, overlap=not args.no_overlap, native=True,
                              layers=args.layers, rebalance_every=every, rebalance_bounds=_default_bounds(args, world))
    core = drv.engine_core
    origin, edge = drv.balance["origin"], drv.balance["edge"]
    samples, spent = [], 0.0

    def sample(step):
        owned = [None] * world
        dist.all_gather_object(owned, core.n_owned())
        planes = [None] * world
        dist.all_gather_object(planes, drv.hi)
        layers = [0] + [int(round((q - origin) / edge)) for q in planes[:-1]] + [drv.balance["n_layers"]]
        samples.append(dict(step=step, planes=layers, owned=owned, max_over_mean=max(owned) * world / sum(owned)))

    sample(0)
    drv.wcsph_step(args.warmup)  # (code objects, message buffers; counted as steps of the run, not timed)
    done = args.warmup
    while done < args.warmup + args.steps:
        k = min(args.every, args.warmup + args.steps - done)
        core.sync()
        dist.barrier()
        t0 = time.perf_counter()
        drv.wcsph_step(k)
        core.sync()
        dist.barrier()
        spent += time.perf_counter() - t0
        done += k
        sample(done)  # (outside the timed window, in both runs)
    looks, moves = core.slab_rebalance_state()[2:] if every else (0, 0)
    st = drv.engine.status()
    if rank == 0:
        with open(out, "wb") as f:
            pickle.dump(dict(samples=samples, ms_per_step=1.0e3 * spent / args.steps, looks=looks, moves=moves,
                             n_layers=drv.balance["n_layers"], overflow=st[0], missed=st[1]), f)
    dist.destroy_process_group()


def _default_bounds(args, world):
    """the bounds SlabDriver.dambreak takes when none are given: anywhere that leaves every slab two layers thick"""
    n_layers = 2 * args.n3 + 2  # box 4 L = 4 n3 dx along x, h = 2 dx, one cell layer of grid beyond each wall
    return ([2 * r for r in range(world + 1)], [n_layers - 2 * (world - r) for r in range(world + 1)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=4)
    ap.add_argument("--n3", type=int, default=64)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--layers", default=None, help="initial split in lattice layers, comma-separated (default: 1/8, 2/8, 3/8 of the block, ...)")
    ap.add_argument("--no-overlap", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slab_rebalance.jsonl"))
    args = ap.parse_args()
    if args.layers is None:  # an unbalanced start: every rank but the last holds an eighth of the block
        step = max(2, (args.n3 // 8) // 2 * 2)
        args.layers = [r * step for r in range(args.world)] + [args.n3]
    else:
        args.layers = [int(v) for v in args.layers.split(",")]
    assert len(args.layers) == args.world + 1
    import torch.multiprocessing as mp
    runs = {}
    for name, every in (("off", 0), ("on", args.every)):
        out = os.path.join(tempfile.mkdtemp(prefix="dsl_rebalance_run_"), "run.pkl")
        mp.spawn(_worker, args=(args.world, _free_port(), args, every, out), nprocs=args.world, join=True)
        with open(out, "rb") as f:
            runs[name] = pickle.load(f)
        os.remove(out)
    base = dict(world=args.world, n3=args.n3, particles=args.n3 ** 3, axis="x", overlap=not args.no_overlap,
                transport="HostStagedComm, all ranks on one GPU: step times say nothing about scaling")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for name in ("off", "on"):
            r = runs[name]
            for s in r["samples"]:
                f.write(json.dumps(dict(kind="sample", run=name, **s)) + "\n")
            f.write(json.dumps(dict(kind="run", run=name, every=0 if name == "off" else args.every, steps=args.steps,
                                    warmup=args.warmup, ms_per_step=round(r["ms_per_step"], 4), looks=r["looks"],
                                    plane_moves=r["moves"], n_layers=r["n_layers"], overflow=r["overflow"],
                                    margin_missed=r["missed"], first_max_over_mean=r["samples"][0]["max_over_mean"],
                                    last_max_over_mean=r["samples"][-1]["max_over_mean"], **base)) + "\n")
        on, off = runs["on"], runs["off"]
        line = dict(kind="compare", ms_per_step_off=round(off["ms_per_step"], 4), ms_per_step_on=round(on["ms_per_step"], 4),
                    added_ms_per_step=round(on["ms_per_step"] - off["ms_per_step"], 4), every=args.every,
                    last_max_over_mean_off=off["samples"][-1]["max_over_mean"],
                    last_max_over_mean_on=on["samples"][-1]["max_over_mean"], **base)
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
