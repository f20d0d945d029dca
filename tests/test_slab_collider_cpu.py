"""A collider mesh on slab ranks, on the CPU: gloo ranks drive SlabDriver's Python protocol with the oracle-backed engine
(oracle_slab_collider_engine.py: collide() = collider_ref.respond on the finite rows) through
SlabDriver.dambreak(..., collider=...), and the result is compared with the single-domain oracle that applies `respond`
after every step.  What is exercised: the driver collides after the integrate and BEFORE the pack, so that a particle
the response sets back across a plane stays with its rank, every particle is collided by exactly one rank, and the
ghosts (NaN after the integrate) are not.

Scenes A and B of slab_collider_scenes.py.  A collision is a classification: the ranks sum a particle's neighbours in
another order than the single domain, so a particle within rounding of the mesh could hit on one side and miss on the
other.  These scenes do not: the per-step sets of moved particle ids are EQUAL, which is what makes the float32 tolerances
of tests/test_slab_cpu.py (2e-6, 2e-5) apply to the state."""
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import collider_ref
import helpers
import slab_collider_scenes as sc
from oracle import pyoracle as po
from test_slab_cpu import _free_port


def _worker(rank, world, port, name, out):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dieselfluid_amd.slab import SlabDriver
    from oracle_slab_collider_engine import OracleSlabColliderEngine
    drv = SlabDriver.dambreak(sc.SCENES[name]["n3"], math_mode=0, device=0, axis=sc.AXIS, vel_fn=sc.vel_fn,
                             engine_factory=OracleSlabColliderEngine, collider=sc.collider_of(name))
    assert drv.collider and drv.engine.mesh is not None
    drv.wcsph_step(sc.STEPS)
    assert len(drv.engine.hit_log) == sc.STEPS, "one collide per step and rank"
    res = drv.gather_state(drv.n_total)
    logs = [None] * world if rank == 0 else None
    dist.gather_object(drv.engine.hit_log, logs, dst=0)
    if rank == 0:
        gp, gv, seen = res
        hits = {f"hits_{r}_{s}": logs[r][s] for r in range(world) for s in range(sc.STEPS)}
        np.savez(out, pos=gp, vel=gv, seen=seen, **hits)
    dist.destroy_process_group()


def _single_domain(name):
    """the single-domain oracle with respond after every step: (positions, velocities, moved ids per step)"""
    n3 = sc.SCENES[name]["n3"]
    p, pos, vel = sc.initial_state(n3)
    verts, normals, radius, rest = sc.collider_of(name)
    q = helpers.oracle_params(p)
    frc = np.tile(np.array(p.force_reset[:], np.float32), (n3 ** 3, 1))
    moved_ids = []
    for _ in range(sc.STEPS):
        ora = po.OracleSPH.from_state(q, pos, vel=vel, force=frc)
        ora.wcsph_step(1)
        pos, vel, moved = collider_ref.respond(ora.positions(), ora.velocities(), verts, normals, p.dt, radius, rest)
        moved_ids.append(np.flatnonzero(moved))
    return pos, vel, moved_ids


@pytest.mark.parametrize("name", ["A", "B"])
def test_slab_ranks_with_a_collider_match_the_single_domain(tmp_path, name):
    world = sc.SCENES[name]["world"]
    out = str(tmp_path / "slab.npz")
    mp.spawn(_worker, args=(world, _free_port(), name, out), nprocs=world, join=True)
    z = np.load(out)
    assert np.all(z["seen"] == 1), "every particle must be owned by exactly one rank"
    pos, vel, moved_ids = _single_domain(name)
    on_rank = np.zeros(world, dtype=np.int64)
    for s in range(sc.STEPS):
        per_rank = [z[f"hits_{r}_{s}"] for r in range(world)]
        got = np.concatenate(per_rank)
        assert got.size == np.unique(got).size, f"step {s}: a particle was collided by two ranks"
        assert moved_ids[s].size > 0, f"step {s}: the scene must collide in every step"
        assert np.array_equal(np.sort(got), moved_ids[s]), f"step {s}: the ranks moved other particles than the single domain"
        on_rank += [h.size for h in per_rank]
    assert np.all(on_rank > 0), "every rank must have collided some particle"
    assert helpers.rel_err(z["pos"], pos) < 2e-6
    assert helpers.rel_err(z["vel"], vel) < 2e-5
