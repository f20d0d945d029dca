"""N>1 path on CPU: two gloo ranks drive SlabDriver with the oracle-backed engine and the
result is compared with a single-process run of the same scene.  Exercises band
selection, migration across the slab plane, ghost classification and id bookkeeping."""
import functools
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import helpers
from oracle import pyoracle as po

N3 = 10
STEPS = 6


def _vel_fn(ids, pos, axis=2):
    # push particles across the slab plane so that migration happens within a few steps
    v = np.zeros_like(pos)
    v[:, axis] = np.where((ids % 3) == 0, 30.0, -25.0).astype(np.float32)
    v[:, (axis + 1) % 3] = 1.0
    return v


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, axis, out, steps=STEPS):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dieselfluid_amd.slab import SlabDriver
    from oracle_slab_engine import OracleSlabEngine
    drv = SlabDriver.dambreak(N3, math_mode=0, device=0, axis=axis, engine_factory=OracleSlabEngine,
                             vel_fn=functools.partial(_vel_fn, axis=axis))
    moved = 0
    for _ in range(steps):
        before = set(drv.engine.owned_state(drv.axis, drv.lo, drv.hi)[0].tolist())
        drv.wcsph_step(1)
        after = set(drv.engine.owned_state(drv.axis, drv.lo, drv.hi)[0].tolist())
        moved += len(after - before)
    res = drv.gather_state(N3 ** 3)
    tot = [None] * world if rank == 0 else None
    dist.gather_object(moved, tot, dst=0)
    if rank == 0:
        gp, gv, seen = res
        np.savez(out, pos=gp, vel=gv, seen=seen, migrated=np.array(sum(tot)))
    dist.destroy_process_group()


@pytest.mark.parametrize("axis,world", [(2, 2), (0, 2), (2, 3)])
def test_slabs_match_single_domain(tmp_path, axis, world):
    from dieselfluid_amd import scenes
    out = str(tmp_path / "slab.npz")
    mp.spawn(_worker, args=(world, _free_port(), axis, out), nprocs=world, join=True)
    z = np.load(out)
    assert np.all(z["seen"] == 1), "every particle must be owned by exactly one rank"
    assert int(z["migrated"]) > 0, "the test must exercise migration across the plane"
    # single-domain oracle run
    p, pos = scenes.dambreak_scene(N3, math_mode=0)
    ids = np.arange(N3 ** 3)
    vel = _vel_fn(ids, pos, axis)
    frc = np.tile(np.array(p.force_reset[:], np.float32), (N3 ** 3, 1))
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, vel=vel, force=frc)
    ora.wcsph_step(STEPS)
    # summation order differs (different particle order per rank): float32 tolerance
    assert helpers.rel_err(z["pos"], ora.positions()) < 2e-6
    assert helpers.rel_err(z["vel"], ora.velocities()) < 2e-5


def test_slab_id_subsets_partition_the_block():
    from dieselfluid_amd import scenes
    n3 = 6
    for axis in (0, 1, 2):
        a = scenes.dambreak_slab_ids(n3, axis, 0, 2)
        b = scenes.dambreak_slab_ids(n3, axis, 2, 6)
        assert np.array_equal(np.sort(np.concatenate([a, b])), np.arange(n3 ** 3))
        full = scenes.dambreak_positions(n3, 0.1)
        assert np.array_equal(scenes.dambreak_positions_ids(n3, 0.1, a), full[a])
        lay = np.floor(full[a][:, axis] / 0.1).astype(int)
        assert lay.min() == 0 and lay.max() == 1


def test_message_reference_matches_the_oracle_engine_word_for_word():
    """helpers.slab_message_reference (the yardstick of tests/test_gpu_slab_messages.py, written from the header's
    description of a message) against OracleSlabEngine.pack (written for the driver tests): the middle rank of a
    3-slab split of the jittered 12^3 lattice, capacities that hold every record, both sides.  Every word either
    of them writes must be the same word; the words behind the records are the oracle's zero fill on one side and
    the reference's "never written" mask on the other."""
    from dieselfluid_amd import scenes
    from oracle_slab_engine import OracleSlabEngine
    n3, axis = 12, 2
    pos = helpers.jittered_lattice(n3)
    vel = helpers.seeded_velocities(n3 ** 3)
    gid = np.random.default_rng(5).permutation(n3 ** 3).astype(np.int32) + 1000
    a = pos[:, axis]
    step = (float(a.max()) - float(a.min())) / (n3 - 1)
    planes = [float(a.min()) - 0.5 * step + r * 4 * step for r in range(4)]
    lo, hi = planes[1], planes[2]
    mine = (a >= np.float32(lo)) & (a < np.float32(hi))
    width_full, width = 1.0 * step, 2.0 * step
    p, _ = scenes.dambreak_scene(n3, math_mode=0, positions=False)
    p.n_particles = int(mine.sum())
    cap_full, cap_x = n3 * n3 * 2, n3 * n3 * 2
    eng = OracleSlabEngine(p, 0, cap_full, cap_x)
    eng.upload("positions", pos[mine])
    eng.upload("velocities", vel[mine])
    eng.set_ids(gid[mine])
    eng.slab_config(axis, lo, hi)
    got = eng.pack(width_full, width, True, True)
    ref = helpers.slab_message_reference(pos[mine], vel[mine], gid[mine], axis, lo, hi, width_full, width, cap_full, cap_x)
    for side, msg in zip(("lo", "hi"), got):
        r = ref[side]
        nf, nx = r["counts"]
        # a layer of 144 particles per category, give or take the jitter; nothing is clamped
        assert 100 < nf <= cap_full and 100 < nx <= cap_x
        words = msg.numpy().view(np.uint32)
        assert words.shape == r["words"].shape
        w = r["written"]
        assert np.array_equal(words[w], r["words"][w]), side
        assert not words[~w].any(), "the oracle engine wrote a word the reference calls untouched"
        assert np.all(r["words"][~w] == helpers.SLAB_SENTINEL)
        assert eng.status()[2:] == (max(ref["lo"]["counts"][0], ref["hi"]["counts"][0]),
                                    max(ref["lo"]["counts"][1], ref["hi"]["counts"][1]))
    # the two messages of this slab share no particle (4 layers, bands of 2), and together they hold all of it
    packed = np.concatenate([gid[mine][ref[s][k]] for s in ("lo", "hi") for k in ("full", "xonly")])
    assert np.array_equal(np.sort(packed), np.sort(gid[mine]))
