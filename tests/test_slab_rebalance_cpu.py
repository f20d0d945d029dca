"""Slab re-balancing on the CPU: the plan (slab.plan_planes) by hand and by its properties, and the Python protocol --
look, plan, apply -- of SlabDriver over gloo, with an oracle-backed engine that has the two building blocks
(layer_counts, move_planes) in numpy.  The dam-break split along x starts unbalanced; planes move one cell layer per
look; every particle stays owned exactly once and the run stays the single-domain run."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import helpers
from oracle import pyoracle as po
from oracle_slab_engine import OracleSlabEngine
from test_slab_cpu import _free_port, _vel_fn

N3 = 12
STEPS = 8
EVERY = 2
AXIS = 0


# ---- the plan ---------------------------------------------------------------------------------

def _plan(counts, planes, lo=None, hi=None, min_layers=2):
    from dieselfluid_amd.slab import plan_planes
    R, n = len(planes) - 1, len(counts)
    lo = [0] * (R + 1) if lo is None else lo
    hi = [n] * (R + 1) if hi is None else hi
    return plan_planes(counts, planes, lo, hi, min_layers)


def test_plan_two_ranks_75_25():
    # 8 layers of 10 particles, the plane after layer 6: 75 % below it.  The even split is at 4; one layer per look.
    counts = [10] * 8
    assert _plan(counts, [0, 6, 8]) == [0, 5, 8]
    assert _plan(counts, [0, 5, 8]) == [0, 4, 8]
    assert _plan(counts, [0, 4, 8]) == [0, 4, 8]
    assert _plan(counts, [0, 2, 8]) == [0, 3, 8]  # ... and from the other side


def test_plan_three_ranks_2_8_2_of_12():
    counts = [7] * 12
    assert _plan(counts, [0, 2, 10, 12]) == [0, 3, 9, 12]
    assert _plan(counts, [0, 3, 9, 12]) == [0, 4, 8, 12]
    assert _plan(counts, [0, 4, 8, 12]) == [0, 4, 8, 12]  # every plane at its target: nothing moves


def test_plan_targets_follow_the_histogram_and_ties_take_the_lower_layer():
    # all particles in layers 2 and 3: the even split of two ranks is between them
    assert _plan([0, 0, 50, 50, 0, 0], [0, 4, 6]) == [0, 3, 6]
    assert _plan([0, 0, 50, 50, 0, 0], [0, 3, 6]) == [0, 3, 6]
    # an empty stretch: S(k) R = N for k = 1 .. 4; the smallest wins, so a plane at 3 moves down
    assert _plan([10, 0, 0, 0, 10], [0, 3, 5], min_layers=1) == [0, 2, 5]
    # no particles at all: no target, no move
    assert _plan([0] * 6, [0, 4, 6]) == [0, 4, 6]


def test_plan_a_bound_stops_a_move():
    counts = [10] * 8
    assert _plan(counts, [0, 6, 8], lo=[0, 6, 8], hi=[0, 7, 8]) == [0, 6, 8]
    assert _plan(counts, [0, 6, 8], lo=[0, 5, 8], hi=[0, 7, 8]) == [0, 5, 8]
    assert _plan(counts, [0, 2, 8], lo=[0, 1, 8], hi=[0, 2, 8]) == [0, 2, 8]


def test_plan_min_layers_stops_a_move():
    # the even split is at 1, the lower slab may not get thinner than 2
    assert _plan([90, 2, 2, 2, 2, 2], [0, 2, 6], min_layers=2) == [0, 2, 6]
    assert _plan([90, 2, 2, 2, 2, 2], [0, 3, 6], min_layers=2) == [0, 2, 6]
    # upper end likewise
    assert _plan([2, 2, 2, 2, 2, 90], [0, 4, 6], min_layers=2) == [0, 4, 6]
    # two interior planes that want the same ground: plane 1 may go up only if plane 2 coming DOWN one layer still
    # leaves min_layers between them
    counts = [1, 1, 1, 1, 40, 40, 1, 1, 1, 1]
    assert _plan(counts, [0, 3, 6, 10], min_layers=2) == [0, 3, 5, 10]  # 1 -> 4 is dropped (5 - 4 < 2); 2 goes to 5
    assert _plan(counts, [0, 2, 8, 10], min_layers=2) == [0, 3, 7, 10]


def test_plan_properties_on_random_histograms():
    rng = np.random.default_rng(20240611)
    for _ in range(400):
        n = int(rng.integers(6, 40))
        R = int(rng.integers(2, 6))
        m = int(rng.integers(2, 4))
        if n < R * m:
            continue
        kind = rng.integers(0, 3)
        counts = rng.integers(0, 1000, n)
        if kind == 1:  # a block of fluid in part of the domain
            a = int(rng.integers(0, n - 1))
            counts[:a] = 0
            counts[min(n, a + int(rng.integers(1, n))):] = 0
        elif kind == 2:
            counts[rng.random(n) < 0.7] = 0
        # planes at least m apart
        gaps = rng.multinomial(n - R * m, np.ones(R) / R) + m
        planes = [0] + [int(v) for v in np.cumsum(gaps)]
        assert planes[-1] == n
        lo = [0] + [int(max(0, q - rng.integers(0, 4))) for q in planes[1:-1]] + [n]
        hi = [0] + [int(min(n, q + rng.integers(0, 4))) for q in planes[1:-1]] + [n]
        new = _plan(counts, planes, lo, hi, m)
        assert new[0] == planes[0] and new[-1] == planes[-1]            # the end planes never move
        assert all(abs(a - b) <= 1 for a, b in zip(new, planes))        # one layer per plane per look
        assert all(lo[r] <= new[r] <= hi[r] for r in range(1, R))       # bounds
        assert all(b - a >= m for a, b in zip(new, new[1:]))            # min_layers
        # iterated, the plan comes to rest, and a plan at rest is reproduced (no move once nothing wants to move)
        cur = new
        for _it in range(2 * n):
            nxt = _plan(counts, cur, lo, hi, m)
            if nxt == cur:
                break
            cur = nxt
        assert _plan(counts, cur, lo, hi, m) == cur
        # every plane at its target: no move, whatever the bounds
        if counts.sum() > 0:
            S = np.concatenate([[0], np.cumsum(counts)])
            N = int(S[-1])
            T = [0] + [int(np.argmin(np.abs(S * R - r * N))) for r in range(1, R)] + [n]
            if all(b - a >= m for a, b in zip(T, T[1:])):
                assert _plan(counts, T, lo, hi, m) == T


# ---- the Python protocol over gloo ----------------------------------------------------------------

class OracleBalanceEngine(OracleSlabEngine):
    """OracleSlabEngine + the two building blocks of the re-balancing, in numpy"""

    def layer_counts(self, origin, n_layers):
        own = self._owned(self.pos)  # false for NaN
        inv = np.float32(1.0) / np.float32(self.p.h)
        f = np.floor((self.pos[own, self.axis] - np.float32(origin)) * inv)
        lay = np.clip(f, 0, n_layers - 1).astype(np.int64)
        return torch.from_numpy(np.bincount(lay, minlength=n_layers).astype(np.int32))

    def move_planes(self, lo, hi):
        self.lo, self.hi = lo, hi


def _worker(rank, world, port, layers, every, out):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dieselfluid_amd.slab import SlabDriver
    drv = SlabDriver.dambreak(N3, math_mode=0, device=0, axis=AXIS, engine_factory=OracleBalanceEngine,
                              vel_fn=functools.partial(_vel_fn, axis=AXIS), layers=layers, rebalance_every=every)
    planes0 = list(drv.balance["planes"]) if every else None
    owned0 = len(drv.engine.owned_state(drv.axis, drv.lo, drv.hi)[0])
    seen_ok = True
    for _ in range(STEPS):
        drv.wcsph_step(1)
        res = drv.gather_state(N3 ** 3)
        if rank == 0:
            seen_ok = seen_ok and bool(np.all(res[2] == 1))
    owned1 = len(drv.engine.owned_state(drv.axis, drv.lo, drv.hi)[0])
    info = [None] * world if rank == 0 else None
    log = [(s, c.tolist(), pl) for s, c, pl in drv.balance_log]
    dist.gather_object((owned0, owned1, log, drv.lo, drv.hi), info, dst=0)
    if rank == 0:
        import pickle
        with open(out, "wb") as f:
            pickle.dump(dict(pos=res[0], vel=res[1], seen_ok=seen_ok, info=info, planes0=planes0,
                             balance={k: v for k, v in (drv.balance or {}).items() if k != "counts"}), f)
    dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _oracle_single():
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(N3, math_mode=0)
    vel = _vel_fn(np.arange(N3 ** 3), pos, AXIS)
    frc = np.tile(np.array(p.force_reset[:], np.float32), (N3 ** 3, 1))
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, vel=vel, force=frc)
    ora.wcsph_step(STEPS)
    return ora.positions(), ora.velocities()


def _run(tmp_path, layers, every):
    import pickle
    world = len(layers) - 1
    out = str(tmp_path / "rebalance.pkl")
    mp.spawn(_worker, args=(world, _free_port(), layers, every, out), nprocs=world, join=True)
    with open(out, "rb") as f:
        return pickle.load(f)


@pytest.mark.parametrize("layers", [[0, 8, 12], [0, 2, 10, 12]], ids=["2ranks", "3ranks"])
def test_moving_planes_keep_the_single_domain_run(tmp_path, layers):
    from dieselfluid_amd.slab import plan_planes
    z = _run(tmp_path, layers, EVERY)
    world = len(layers) - 1
    assert z["seen_ok"], "every particle must be owned by exactly one rank after every step"
    b, logs = z["balance"], [i[2] for i in z["info"]]
    assert all(l == logs[0] for l in logs), "every rank must have taken the same decisions"
    log = logs[0]
    assert [s for s, _, _ in log] == list(range(EVERY, STEPS + 1, EVERY))
    # the planes recorded are the plan replayed on the histograms recorded
    cur = z["planes0"]
    moved = [0] * (world + 1)
    for _s, counts, planes in log:
        assert sum(counts) == N3 ** 3, "the ranks' histograms must add up to every particle"
        want = plan_planes(counts, cur, b["plane_min"], b["plane_max"], b["min_layers"])
        assert planes == want
        moved = [m + (a != c) for m, a, c in zip(moved, planes, cur)]
        cur = planes
    assert all(m > 0 for m in moved[1:-1]), f"every interior plane must move at least once: {moved}"
    assert moved[0] == 0 and moved[-1] == 0
    # the planes in force are the last applied plan (the plan of the last look, at step STEPS, is still pending)
    applied = log[-2][2]
    for r, (_o0, _o1, _l, lo, hi) in enumerate(z["info"]):
        if r > 0:
            assert np.float32(lo) == np.float32(b["origin"]) + np.float32(applied[r]) * np.float32(b["edge"])
        if r < world - 1:
            assert np.float32(hi) == np.float32(b["origin"]) + np.float32(applied[r + 1]) * np.float32(b["edge"])
    # balance: max / mean of the owned counts
    own0 = np.array([i[0] for i in z["info"]], float)
    own1 = np.array([i[1] for i in z["info"]], float)
    assert own0.sum() == N3 ** 3 and own1.sum() == N3 ** 3
    r0, r1 = own0.max() / own0.mean(), own1.max() / own1.mean()
    print(f"max/mean owned: {r0:.3f} -> {r1:.3f}; planes {z['planes0']} -> {cur}")
    assert r1 < r0
    opos, ovel = _oracle_single()
    ex, ev = helpers.rel_err(z["pos"], opos), helpers.rel_err(z["vel"], ovel)
    print(f"against the single-domain oracle: x {ex:.2e} v {ev:.2e}")
    assert ex < 2e-6
    assert ev < 2e-5


def test_static_planes_of_the_same_split_agree_as_well(tmp_path):
    """the same unbalanced split with re-balancing off: no look is taken, no plane moves, and the run is the
    single-domain run to the same tolerance (what the runs with moves are compared with)"""
    z = _run(tmp_path, [0, 8, 12], 0)
    assert z["seen_ok"]
    assert all(i[2] == [] for i in z["info"])
    own0, own1 = [i[0] for i in z["info"]], [i[1] for i in z["info"]]
    assert own0 == [8 * N3 * N3, 4 * N3 * N3] and sum(own1) == N3 ** 3
    opos, ovel = _oracle_single()
    assert helpers.rel_err(z["pos"], opos) < 2e-6
    assert helpers.rel_err(z["vel"], ovel) < 2e-5
