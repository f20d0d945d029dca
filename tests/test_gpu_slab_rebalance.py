"""GPU: slab re-balancing -- the planes move during a run.

dsl_slab_layer_counts (k_slab_layer_count) against numpy, integer for integer; the native drivers with
dsl_slab_rebalance on (dsl_slab_wcsph_step / dsl_slab_pcisph_step over HostStagedComm, slabs along x, unbalanced
starts) against the single engine and the single-domain oracle; native against the Python protocol bit for bit; off
means off; the refusals; and a message capacity too small for a moving plane's migrants."""
import functools
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import helpers
from test_slab_cpu import _free_port, _vel_fn

pytestmark = pytest.mark.gpu

STEPS = 10   # as in test_gpu_slab.py
EVERY = 2
AXIS = 0     # slabs along x: the block fills a quarter of the box length
INF = float("inf")


# ---- dsl_slab_layer_counts against numpy ------------------------------------------------------------------------
# the unit scene of test_gpu_slab_messages.py: h = 1, grid box [-8, 8]^3 (16 cell layers, tiles of 4), dyadic planes

GUARD, SENTINEL = 64, -559038737
N_ODD = 1701  # 26 waves + 37 lanes, 6 workgroups + 165 lanes: neither a wave nor a block multiple


def _lattice():
    return (np.float32(5.0) * helpers.jittered_lattice(12)).astype(np.float32)  # 12^3 in [-5.2, 5)^3


def _slab_engine(pos, axis, lo, hi):
    from test_gpu_slab_messages import _engine, _unit_params
    vel = helpers.seeded_velocities(pos.shape[0])
    return _engine(_unit_params(pos.shape[0], capacity=pos.shape[0] + 256), pos, vel, None, (axis, lo, hi))


def _ref_counts(pos, axis, lo, hi, origin, n_layers):
    a = pos[:, axis]
    with np.errstate(invalid="ignore"):
        own = (a >= np.float32(lo)) & (a < np.float32(hi))  # false for NaN
    f = np.floor((a[own] - np.float32(origin)) * np.float32(1.0))
    return np.bincount(np.clip(f, 0, n_layers - 1).astype(np.int64), minlength=n_layers).astype(np.int32), int(own.sum())


def _counts(eng, origin, n_layers):
    """the call into a sentinel-filled buffer with a guard tail nobody may touch"""
    import torch
    buf = torch.full((n_layers + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    eng.slab_layer_counts(origin, n_layers, buf.data_ptr())
    eng.sync()
    got = buf.cpu().numpy()
    assert np.all(got[n_layers:] == SENTINEL), "the count wrote behind its n_layers words"
    return got[:n_layers]


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("n", [N_ODD, 12 ** 3])
def test_layer_counts_equal_numpy_on_every_axis(axis, n):
    pos = _lattice()[:n]
    lo, hi = -2.0, 3.0  # a slab in the middle: live particles on both sides are not owned
    eng = _slab_engine(pos, axis, lo, hi)
    state = eng.download("positions", sorted_order=True)
    want, owned = _ref_counts(state, axis, lo, hi, -8.0, 16)
    assert 0 < owned < n and eng.n_owned() == owned
    got = _counts(eng, -8.0, 16)
    assert np.array_equal(got, want), (got, want)
    assert got[:6].sum() == 0 and got[11:].sum() == 0 and np.count_nonzero(got) == 5
    # a second look overwrites the first (and an unsorted upload order counts the same after the neighbour build)
    eng.nn()
    assert np.array_equal(_counts(eng, -8.0, 16), want)
    eng.close()


def test_layer_counts_right_after_a_step_skip_the_nan_ghosts():
    pos = _lattice()[:N_ODD]
    lo, hi = -2.0, 3.0
    eng = _slab_engine(pos, 2, lo, hi)
    eng.nn()
    eng.density_all()
    eng.force_pass()  # owned particles are integrated, every ghost's position becomes NaN
    state = eng.download("positions", sorted_order=True)
    assert np.isnan(state[:, 2]).sum() > 0
    want, owned = _ref_counts(state, 2, lo, hi, -8.0, 16)
    assert owned > 0 and want.sum() == owned
    assert np.array_equal(_counts(eng, -8.0, 16), want)
    eng.close()


def test_layer_counts_clamp_into_the_first_and_the_last_layer():
    """an origin one and a half tiles below the grid and fewer layers than reach the top: owned particles below the
    origin (they lie outside the grid box as well) count in layer 0, those above the last layer in the last"""
    pos = _lattice()[:N_ODD].copy()
    pos[:5, 0] = np.array([-20.5, -15.25, -14.0009765625, -300.0, -14.0], np.float32)
    lo, hi, origin, n_layers = -INF, 3.0, -14.0, 12  # layers cover [-14, -2)
    eng = _slab_engine(pos, 0, lo, hi)
    state = eng.download("positions", sorted_order=True)
    want, owned = _ref_counts(state, 0, lo, hi, origin, n_layers)
    below, above = int((state[:, 0] < np.float32(origin)).sum()), int(((state[:, 0] >= -2.0) & (state[:, 0] < 3.0)).sum())
    assert below == 4 and above > 100
    assert want[0] == below + 1 and want[-1] >= above and want.sum() == owned
    assert np.array_equal(_counts(eng, origin, n_layers), want)
    eng.close()


@pytest.mark.parametrize("n_layers", [1, 4096])
def test_layer_counts_with_one_and_with_4096_layers(n_layers):
    pos = _lattice()[:N_ODD]
    eng = _slab_engine(pos, 1, -2.0, 3.0)
    state = eng.download("positions", sorted_order=True)
    want, owned = _ref_counts(state, 1, -2.0, 3.0, -8.0, n_layers)
    got = _counts(eng, -8.0, n_layers)
    assert np.array_equal(got, want)
    assert got.sum() == owned and (n_layers > 1 or got[0] == owned)
    eng.close()


def test_layer_counts_with_every_particle_in_one_layer():
    pos = _lattice()[:N_ODD].copy()
    pos[:, 2] = (np.float32(0.5) + np.float32(0.08) * pos[:, 2]).astype(np.float32)  # all inside [0, 1): layer 8
    eng = _slab_engine(pos, 2, -2.0, 3.0)
    got = _counts(eng, -8.0, 16)
    want = np.zeros(16, np.int32)
    want[8] = N_ODD
    assert np.array_equal(got, want)
    eng.close()


# ---- the drivers ------------------------------------------------------------------------------------------------

def _pci_params(p):
    from test_gpu_slab import _pci_params as base
    base(p, False)


def _worker(rank, world, port, cfg, out):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import torch
    torch.cuda.set_device(0)
    from dieselfluid_amd.slab import SlabDriver, SlabOverflow
    SlabDriver.REPLAN_EVERY = 4  # the message re-sizing runs inside the run, with a histogram to look at
    pcisph, native = cfg["pcisph"], cfg["native"]
    kw = dict(layers=cfg["layers"]) if cfg["layers"] else {}
    if cfg["every"] or cfg["configured"]:
        kw.update(rebalance_every=cfg["every"], rebalance_bounds=cfg["bounds"])
    vel = (lambda ids, pos: 0.5 * _vel_fn(ids, pos, axis=2)) if pcisph else (lambda ids, pos: _vel_fn(ids, pos, axis=AXIS))
    drv = SlabDriver.dambreak(cfg["n3"], math_mode=cfg["math_mode"], device=0, axis=AXIS, overlap=cfg["overlap"],
                              native=native and not cfg["cap_full"], pcisph=pcisph, vel_fn=vel,
                              params_hook=_pci_params if pcisph else None, **kw)
    if cfg["cap_full"]:  # a message capacity the re-plan cannot grow past
        drv.engine.cap_full = cfg["cap_full"]
        drv.engine.max_full = 2 * cfg["cap_full"]
        if native:
            drv.attach_native()
    assert bool(getattr(drv, "native", False)) == native
    step = drv.pcisph_step if pcisph else drv.wcsph_step
    # (the planes the run starts from: the Python protocol keeps its current plan in drv.balance["planes"])
    balance0 = None if drv.balance is None else {k: list(v) if isinstance(v, list) else v for k, v in drv.balance.items()}
    log, raised = [], None
    for s in range(1, STEPS + 1):
        if cfg["stop_after"] and s == cfg["stop_after"] + 1:
            drv.set_rebalance_every(0)
        try:
            step(1)  # one call per step: a plan pending when a call returns is applied by the next call's first step
        except SlabOverflow as e:
            raised = (s, str(e))
            break
        planes, counts, looks = drv.balance_state() if drv.balance is not None else (None, None, 0)
        log.append((s, planes, None if counts is None else np.asarray(counts).tolist(), looks, drv.lo, drv.hi,
                    drv.engine.status()[0] if cfg["cap_full"] else 0))
    res = drv.gather_state(cfg["n3"] ** 3) if raised is None else None
    st = drv.engine.status()
    core = drv.engine_core
    calls = list(core._comm.calls) if native else []
    mine = dict(n=drv.engine.n, owned=core.n_owned() if raised is None else -1, st=st, log=log, raised=raised, calls=calls,
                balance=balance0,
                pci=(core.stats().pci_iters, core.stats().pci_max_error) if pcisph else None)
    info = [None] * world if rank == 0 else None
    dist.gather_object(mine, info, dst=0)
    if rank == 0:
        with open(out, "wb") as f:
            pickle.dump(dict(pos=None if res is None else res[0], vel=None if res is None else res[1],
                             seen=None if res is None else res[2], info=info), f)
    dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _run(n3, math_mode, overlap, layers, every=EVERY, native=True, pcisph=False, stop_after=0, cap_full=0,
         configured=True, bounds=None):
    """one run of `len(layers) - 1` ranks on cuda:0; cached: the tests below share the runs they have in common"""
    world = len(layers) - 1
    cfg = dict(n3=n3, math_mode=math_mode, overlap=overlap, layers=list(layers), every=every, native=native, pcisph=pcisph,
               stop_after=stop_after, cap_full=cap_full, configured=configured, bounds=bounds)
    out = os.path.join(tempfile.mkdtemp(prefix="dsl_rebalance_"), "run.pkl")
    mp.spawn(_worker, args=(world, _free_port(), cfg, out), nprocs=world, join=True)
    with open(out, "rb") as f:
        z = pickle.load(f)
    os.remove(out)
    return z


@functools.lru_cache(maxsize=None)
def _single(n3, math_mode, shuffle=False):
    from test_gpu_slab import _single as run
    return run(n3, math_mode, 1.0, steps=STEPS, shuffle=shuffle, axis=AXIS)


def _looks_of(z):
    """[(histogram, planes planned)] per look, from the per-step states rank 0 recorded (identical on every rank)"""
    logs = [i["log"] for i in z["info"]]
    assert all([e[:4] for e in l] == [e[:4] for e in logs[0]] for l in logs), "the ranks disagree on planes or histograms"
    looks, seen = [], 0
    for _s, planes, counts, n_looks, _lo, _hi, _ovf in logs[0]:
        assert n_looks in (seen, seen + 1)
        if n_looks > seen:
            looks.append((counts, planes))
            seen = n_looks
    return looks


def _check_balanced_run(z, n3, world, every=EVERY, n_looks=None):
    """what every case asserts: ownership, no overflow, moves on every interior plane, the plan replayed, and one
    all-reduce of n_layers words per look on every rank"""
    from dieselfluid_amd.slab import plan_planes
    assert np.all(z["seen"] == 1)
    assert sum(i["owned"] for i in z["info"]) == n3 ** 3       # every particle owned exactly once
    assert sum(i["n"] for i in z["info"]) > n3 ** 3            # ghosts are present
    assert all(i["st"][0] == 0 and i["st"][1] == 0 for i in z["info"])  # no overflow flag, the split margin held
    b = z["info"][0]["balance"]
    looks = _looks_of(z)
    n_looks = STEPS // every if n_looks is None else n_looks
    assert len(looks) == n_looks
    cur, moved = list(b["planes"]), [0] * (world + 1)
    for counts, planes in looks:
        assert sum(counts) == n3 ** 3, "the MAX of the ranks' disjoint histograms must be their sum"
        assert planes == plan_planes(counts, cur, b["plane_min"], b["plane_max"], b["min_layers"])
        moved = [m + (a != c) for m, a, c in zip(moved, planes, cur)]
        cur = planes
    assert all(m > 0 for m in moved[1:-1]), f"every interior plane must move: {moved}"
    assert moved[0] == 0 and moved[-1] == 0
    for i in z["info"]:
        if i["calls"]:
            assert sum(1 for c in i["calls"] if c == ("all_reduce_max", b["n_layers"])) == n_looks
            assert {c[1] for c in i["calls"] if isinstance(c, tuple) and c[0] == "all_reduce_max"} <= {1, 4, b["n_layers"]}
    # drv.lo / drv.hi follow the planes: after the last step the plan of the last look but one is in force
    applied = looks[-2][1] if STEPS % every == 0 and n_looks == STEPS // every else looks[-1][1]
    for r, i in enumerate(z["info"]):
        lo, hi = i["log"][-1][4], i["log"][-1][5]
        if r > 0:
            assert np.float32(lo) == np.float32(b["origin"]) + np.float32(applied[r]) * np.float32(b["edge"])
        if r < world - 1:
            assert np.float32(hi) == np.float32(b["origin"]) + np.float32(applied[r + 1]) * np.float32(b["edge"])
    # balance: the largest share, by the first and by the last histogram and the planes in force then
    def ratio(counts, planes):
        own = np.array([sum(counts[planes[r]:planes[r + 1]]) for r in range(world)], float)
        return own.max() / own.mean()
    r0, r1 = ratio(looks[0][0], b["planes"]), ratio(looks[-1][0], applied)
    print(f"max/mean owned {r0:.3f} -> {r1:.3f}, planes {b['planes']} -> {cur}")
    assert r1 < r0
    return looks


EXACT_CASES = [(16, (0, 12, 16)), (24, (0, 4, 20, 24))]


@pytest.mark.parametrize("n3,layers", EXACT_CASES, ids=["2ranks_n16", "3ranks_n24"])
def test_exact_slabs_with_moving_planes_are_the_single_domain_run(n3, layers):
    from test_gpu_slab import _assert_identical, _oracle_single
    from test_gpu_slab import _check_exchange_calls
    z = _run(n3, 0, None, layers)
    _check_balanced_run(z, n3, len(layers) - 1)
    _check_exchange_calls([i["calls"] for i in z["info"]], len(layers) - 1)
    pos, vel = _single(n3, 0)
    _assert_identical("the single engine", z["pos"], z["vel"], pos, vel)
    opos, ovel = _oracle_single(n3, 1.0, steps=STEPS, axis=AXIS)
    _assert_identical("the single-domain oracle", z["pos"], z["vel"], opos, ovel)


@pytest.mark.parametrize("overlap", [False, True], ids=["unsplit", "split"])
def test_fast_slabs_with_moving_planes_stay_within_the_shuffle_yardstick(overlap):
    """the yardstick of test_gpu_slab._slabs_against_single: what re-ordering the particles and moving the grid origin
    does to a single-engine run, times five"""
    n3, layers = 32, (0, 24, 32)
    z = _run(n3, 1, overlap, layers)
    _check_balanced_run(z, n3, 2)
    pos, vel = _single(n3, 1)
    pos_s, vel_s = _single(n3, 1, shuffle=True)
    tol_x = max(4e-6, 5.0 * helpers.rel_err(pos_s, pos))
    tol_v = max(1e-4, 5.0 * helpers.rel_err(vel_s, vel))
    ex, ev = helpers.rel_err(z["pos"], pos), helpers.rel_err(z["vel"], vel)
    print(f"slab-vs-single x {ex:.2e} (tol {tol_x:.2e})  v {ev:.2e} (tol {tol_v:.2e})")
    assert ex < tol_x
    assert ev < tol_v


def test_pcisph_exact_slabs_with_moving_planes_are_the_single_engine():
    from test_gpu_slab import _assert_identical, _pci_single
    n3, layers = 16, (0, 12, 16)
    z = _run(n3, 0, None, layers, pcisph=True)
    _check_balanced_run(z, n3, 2)
    pos, vel, iters, err = _pci_single(n3, 0, False)
    assert all(i["pci"][0] == iters and np.float32(i["pci"][1]) == np.float32(err) for i in z["info"])
    _assert_identical("the single engine", z["pos"], z["vel"], pos, vel)
    for i in z["info"]:
        assert sum(1 for c in i["calls"] if c == ("all_reduce_max", 1)) == STEPS * 4  # the iteration error, as before


@pytest.mark.parametrize("n3,math_mode,overlap,layers", [(16, 0, None, (0, 12, 16)), (32, 1, True, (0, 24, 32))],
                         ids=["exact", "fast_split"])
def test_native_driver_equals_the_python_protocol_with_moving_planes(n3, math_mode, overlap, layers):
    from test_gpu_slab import _bits_equal
    nat = _run(n3, math_mode, overlap, layers)
    py = _run(n3, math_mode, overlap, layers, native=False)
    _check_balanced_run(py, n3, len(layers) - 1)
    assert _looks_of(py) == _looks_of(nat)  # the same histograms, the same planes, look for look
    assert [[e[4:6] for e in i["log"]] for i in py["info"]] == [[e[4:6] for e in i["log"]] for i in nat["info"]]
    assert _bits_equal(py["pos"], nat["pos"]) and _bits_equal(py["vel"], nat["vel"])


def test_every_zero_after_every_two_stops_the_moves():
    """looks after steps 2 and 4, dsl_slab_rebalance(0) after step 4: the move planned at step 4 is still applied (step
    5), then nothing moves and nothing is counted or reduced any more; the run stays the single-domain run"""
    from test_gpu_slab import _assert_identical
    n3, layers = 16, (0, 12, 16)
    z = _run(n3, 0, None, layers, stop_after=4)
    assert np.all(z["seen"] == 1) and sum(i["owned"] for i in z["info"]) == n3 ** 3
    b = z["info"][0]["balance"]
    for i in z["info"]:
        assert [e[3] for e in i["log"]] == [0, 1, 1, 2, 2, 2, 2, 2, 2, 2]
        assert sum(1 for c in i["calls"] if c == ("all_reduce_max", b["n_layers"])) == 2
        planes = [(e[4], e[5]) for e in i["log"]]
        assert planes[0] == planes[1] and planes[2] == planes[3] and planes[1] != planes[2] and planes[3] != planes[4]
        assert all(q == planes[4] for q in planes[5:])
    pos, vel = _single(n3, 0)
    _assert_identical("the single engine", z["pos"], z["vel"], pos, vel)


def test_a_run_that_never_enabled_it_makes_todays_transport_calls():
    from test_gpu_slab import _assert_identical, _check_exchange_calls
    n3, layers = 16, (0, 12, 16)
    z = _run(n3, 0, None, layers, every=0, configured=False)
    assert np.all(z["seen"] == 1) and sum(i["owned"] for i in z["info"]) == n3 ** 3
    calls = [i["calls"] for i in z["info"]]
    _check_exchange_calls(calls, 2)
    for seq in calls:
        assert {c for c in seq if isinstance(c, tuple) and c[0] == "all_reduce_max"} == {("all_reduce_max", 4)}
        assert sum(1 for c in seq if c == "group_start") == STEPS + 1  # the first exchange, then one per step
    for i in z["info"]:
        assert all(e[4:6] == i["log"][0][4:6] for e in i["log"])  # the planes stay
    pos, vel = _single(n3, 0)
    _assert_identical("the single engine", z["pos"], z["vel"], pos, vel)


def test_a_message_too_small_for_a_moving_planes_migrants_is_an_overflow_on_every_rank():
    """cap_full = 800 holds the h band of the 16^3 block (two lattice layers of 256 and the step's migrants); the plane
    that moves in step 3 sends a cell layer -- 512 more -- on top, before any re-plan could have grown the messages: the
    flag is up after step 3 and not before, and the library's next re-plan -- step 8 -- fails on every rank"""
    z = _run(16, 0, None, (0, 12, 16), cap_full=800)
    for i in z["info"]:
        assert i["raised"] is not None and i["raised"][0] == 8 and "overflow" in i["raised"][1]
        assert [e[6] for e in i["log"]][:2] == [0, 0]
    assert max(i["log"][2][6] for i in z["info"]) > 0


# ---- refusals ---------------------------------------------------------------------------------------------------

def _attached(rank=0):
    """rank `rank` of two on the unit grid ([-8, 8], h = 1), plane at 0; the communicator's table is never called"""
    from dieselfluid_amd import DslError
    from dieselfluid_amd.engine import HostStagedComm
    pos = _lattice()[:N_ODD]
    lo, hi = (-INF, 0.0) if rank == 0 else (0.0, INF)
    eng = _slab_engine(pos, 0, lo, hi)
    comm = HostStagedComm(2, rank, 0)
    eng.slab_attach(comm, -1 if rank == 0 else 0, 1 if rank == 0 else -1, 1.0, 2.0, 64, 64, False)
    return eng, DslError


GOOD = dict(every=2, origin=-8.0, n_layers=16, planes=[0, 8, 16], plane_min=[0, 4, 16], plane_max=[0, 12, 16], min_layers=2)


@pytest.mark.parametrize("change,word", [
    (dict(planes=[0, 7, 16]), "is not origin"),               # this rank's plane is not where the planes say
    (dict(origin=-8.5), "cell plane"),                          # the layers are off the cell lattice
    (dict(plane_max=[0, 15, 16]), "grid covers"),               # plane + band would leave the rank's grid
    (dict(plane_min=[0, 1, 16]), "grid covers"),
    (dict(n_layers=4097), "4096"),
    (dict(min_layers=1), "min_layers"),
    (dict(planes=[0, 8, 9], n_layers=9, plane_max=[0, 8, 9]), "min_layers apart"),
])
@pytest.mark.parametrize("rank", [0, 1])
def test_rebalance_refusals_name_the_shortfall(rank, change, word):
    eng, DslError = _attached(rank)
    with pytest.raises(DslError, match=word):
        eng.slab_rebalance(**dict(GOOD, **change))
    eng.slab_rebalance(**GOOD)  # ... and the arguments without the change are accepted
    planes, counts, looks, moves = eng.slab_rebalance_state()
    assert planes.tolist() == [0, 8, 16] and not counts.any() and looks == 0 and moves == 0
    eng.slab_rebalance(0)
    eng.close()


def test_rebalance_needs_an_attached_slab_and_the_building_blocks_need_a_slab():
    from dieselfluid_amd import DslError, SPHEngine
    from test_gpu_slab_messages import _unit_params
    pos = _lattice()[:N_ODD]
    eng = _slab_engine(pos, 0, -2.0, 3.0)
    with pytest.raises(DslError, match="dsl_slab_attach"):
        eng.slab_rebalance(**GOOD)
    with pytest.raises(DslError, match="dsl_slab_rebalance first"):
        eng.slab_rebalance_state()
    assert eng.slab_get_planes() == (-2.0, 3.0)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0)):
        with pytest.raises(DslError, match="empty range"):
            eng.slab_move_planes(lo, hi)
    assert eng.slab_get_planes() == (-2.0, 3.0)
    eng.slab_move_planes(-3.0, 2.0)
    assert eng.slab_get_planes() == (-3.0, 2.0)
    state = eng.download("positions", sorted_order=True)
    assert np.array_equal(_counts(eng, -8.0, 16), _ref_counts(state, 0, -3.0, 2.0, -8.0, 16)[0])  # the count sees the new planes
    import torch
    buf = torch.zeros(4097, dtype=torch.int32, device="cuda")
    for origin, n_layers, word in ((-8.0, 0, "n_layers"), (-8.0, 4097, "n_layers"), (-8.25, 16, "cell plane")):
        with pytest.raises(DslError, match=word):
            eng.slab_layer_counts(origin, n_layers, buf.data_ptr())
    with pytest.raises(DslError, match="null output"):
        eng.slab_layer_counts(-8.0, 16, 0)
    eng.close()
    plain = SPHEngine(_unit_params(N_ODD))
    plain.upload("positions", pos)
    for call in (lambda: plain.slab_move_planes(-1.0, 1.0), lambda: plain.slab_get_planes(),
                 lambda: plain.slab_layer_counts(-8.0, 16, buf.data_ptr())):
        with pytest.raises(DslError, match="no slab configured"):
            call()
    plain.close()
