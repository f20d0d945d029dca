"""GPU: a collider mesh on slab ranks (DSL_OPT_COLLIDE_SLAB; csrc/collide_slab.hip).

Ranks are processes on cuda:0 over gloo, as in test_gpu_slab_rebalance.py; the scenes are slab_collider_scenes.py's.
EXACT ranks under the native driver are the single engine with the same mesh, bit for bit -- unsplit, with the cell
index, with moving planes, and under PCISPH; FAST ranks (split and unsplit) give the same bits under the native driver
and under the Python protocol; one handle without neighbours is held, phase by phase, to collider_ref.respond; the
refusals name the order; and a run that never sets the option launches no collide kernel.

Every multi-rank test first asserts, on its own single-engine run (made in pieces: build, density, force_pass, download,
collide, download), that the scene does what it is for: a hit in every step, a hit among the particles of every rank, a
particle set back across every interior plane, and for scene C band and inner hits on one rank."""
import functools
import os
import pickle
import tempfile

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import collider_ref
import slab_collider_scenes as sc
from test_slab_cpu import _free_port, _vel_fn

pytestmark = pytest.mark.gpu

INF = float("inf")
PCI_N3, PCI_LAYERS = 16, (0, 12, 16)


def _pci_params(p):
    from test_gpu_slab import _pci_params as base
    base(p, False)


def _pci_collider():
    """a box whose lower z face lies h / 2 above the plane z = 0.75 of PCI_LAYERS: particles that rise through the plane
    meet it at once and are set back across"""
    from dieselfluid_amd import scenes
    p, _ = scenes.dambreak_scene(PCI_N3, math_mode=0, positions=False)
    h, size_z = float(p.h), 0.23
    v, n = scenes.box_mesh((0.5, 0.5, 0.75 + 0.5 * h + 0.5 * size_z), (0.3, 1.2, size_z))
    return v, n, float(np.float32(p.h) / np.float32(2.0)), sc.RESTITUTION


def _collider(cfg):
    if not cfg["collider"]:
        return None
    return _pci_collider() if cfg["pcisph"] else sc.collider_of(cfg["scene"], cfg["math_mode"])


# ---- the ranks ----------------------------------------------------------------------------------------------------

def _worker(rank, world, port, cfg, out):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import torch
    torch.cuda.set_device(0)
    from dieselfluid_amd.slab import SlabDriver
    SlabDriver.REPLAN_EVERY = 4
    pcisph = cfg["pcisph"]
    kw = dict(layers=cfg["layers"]) if cfg["layers"] else {}
    if cfg["every"]:
        kw.update(rebalance_every=cfg["every"])
    vel = (lambda ids, pos: 0.5 * _vel_fn(ids, pos, axis=2)) if pcisph else sc.vel_fn
    drv = SlabDriver.dambreak(cfg["n3"], math_mode=cfg["math_mode"], device=0, axis=sc.AXIS, overlap=cfg["overlap"],
                              native=cfg["native"], pcisph=pcisph, vel_fn=vel, params_hook=_pci_params if pcisph else None,
                              collider=_collider(cfg), collide_index=cfg["index"], **kw)
    assert bool(getattr(drv, "native", False)) == cfg["native"]
    assert drv.overlap == bool(cfg["overlap"])
    core = drv.engine_core
    core.timing_enable(1)
    assert core.get_option("collide_slab") == (1 if cfg["collider"] else 0)
    step = drv.pcisph_step if pcisph else drv.wcsph_step
    hits, planes = [], []
    for _ in range(cfg["steps"]):
        step(1)
        hits.append(int(core.get_option("collide_hits")))
        planes.append((drv.lo, drv.hi))
    res = drv.gather_state(cfg["n3"] ** 3)
    mine = dict(n=drv.engine.n, owned=core.n_owned(), st=drv.engine.status(), hits=hits, planes=planes,
                visits=core.get_option("collide_visits"), launches=core.timing("collide")[1],
                calls=list(core._comm.calls) if cfg["native"] else [],
                pci=(core.stats().pci_iters, core.stats().pci_max_error) if pcisph else None)
    info = [None] * world if rank == 0 else None
    dist.gather_object(mine, info, dst=0)
    if rank == 0:
        with open(out, "wb") as f:
            pickle.dump(dict(pos=res[0], vel=res[1], seen=res[2], info=info), f)
    dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _run(scene, math_mode=0, overlap=False, native=True, collider=True, index=False, layers=None, every=0, pcisph=False,
         steps=sc.STEPS):
    n3 = PCI_N3 if pcisph else sc.SCENES[scene]["n3"]
    world = len(layers) - 1 if layers else sc.SCENES[scene]["world"]
    cfg = dict(scene=scene, n3=n3, math_mode=math_mode, overlap=overlap, native=native, collider=collider, index=index,
               layers=list(layers) if layers else None, every=every, pcisph=pcisph, steps=steps)
    out = os.path.join(tempfile.mkdtemp(prefix="dsl_slab_collider_"), "run.pkl")
    mp.spawn(_worker, args=(world, _free_port(), cfg, out), nprocs=world, join=True)
    with open(out, "rb") as f:
        z = pickle.load(f)
    os.remove(out)
    return z


# ---- the single engine, in pieces ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _single(scene, math_mode=0, pcisph=False, index=False):
    """per step: the positions at its start, after the integrate, after the collide (host order) and the hits; the
    final state"""
    from dieselfluid_amd import SPHEngine
    n3 = PCI_N3 if pcisph else sc.SCENES[scene]["n3"]
    p, pos, vel = sc.initial_state(n3, math_mode)
    cfg = dict(collider=True, pcisph=pcisph, scene=scene, math_mode=math_mode)
    mesh = _collider(cfg)
    if pcisph:
        _pci_params(p)
        vel = (0.5 * vel).astype(np.float32)
    eng = SPHEngine(p)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.reset_forces()
    if index:
        eng.set_option("collide_index", 1)
    if pcisph:
        eng.pcisph_begin()
    else:
        eng.set_collider_mesh(*mesh)
    steps = []
    for _ in range(sc.STEPS):
        start = eng.download("positions")
        if pcisph:
            # DSL_PCI_END_STEP is Update + collide in one call: the mesh is set between the two halves, so that the state
            # in between can be read; the launches, and so the bits, are those of a step with the mesh set throughout
            eng.pcisph_phase(0)
            for _it in range(int(p.pci_max_iters)):
                eng.pcisph_phase(1)
                eng.pcisph_phase(2)
            eng.pcisph_phase(3)
            eng.set_collider_mesh(*mesh)
        else:
            eng.nn()
            eng.density_all()
            eng.force_pass()
        pre = eng.download("positions")
        eng.collide()
        post = eng.download("positions")
        steps.append(dict(start=start, pre=pre, post=post, hits=int(eng.get_option("collide_hits"))))
        if pcisph:
            eng.set_collider_mesh(None)
    st = eng.stats()
    out = dict(pos=eng.download("positions"), vel=eng.download("velocities"), steps=steps, pci=(st.pci_iters, st.pci_max_error))
    eng.close()
    return out


def _moved(step):
    return np.any(step["pre"].view(np.uint32) != step["post"].view(np.uint32), axis=1)


def _assert_conditions(single, planes_by_step, band=None):
    """`planes_by_step`: the interior planes in force when each step packs.  band = (lo, hi): scene C -- hits among the
    particles that start a step inside [lo, hi) along z (band layers) and outside (inner layers), on one rank."""
    world = len(planes_by_step[0]) + 1
    on_rank, cross = np.zeros(world, np.int64), np.zeros(world - 1, np.int64)
    band_hits = inner_hits = 0
    for s, (step, planes) in enumerate(zip(single["steps"], planes_by_step)):
        moved = _moved(step)
        assert step["hits"] == int(moved.sum()) and step["hits"] > 0, f"step {s}: the scene must collide in every step"
        owner = sc.rank_of(step["start"][:, sc.AXIS], planes)
        on_rank += np.bincount(owner[moved], minlength=world)
        for k, q in enumerate(planes):
            cross[k] += int((moved & ((step["pre"][:, sc.AXIS] >= q) != (step["post"][:, sc.AXIS] >= q))).sum())
        if band is not None:
            z0 = step["start"][:, sc.AXIS]
            lower = moved & (owner == 0)
            band_hits += int((lower & (z0 >= band[0])).sum())
            inner_hits += int((lower & (z0 < band[0])).sum())
    assert np.all(on_rank > 0), f"hits per rank {on_rank}: every rank must collide some particle of its own"
    assert np.all(cross > 0), f"cross-backs per plane {cross}: the response must set a particle back across every plane"
    if band is not None:
        assert band_hits > 0 and inner_hits > 0, (band_hits, inner_hits)
    print(f"hits per step {[s['hits'] for s in single['steps']]}, per rank {on_rank.tolist()}, cross-backs {cross.tolist()}")


def _fixed_planes(n3, world, layers=None):
    return [sc.planes_of(n3, world, layers)] * sc.STEPS


def _check_ownership(z, n3):
    assert np.all(z["seen"] == 1)
    assert sum(i["owned"] for i in z["info"]) == n3 ** 3        # every particle owned exactly once
    assert all(i["st"][0] == 0 and i["st"][1] == 0 for i in z["info"])  # no overflow flag, the split margin held


# ---- 1. EXACT, unsplit, native driver --------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,index", [("A", False), ("B", False), ("A", True)], ids=["A", "B", "A_indexed"])
def test_exact_slabs_with_a_collider_are_the_single_engine(scene, index):
    from test_gpu_slab import _assert_identical
    n3, world = sc.SCENES[scene]["n3"], sc.SCENES[scene]["world"]
    single = _single(scene)
    _assert_conditions(single, _fixed_planes(n3, world))
    z = _run(scene, index=index)
    _check_ownership(z, n3)
    _assert_identical("the single engine", z["pos"], z["vel"], single["pos"], single["vel"])
    for s, step in enumerate(single["steps"]):
        assert sum(i["hits"][s] for i in z["info"]) == step["hits"], f"step {s}"
    for i in z["info"]:
        assert i["launches"] == sc.STEPS  # one collide per step and rank
        assert (i["visits"] >= 0) if index else (i["visits"] == -1)


# ---- 2. EXACT, moving planes ----------------------------------------------------------------------------------------

def test_exact_slabs_with_a_collider_and_moving_planes_are_the_single_engine():
    from test_gpu_slab import _assert_identical
    n3, layers = sc.SCENES["B"]["n3"], (0, 4, 20, 24)
    z = _run("B", layers=layers, every=2)
    _check_ownership(z, n3)
    # the planes in force when step s packs: what the ranks report after it (rank r's upper plane is rank r + 1's lower)
    by_step = [[np.float32(z["info"][r]["planes"][s][1]) for r in range(2)] for s in range(sc.STEPS)]
    assert all(np.float32(z["info"][r + 1]["planes"][s][0]) == by_step[s][r] for r in range(2) for s in range(sc.STEPS))
    first = sc.planes_of(n3, 3, layers)
    assert all(any(by_step[s][k] != first[k] for s in range(sc.STEPS)) for k in range(2)), "every interior plane must move"
    single = _single("B")
    _assert_conditions(single, by_step)
    _assert_identical("the single engine", z["pos"], z["vel"], single["pos"], single["vel"])
    for s, step in enumerate(single["steps"]):
        assert sum(i["hits"][s] for i in z["info"]) == step["hits"], f"step {s}"


# ---- 3. EXACT PCISPH ------------------------------------------------------------------------------------------------

def test_pcisph_exact_slabs_with_a_collider_are_the_single_engine():
    from test_gpu_slab import _assert_identical
    single = _single("pci", pcisph=True)
    _assert_conditions(single, _fixed_planes(PCI_N3, 2, PCI_LAYERS))
    z = _run("pci", layers=PCI_LAYERS, pcisph=True)
    _check_ownership(z, PCI_N3)
    iters, err = single["pci"]
    assert all(i["pci"][0] == iters and np.float32(i["pci"][1]) == np.float32(err) for i in z["info"])
    _assert_identical("the single engine", z["pos"], z["vel"], single["pos"], single["vel"])
    for s, step in enumerate(single["steps"]):
        assert sum(i["hits"][s] for i in z["info"]) == step["hits"], f"step {s}"


# ---- 4. FAST, scene C: native driver against the Python protocol ----------------------------------------------------

@pytest.mark.parametrize("overlap", [True, False], ids=["split", "unsplit"])
def test_fast_native_driver_equals_the_python_protocol_with_a_collider(overlap):
    from test_gpu_slab import _bits_equal
    n3 = sc.SCENES["C"]["n3"]
    _assert_conditions(_single("C", math_mode=1), _fixed_planes(n3, 2), band=(0.25, 0.75))
    nat = _run("C", math_mode=1, overlap=overlap)
    py = _run("C", math_mode=1, overlap=overlap, native=False)
    for z in (nat, py):
        _check_ownership(z, n3)
        assert all(i["launches"] == (2 if overlap else 1) * sc.STEPS for i in z["info"])
    assert _bits_equal(py["pos"], nat["pos"]) and _bits_equal(py["vel"], nat["vel"])
    assert [i["hits"] for i in py["info"]] == [i["hits"] for i in nat["info"]]
    assert all(min(i["hits"]) > 0 for i in nat["info"])


# ---- 5. one handle, phase by phase, against collider_ref.respond ----------------------------------------------------

REC, REC_X = 7, 4


@functools.lru_cache(maxsize=None)
def _lower_rank_of_c():
    """scene C's lower rank with the ghosts a neighbour would have sent: the particles below z = 0.5 + 2h"""
    p, pos, vel = sc.initial_state(sc.SCENES["C"]["n3"], 1)
    keep = pos[:, 2] < np.float32(0.5 + 2.0 * p.h)
    ids = np.flatnonzero(keep).astype(np.int32)
    return p, pos[keep], vel[keep], ids


def _handle(mesh, index=False, warm_up=False):
    """warm_up: one step as a single domain first (no collide: dsl_force_pass is one to one), ghost layers included.
    The particles that rise towards the box above the plane then come within its radius in the step that is tested,
    and there are still ghosts above the plane to be marked NaN by it."""
    import torch
    from dieselfluid_amd import SPHEngine
    p, pos, vel, ids = _lower_rank_of_c()
    p.n_particles, p.capacity = pos.shape[0], pos.shape[0] + 1024
    eng = SPHEngine(p)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.set_ids(ids)
    eng.reset_forces()
    eng.timing_enable(1)
    if mesh is not None:
        eng.set_option("collide_slab", 1)
        if index:
            eng.set_option("collide_index", 1)
    if warm_up:
        if mesh is not None:
            eng.set_collider_mesh(*mesh)  # the mesh first, dsl_slab_config second
        eng.nn()
        eng.density_all()
        eng.force_pass()
    eng.slab_config(2, -INF, 0.5)
    if mesh is not None and not warm_up:
        eng.set_collider_mesh(*mesh)  # ... and the other order
    eng.slab_split(2.0 * p.h, 2.0 * p.h)
    eng.nn()
    eng.density_all()
    return eng, p


def _slot_state(eng):
    return (eng.download("positions", sorted_order=True), eng.download("velocities", sorted_order=True), eng.download_ids())


def _band_message(eng, p, n):
    import torch
    buf = torch.zeros((n + 1) * REC + n * REC_X, dtype=torch.int32, device="cuda")
    eng.slab_pack_band(p.h, 0, buf.data_ptr(), n, n, 0)
    return buf


@pytest.mark.parametrize("split,index", [(True, False), (False, False), (True, True)], ids=["split", "unsplit", "split_indexed"])
def test_one_handle_collides_what_the_last_integrate_wrote(split, index):
    mesh = sc.collider_of("C", 1)
    z_eng, p = _handle(None, warm_up=True)
    m_eng, _ = _handle(mesh, index, warm_up=True)
    n = z_eng.n
    if split:
        z_eng.force_pass_split(1)
        _band_message(z_eng, p, n)
        z_eng.force_pass_split(2)
        m_eng.force_pass_split(1)
        m_eng.collide()
        band_hits = int(m_eng.get_option("collide_hits"))
        msg = _band_message(m_eng, p, n)
        m_eng.force_pass_split(2)
        m_eng.collide()
    else:
        z_eng.force_pass()
        m_eng.force_pass()
        m_eng.collide()
    zp, zv, zi = _slot_state(z_eng)
    mp_, mv, mi = _slot_state(m_eng)
    assert np.array_equal(zi, mi)
    rows = np.isfinite(zp).all(axis=1)
    assert 0 < (~rows).sum() < n, "the handle must hold ghosts: NaN rows after the integrate"
    ep, ev = zp.copy(), zv.copy()
    ep[rows], ev[rows], moved = collider_ref.respond(zp[rows], zv[rows], mesh[0], mesh[1], p.dt, mesh[2], mesh[3])
    assert np.array_equal(np.isnan(mp_), np.isnan(zp)), "M's NaN rows are Z's NaN rows"
    assert np.array_equal(mp_[rows].view(np.uint32), ep[rows].view(np.uint32))
    assert np.array_equal(mv[rows].view(np.uint32), ev[rows].view(np.uint32))
    hits = int(m_eng.get_option("collide_hits"))
    assert hits == int(moved.sum()) and hits > 0
    assert m_eng.timing("collide")[1] == (2 if split else 1) and z_eng.timing("collide")[1] == 0
    assert (m_eng.get_option("collide_visits") >= 0) if index else (m_eng.get_option("collide_visits") == -1)
    if split:
        # band + inner: the counters sum over the step's launches, and both launches moved something
        assert 0 < band_hits < hits
        words = msg.cpu().numpy().view(np.uint32)
        nf = int(words[:1].view(np.int32)[0])
        full = words[REC:(nf + 1) * REC].reshape(nf, REC)
        assert nf > 0
        slot_of = {int(g): k for k, g in enumerate(mi)}
        at = np.array([slot_of[int(g)] for g in full[:, 6].view(np.int32)])
        assert np.array_equal(full[:, 0:3], mp_[at].view(np.uint32)), "a band record is not the sender's final state"
        assert np.array_equal(full[:, 3:6], mv[at].view(np.uint32))
        assert np.any(moved[np.flatnonzero(rows).searchsorted(at)]), "a collided particle must be in the band message"
    z_eng.close()
    m_eng.close()


# ---- 6. refusals and life cycle --------------------------------------------------------------------------------------

def test_refusals_name_the_order_and_the_option_guards_both_doors():
    import torch
    from dieselfluid_amd import DslError, SPHEngine
    mesh = sc.collider_of("C", 1)
    p, pos, vel, ids = _lower_rank_of_c()
    # the option at 0: both of today's refusals
    a = SPHEngine(p)
    a.upload("positions", pos)
    a.slab_config(2, -INF, 0.5)
    with pytest.raises(DslError, match="not supported in slab mode"):
        a.set_collider_mesh(*mesh)
    a.close()
    b = SPHEngine(p)
    b.upload("positions", pos)
    b.set_collider_mesh(*mesh)
    with pytest.raises(DslError, match="dsl_slab_config: a collider mesh is not supported in slab mode"):
        b.slab_config(2, -INF, 0.5)
    b.set_option("collide_slab", 1)
    b.slab_config(2, -INF, 0.5)  # ... and with the option the same handle becomes a slab
    with pytest.raises(DslError, match="DSL_OPT_COLLIDE_SLAB cannot go back to 0"):
        b.set_option("collide_slab", 0)
    assert b.get_option("collide_slab") == 1 and b.get_option("collider_triangles") == mesh[0].shape[0]
    with pytest.raises(DslError, match="slab mode"):
        b.collider_query()
    b.close()

    eng, p = _handle(mesh)
    n = eng.n
    order = "integrate -> collide -> pack"
    with pytest.raises(DslError, match=order):  # after the neighbour build, before any integrate
        eng.collide()
    eng.force_pass()
    eng.collide()
    with pytest.raises(DslError, match=order):  # a second collide
        eng.collide()
    eng.nn()
    eng.density_all()
    eng.force_pass()
    buf = torch.zeros((n + 1) * REC + n * REC_X, dtype=torch.int32, device="cuda")
    eng.slab_pack(p.h, 2.0 * p.h, 0, buf.data_ptr(), n, n)
    with pytest.raises(DslError, match=order):  # after a pack
        eng.collide()
    eng.nn()
    eng.density_all()
    eng.force_pass()
    empty = torch.zeros((8 + 1) * REC + 8 * REC_X, dtype=torch.int32, device="cuda")
    eng.slab_append(empty.data_ptr(), 8, 8)
    with pytest.raises(DslError, match=order):  # after an append
        eng.collide()
    eng.nn()
    eng.density_all()
    eng.force_pass_split(1)
    eng.slab_pack_band(p.h, 0, buf.data_ptr(), n, n, 0)
    with pytest.raises(DslError, match=order):  # after the band pack, for that phase
        eng.collide()
    eng.force_pass_split(2)
    eng.collide()  # ... the inner phase is still open
    eng.sync()
    eng.close()


def test_removing_the_mesh_on_a_slab_handle_leaves_a_run_that_never_had_one():
    mesh = sc.collider_of("C", 1)
    z_eng, p = _handle(None)
    m_eng, _ = _handle(mesh)
    m_eng.set_collider_mesh(None)
    assert m_eng.get_option("collider_triangles") == 0 and m_eng.get_option("collide_slab") == 1
    for _ in range(2):
        for e in (z_eng, m_eng):
            e.force_pass_split(1)
            e.collide()  # without a mesh: nothing, in any order
            e.force_pass_split(2)
            e.collide()
            e.nn()
            e.density_all()
    zs, ms = _slot_state(z_eng), _slot_state(m_eng)
    for a, b in zip(zs, ms):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    assert m_eng.timing("collide")[1] == 0
    z_eng.close()
    m_eng.close()


# ---- 7. a run that never sets the option ----------------------------------------------------------------------------

def test_a_run_that_never_sets_the_option_makes_todays_calls_and_launches_no_collide_kernel():
    from test_gpu_slab import STEPS, _assert_identical, _check_exchange_calls, _single as plain_single
    z = _run("A", collider=False, steps=STEPS)
    _check_ownership(z, 16)
    _check_exchange_calls([i["calls"] for i in z["info"]], 2)
    for i in z["info"]:
        assert i["launches"] == 0 and all(h == 0 for h in i["hits"]) and i["visits"] == -1
        assert sum(1 for c in i["calls"] if c == "group_start") == STEPS + 1  # the first exchange, then one per step
    pos, vel = plain_single(16, 0, 1.0)
    _assert_identical("the single engine", z["pos"], z["vel"], pos, vel)
