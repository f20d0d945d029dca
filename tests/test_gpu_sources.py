"""GPU: sources and sinks (include/dslsph.h: dsl_particles_append, dsl_emitter_add, dsl_emit, dsl_sink_add,
dsl_particles_remove; csrc/sources.hip) against tests/sources_ref.py, the numpy restatement of the build-defined rule, and
against the oracle step by step.  The scene is the n3 = 6 dam-break (216 particles, h = 2 dx, walls on) with capacity 1024:
a few hundred particles, where the count still crosses a wave (64) and a workgroup (256) inside a run.

A step with a changed count is checked by REPLAY: the state before the step, with the reference's layer behind it (or the
reference's compaction of it), is handed to the oracle (or to a fresh handle) as a new system that takes one step.  That
rests on a premise -- a step depends on nothing but positions, velocities and forces (and, for PCISPH, the predictor state)
-- which every such test first asserts on steps without emission, so that a broken premise shows as such.

The capture refusal (a step that would emit or look while the caller's stream is being captured returns
DSL_ERR_UNSUPPORTED) is not exercised here: it would need a capture that is then abandoned with an error inside it; it is
covered by review of sources_step, which asks hipStreamIsCapturing exactly as pci_drift_check does."""
import numpy as np
import pytest

import helpers
import sources_ref as sr
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = 0, 1
CAP = 1024
N0 = 216
# a 5 x 4 face just above the block [0, 1]^3, u and v neither orthogonal nor axis-aligned, moving down at 60 m/s: a layer per
# step is 0.68 dx behind the one before
FACE = dict(origin=(0.15, 1.08, 0.12), u=(0.16, 0.0, 0.012), v=(0.01, 0.004, 0.17), nu=5, nv=4, velocity=(0.0, -60.0, 0.0))
DISC = dict(origin=(1.4, 0.9, 0.1), u=(0.11, 0.002, 0.0), v=(0.003, 0.0, 0.12), nu=7, nv=7, velocity=(1.0, -2.0, 0.5), shape=1)
BUFFERS = ("positions", "velocities", "forces", "densities", "pressures")
PCI = ("pci_positions", "pci_velocities")
INF = float("inf")


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _params(math_mode, n=N0, pci=False):
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(6, math_mode=math_mode)
    p.n_particles = n
    p.capacity = CAP
    if pci:  # (as tests/test_gpu_developed.py sets PCISPH up on this scene: every iteration runs)
        p.pci_max_iters = 3
        p.eos_w = p.eos_w / 3
        p.delta = 1.0e-7
        p.pci_max_error = -1.0
    return p, pos


def _reset(p, n):
    return np.tile(np.array(p.force_reset[:], dtype=f32), (n, 1))


def _dam(math_mode, pci=False):
    from dieselfluid_amd import SPHEngine
    p, pos = _params(math_mode, pci=pci)
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.upload("forces", _reset(p, N0))
    return eng, p, pos


def _state(eng, names=("positions", "velocities")):
    return {k: eng.download(k) for k in names}


def _ref_emitter(d, **kw):
    return sr.Emitter(d["origin"], d["u"], d["v"], d["nu"], d["nv"], d["velocity"], shape=d.get("shape", 0), **kw)


def _oracle_step(p, st, frc=None):
    """one WCSPH step of the oracle from positions, velocities and forces at force_reset"""
    x = st["positions"]
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), x, vel=st["velocities"], force=_reset(p, x.shape[0]) if frc is None else frc)
    ora.wcsph_step(1)
    out = dict(positions=ora.positions(), velocities=ora.velocities(), densities=ora.densities())
    ora.close()
    return out


# ---- 1. one layer's bits ----
@pytest.mark.parametrize("face", [FACE, DISC], ids=["rectangle5x4", "ellipse7x7"])
@pytest.mark.parametrize("how", ["emit", "driver"])
def test_one_layer_is_the_reference_layer_bit_for_bit(face, how):
    eng, p, pos = _dam(EXACT)
    ref = _ref_emitter(face)
    m = ref.m
    assert m == (20 if face is FACE else len(sr.layer_points(7, 7, 1))) and (face is FACE or 20 < m < 49)
    assert eng.add_emitter(**face) == 0 and eng.get_option("emitters") == 1
    if how == "emit":
        eng.density_all()  # (densities on the particles: the new slots must read 0, the old ones keep theirs)
        rho = eng.download("densities")
        eng.emit(0)
        assert eng.n == N0 + m and eng.params.n_particles == N0 + m and eng.get_option("emitted") == m
        assert _same(eng.download("positions"), np.concatenate([pos, ref.points]))
        assert _same(eng.download("velocities"), np.concatenate([np.zeros_like(pos), np.tile(ref.velocity, (m, 1))]))
        assert _same(eng.download("forces"), _reset(p, N0 + m))  # (uploaded, so materialised: force_reset went into the new slots)
        assert _same(eng.download("densities"), np.concatenate([rho, np.zeros(m, f32)])) and rho.all()
        assert _same(eng.download("pressures"), np.zeros(N0 + m, f32))
        assert np.array_equal(np.sort(eng.download_ids()), np.arange(N0 + m))
        assert np.array_equal(eng.download_ids()[N0:], np.arange(N0, N0 + m))
    else:
        eng.wcsph_step(1)
        assert eng.n == N0 + m and eng.stats().steps == 1
        want = _oracle_step(p, dict(positions=np.concatenate([pos, ref.points]),
                                    velocities=np.concatenate([np.zeros_like(pos), np.tile(ref.velocity, (m, 1))])))
        for k in ("positions", "velocities", "densities"):
            assert _same(eng.download(k), want[k]), k
        assert np.array_equal(np.sort(eng.download_ids()), np.arange(N0 + m))
    # dsl_set_params accepts exactly the new count
    q = eng.params
    eng.set_params(q)
    q.n_particles = N0
    from dieselfluid_amd import DslError
    with pytest.raises(DslError):
        eng.set_params(q)
    eng.close()


def test_explicit_append_with_and_without_velocities():
    eng, p, pos = _dam(FAST)
    rng = np.random.default_rng(3)
    a = (rng.random((70, 3)) * 0.3 + np.array([1.5, 0.1, 0.1])).astype(f32)
    b = (rng.random((5, 3)) * 0.3 + np.array([2.5, 0.1, 0.1])).astype(f32)
    va = rng.random((70, 3)).astype(f32)
    eng.append_particles(a, va)
    eng.append_particles(b)
    assert eng.n == N0 + 75 and eng.get_option("emitted") == 0
    assert _same(eng.download("positions"), np.concatenate([pos, a, b]))
    assert _same(eng.download("velocities"), np.concatenate([np.zeros_like(pos), va, np.zeros_like(b)]))
    assert np.array_equal(eng.download_ids(), np.arange(N0 + 75))
    eng.wcsph_step(2)
    assert np.isfinite(eng.download("positions")).all()
    eng.close()


# ---- 2. schedule and grouping ----
def _scheduled(group):
    eng, p, pos = _dam(EXACT)
    eng.add_emitter(**FACE, period=3, first_step=2, max_layers=2)
    eng.add_emitter(**DISC, period=4, first_step=0)
    counts = []
    if group:
        eng.wcsph_step(10)
    else:
        for _ in range(10):
            eng.wcsph_step(1)
            counts.append(eng.n)
    out = _state(eng, ("positions", "velocities", "densities")), eng.n, eng.get_option("emitted"), counts
    eng.close()
    return out


def test_the_schedule_is_the_reference_schedule_and_does_not_depend_on_the_grouping():
    one, n_one, emitted_one, counts = _scheduled(False)
    ten, n_ten, emitted_ten, _ = _scheduled(True)
    sched = sr.Schedule(N0, CAP, [_ref_emitter(FACE, period=3, first_step=2, max_layers=2), _ref_emitter(DISC, period=4, first_step=0)])
    want, fired = [], []
    for s in range(10):
        fired.append(sched.step(s))
        want.append(sched.n)
    assert fired == [[1], [], [0], [], [1], [0], [], [], [1], []]  # (max_layers = 2: nothing at step 8 from emitter 0)
    assert counts == want and n_one == n_ten == sched.n and emitted_one == emitted_ten == sched.emitted
    for k in one:
        assert _same(one[k], ten[k]), k


def test_two_emitters_of_one_step_emit_in_id_order():
    eng, p, pos = _dam(EXACT)
    eng.add_emitter(**DISC)
    eng.add_emitter(**FACE)
    a, b = _ref_emitter(DISC), _ref_emitter(FACE)
    eng.set_option("sink_every", 0)
    eng.emit(0)
    eng.emit(1)
    one = eng.download("positions")
    assert _same(one, np.concatenate([pos, a.points, b.points]))
    eng.close()
    # ... and the driver's first step starts from exactly that state
    drv, _p, _pos = _dam(EXACT)
    drv.add_emitter(**DISC, max_layers=1)
    drv.add_emitter(**FACE, max_layers=1)
    drv.wcsph_step(1)
    vel = np.concatenate([np.zeros_like(pos), np.tile(a.velocity, (a.m, 1)), np.tile(b.velocity, (b.m, 1))])
    want = _oracle_step(p, dict(positions=one, velocities=vel))
    assert _same(drv.download("positions"), want["positions"]) and _same(drv.download("velocities"), want["velocities"])
    drv.close()


# ---- 3. EXACT WCSPH against the oracle, the count crossing 256 ----
def test_exact_wcsph_steps_with_emission_equal_the_oracle_replay_after_every_step():
    eng, p, pos = _dam(EXACT)
    assert p.wcsph_pressure_force and p.wcsph_viscosity
    eng.add_emitter(**FACE, first_step=2)
    ref = _ref_emitter(FACE, first_step=2)
    cont = po.OracleSPH.from_state(helpers.oracle_params(p), pos, force=_reset(p, N0))
    counts = []
    for s in range(8):
        st = _state(eng)
        if s < 2:  # the premise, on steps without emission: a replay from the state equals the continuous run
            cont.wcsph_step(1)
            replay = _oracle_step(p, st)
            for k, got in (("positions", cont.positions()), ("velocities", cont.velocities()), ("densities", cont.densities())):
                assert _same(replay[k], got), ("premise", s, k)
        if ref.due(s):
            st = sr.append_state(st, ref.points, ref.velocity, p.force_reset[:])
        want = _oracle_step(p, st)
        eng.wcsph_step(1)
        counts.append(eng.n)
        for k in ("positions", "velocities", "densities"):
            assert _same(eng.download(k), want[k]), (s, k)
    cont.close()
    assert counts == [216, 216, 236, 256, 276, 296, 316, 336]  # 256 = a workgroup, four waves, is crossed inside the run
    assert eng.get_option("emitted") == 120 and eng.get_option("emit_skipped") == 0
    eng.close()


# ---- 4. FAST: against a fresh handle per step ----
def _fast_run(check):
    from dieselfluid_amd import SPHEngine
    eng, p, pos = _dam(FAST)
    eng.add_emitter(**FACE, first_step=2)
    ref = _ref_emitter(FACE, first_step=2)
    tol = helpers.fast_velocity_tolerance(p, 1)
    for s in range(7):
        st = _state(eng)
        if ref.due(s):
            st = sr.append_state(st, ref.points, ref.velocity, p.force_reset[:])
        eng.wcsph_step(1)
        if check:
            n = st["positions"].shape[0]
            q, _ = _params(FAST, n)
            fresh = SPHEngine(q, device=0)
            fresh.upload("positions", st["positions"])
            fresh.upload("velocities", st["velocities"])
            fresh.upload("forces", _reset(p, n))
            fresh.wcsph_step(1)
            dv = np.abs(eng.download("velocities").astype(np.float64) - fresh.download("velocities")).max()
            print(f"step {s}: n = {n}, max |dv| = {dv:.3e} (bound {tol:.3e})")
            assert eng.n == n and dv < tol, (s, dv, tol)
            fresh.close()
    out = _state(eng, ("positions", "velocities", "densities"))
    assert eng.n == 316
    eng.close()
    return out


def test_fast_steps_with_emission_stay_with_a_fresh_handle_per_step_and_two_runs_agree_bit_for_bit():
    a, b = _fast_run(True), _fast_run(False)
    for k in a:
        assert _same(a[k], b[k]), k


# ---- 5. PCISPH EXACT ----
def _pci_replay(p, st):
    from dieselfluid_amd import SPHEngine
    n = st["positions"].shape[0]
    q, _ = _params(EXACT, n, pci=True)
    fresh = SPHEngine(q, device=0)
    for k in ("positions", "velocities", "forces") + PCI:  # (the PCI uploads start the predictor state)
        fresh.upload(k, st[k])
    fresh.pcisph_set_binning(-1)
    fresh.pcisph_step(1)
    out = _state(fresh, ("positions", "velocities", "densities") + PCI)
    fresh.close()
    return out


def test_exact_pcisph_steps_with_emission_equal_a_fresh_handle_per_step():
    eng, p, pos = _dam(EXACT, pci=True)
    eng.add_emitter(**FACE, first_step=2)
    ref = _ref_emitter(FACE, first_step=2)
    eng.pcisph_begin()
    eng.pcisph_set_binning(-1)
    # new particles' predictor state is their position and velocity
    probe, _p, _pos = _dam(EXACT, pci=True)
    probe.add_emitter(**FACE)
    probe.pcisph_begin()
    probe.pcisph_step(1)
    held = probe.download("pci_positions")
    probe.emit(0)
    assert _same(probe.download("pci_positions"), np.concatenate([held, ref.points]))
    assert _same(probe.download("pci_velocities")[-20:], np.tile(ref.velocity, (20, 1)))
    probe.close()
    names = ("positions", "velocities", "forces") + PCI
    for s in range(5):
        st = _state(eng, names)
        if ref.due(s):  # (s < 2: the premise -- the replay of a state equals the continuous run -- on steps without emission)
            st = sr.append_state(st, ref.points, ref.velocity, p.force_reset[:])
        want = _pci_replay(p, st)
        eng.pcisph_step(1)
        for k in want:
            assert _same(eng.download(k), want[k]), ("premise" if s < 2 else "emission", s, k)
    assert eng.n == 276
    eng.close()


# ---- 6. capacity ----
def test_a_layer_that_does_not_fit_is_skipped_whole_and_lands_once_a_sink_has_made_room():
    from dieselfluid_amd import SPHEngine
    p, pos = _params(FAST)
    p.wcsph_pressure_force = 0  # (256 particles a layer: this test counts, it does not pack fluid)
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    wide = dict(origin=(1.2, 1.5, 0.02), u=(0.15, 0.0, 0.0), v=(0.0, 0.0, 0.06), nu=16, nv=16, velocity=(0.0, -20.0, 0.0))
    eng.add_emitter(**wide)
    sched = sr.Schedule(N0, CAP, [_ref_emitter(wide)])
    for s in range(5):
        eng.wcsph_step(1)
        sched.step(s)
        assert eng.n == sched.n and eng.get_option("emit_skipped") == sched.skipped and eng.get_option("emitted") == sched.emitted
    assert eng.n == 984 and eng.get_option("emit_skipped") == 2  # three layers fitted, two steps went without
    from dieselfluid_amd import DslError
    with pytest.raises(DslError, match="error -3"):
        eng.emit(0)
    assert eng.n == 984
    # an outlet under the emitter: everything right of the block goes at the next look, and the layer of that step lands
    eng.set_option("sink_every", 1)
    eng.add_sink((1.1, -INF, -INF), (INF, INF, INF))
    goes = sr.sink_goes([((1.1, -INF, -INF), (INF, INF, INF), 0)], eng.download("positions"))
    assert goes.sum() == 768
    eng.wcsph_step(1)
    assert eng.n == 984 - 768 + 256 and eng.get_option("removed") == 768 and eng.get_option("emit_skipped") == 2
    assert eng.get_option("emitted") == 4 * 256
    eng.close()


# ---- 7. removal ----
def _block(nx, origin, dx):
    i, j, k = np.meshgrid(np.arange(nx), np.arange(nx), np.arange(nx), indexing="ij")
    return (np.stack([i, j, k], axis=-1).reshape(-1, 3) * dx + np.asarray(origin)).astype(f32)


@pytest.mark.parametrize("driver", ["wcsph", "pcisph"])
def test_removal_moves_every_buffer_with_its_particle(driver):
    pci = driver == "pcisph"
    eng, p, pos = _dam(EXACT, pci=pci)
    eng.append_particles(_block(5, (1.2, 0.1, 0.1), 1.0 / 6.0), np.tile(np.array([-1.0, 0.0, 0.2], f32), (125, 1)))
    names = BUFFERS + (PCI if pci else ())
    if pci:
        eng.pcisph_begin()
        eng.pcisph_step(5)
    else:
        eng.wcsph_step(5)
    assert eng.n == 341 and np.abs(eng.download("velocities")).max() > 0.01
    eng.timing_enable(1)
    # a sink that catches nothing: one launch (the count), no compaction, nothing changes
    before, ids = _state(eng, names), eng.download_ids()
    eng.add_sink((5.0, 5.0, 5.0), (6.0, 6.0, 6.0))
    assert eng.remove_particles() == 0 and eng.timing("sources")[1] == 1 and eng.get_option("removed") == 0
    assert np.array_equal(eng.download_ids(), ids) and all(_same(eng.download(k), before[k]) for k in names)
    eng.clear_sinks()
    counts = [eng.n]
    sinks = [((1.0, -1.0, -1.0), (4.1, 3.0, 2.0), 0),          # an inside box: the appended block
             ((0.5, -INF, -INF), (INF, INF, INF), 0),          # a half-space
             ((0.0, 0.0, 0.0), (0.34, 0.6, 1.1), 1)]           # an outside box: what is not in the corner goes
    for lo, hi, outside in sinks:
        before = _state(eng, names)
        goes = sr.sink_goes([(lo, hi, outside)], before["positions"])
        want = sr.compact(goes, before)
        assert eng.add_sink(lo, hi, bool(outside)) == 0
        assert eng.remove_particles() == int(goes.sum()) > 0
        eng.clear_sinks()
        counts.append(eng.n)
        assert eng.n == want["positions"].shape[0] == eng.params.n_particles
        for k in names:
            assert _same(eng.download(k), want[k]), (counts, k)
        assert np.array_equal(np.sort(eng.download_ids()), np.arange(eng.n))
    print("counts:", counts)
    assert counts[0] > 256 > counts[1] and counts[2] > 64 > counts[3] >= 1  # a workgroup and a wave, crossed downwards
    assert eng.get_option("removed") == counts[0] - counts[3]
    # the handle steps on from there
    (eng.pcisph_step if pci else eng.wcsph_step)(2)
    assert np.isfinite(eng.download("positions")).all()
    # a sink that catches everything leaves the particle with the smallest host index
    first = {k: eng.download(k)[:1] for k in names}
    eng.add_sink((-INF, -INF, -INF), (INF, INF, INF))
    assert eng.remove_particles() == counts[3] - 1 and eng.n == 1
    assert all(_same(eng.download(k), first[k]) for k in names) and list(eng.download_ids()) == [0]
    eng.close()


def test_a_nan_position_is_removed_by_an_outside_sink_and_kept_by_an_inside_one():
    from dieselfluid_amd import SPHEngine
    p, pos = _params(EXACT)
    bad = pos.copy()
    bad[7, 1] = np.nan
    bad[130] = np.nan
    eng = SPHEngine(p, device=0)
    eng.upload("positions", bad)
    eng.add_sink((-INF, -INF, -INF), (INF, INF, INF))      # inside, everywhere: a NaN is never inside, so only the NaNs stay
    goes = sr.sink_goes([((-INF,) * 3, (INF,) * 3, 0)], bad)
    assert list(np.nonzero(~goes)[0]) == [7, 130]
    assert eng.remove_particles() == N0 - 2
    got = eng.download("positions")
    assert got.shape == (2, 3) and np.array_equal(np.isnan(got), np.isnan(bad[[7, 130]]))
    eng.close()
    eng = SPHEngine(p, device=0)
    eng.upload("positions", bad)
    eng.add_sink((-1.0, -1.0, -1.0), (5.0, 5.0, 5.0), outside=True)  # before any step
    assert eng.remove_particles() == 2 and eng.n == N0 - 2
    assert _same(eng.download("positions"), np.delete(pos, [7, 130], axis=0))
    eng.close()


# ---- 8. ten EXACT steps after a removal ----
def test_ten_exact_steps_after_a_removal_equal_the_oracle_replay():
    eng, p, pos = _dam(EXACT)
    eng.wcsph_step(3)
    st = _state(eng)
    goes = sr.sink_goes([((0.5, -INF, -INF), (INF, INF, INF), 0)], st["positions"])
    eng.add_sink((0.5, -INF, -INF), (INF, INF, INF))
    assert eng.remove_particles() == int(goes.sum()) and 64 < eng.n < N0
    eng.clear_sinks()
    assert _same(eng.download("positions"), sr.compact(goes, st)["positions"])
    for s in range(10):
        want = _oracle_step(p, _state(eng))
        eng.wcsph_step(1)
        for k in ("positions", "velocities", "densities"):
            assert _same(eng.download(k), want[k]), (s, k)
    eng.close()


# ---- 9. sinks in the driver ----
def _sunk(group, every=4):
    eng, p, pos = _dam(EXACT)
    eng.set_option("sink_every", every)
    assert eng.get_option("sink_every") == every and eng.get_option("sinks") == 0
    eng.wcsph_step(1)
    eng.add_sink((-INF, -INF, -INF), (0.2, INF, INF))  # the first lattice layer in x sits inside from now on
    counts, at4 = [], None
    if group:
        eng.wcsph_step(9)
    else:
        for s in range(1, 10):
            if s == 4:
                at4 = eng.download("positions")
            eng.wcsph_step(1)
            counts.append(eng.n)
    out = _state(eng, ("positions", "velocities", "densities")), eng.n, eng.get_option("removed"), counts, at4
    eng.close()
    return out


def test_sinks_in_the_driver_act_at_every_fourth_step_whatever_the_grouping():
    one, n_one, removed_one, counts, at4 = _sunk(False)
    ten, n_ten, removed_ten, _, _ = _sunk(True)
    goes4 = int(sr.sink_goes([((-INF,) * 3, (0.2, INF, INF), 0)], at4).sum())
    assert goes4 >= 36
    # steps 1, 2, 3 (the sink exists, no look): the particles inside it live on; step 4 looks; step 8 looks again
    assert counts[:3] == [N0] * 3 and counts[3] == N0 - goes4 and counts[3:7] == [counts[3]] * 4
    assert n_one == n_ten and removed_one == removed_ten == N0 - n_one
    for k in one:
        assert _same(one[k], ten[k]), k
    # every = 0: the drivers never look; dsl_particles_remove does
    eng, p, pos = _dam(EXACT)
    eng.set_option("sink_every", 0)
    eng.add_sink((-INF, -INF, -INF), (0.2, INF, INF))
    eng.wcsph_step(9)
    assert eng.n == N0 and eng.get_option("removed") == 0
    assert eng.remove_particles() > 0 and eng.n < N0
    from dieselfluid_amd import DslError
    with pytest.raises(DslError, match="error -1"):
        eng.set_option("sink_every", -1)
    eng.close()


# ---- 10. a dynamic body while the count crosses 256 ----
def test_a_dynamic_body_takes_the_reference_impulse_while_the_count_crosses_256():
    import bodies_ref as br
    import test_gpu_bodies as bodies_case
    eng, p, pos = _dam(EXACT)
    bodies = bodies_case._dynamic_bodies(p, 1)
    bodies_case._add(eng, bodies[0])
    eng.add_emitter(**FACE)
    ref = _ref_emitter(FACE)
    acc = np.zeros((1, 6), dtype=f32)
    responses = 0
    for s in range(4):
        st = sr.append_state(_state(eng), ref.points, ref.velocity, p.force_reset[:])
        ora = _oracle_step(p, st)
        eng.wcsph_step(1)
        ids = eng.download_ids()  # (the pass ran on the slots the step's sort left)
        x, v, hit, responded, acc = br.step(bodies, ora["positions"], ora["velocities"], float(p.mass), ids, float(p.dt), acc)
        responses += int(responded.sum())
        assert _same(eng.download("positions"), x) and _same(eng.download("velocities"), v), s
        assert bodies_case._state_is(eng, 0, bodies[0]["state"]) and _same(bodies_case._acc(eng, 0), acc[0]), s
        assert eng.get_option("collide_hits") == int(hit.sum())
    assert eng.n == 296 and responses > 0 and acc[0].any()
    eng.close()


# ---- 11. a field volume after an emission ----
@pytest.mark.parametrize("math_mode", [EXACT, FAST])
def test_a_field_volume_after_an_emission_is_field_interpolate_on_the_same_state(math_mode):
    from dieselfluid_amd import scenes
    eng, p, pos = _dam(math_mode)
    eng.add_emitter(**FACE, max_layers=3)
    eng.wcsph_step(3)
    eng.clear_emitters()
    assert eng.n == 276
    eng.density_all()
    origin, step, dims = (-0.1, -0.1, -0.1), 1.0 / 6.0, (9, 9, 8)
    vol = eng.field_volume(origin, step, dims, "densities")
    pts = scenes.volume_points(origin, step, dims)
    assert _same(vol.reshape(-1), eng.field_interpolate(pts, "densities")) and vol.any()
    # ... and the emitted particles are in it: around the face's first layers the field is not zero
    near = eng.field_interpolate(eng.download("positions")[-20:], "densities")
    assert near.all()
    eng.close()


# ---- 12. off means off ----
# DSL_OPT_DEVICE_BYTES of this scene's handle (216 particles, capacity 1024, EXACT, no PCISPH) as the commit before sources
# and sinks reports it: nothing of theirs is allocated until one of their calls is made
PARENT_DEVICE_BYTES = 787036


def test_a_handle_that_never_makes_a_new_call_launches_and_allocates_nothing():
    eng, p, pos = _dam(EXACT)
    fresh = eng.get_option("device_bytes")
    eng.timing_enable(1)
    eng.wcsph_step(10)
    assert eng.timing("sources") == (0.0, 0) and eng.timing("density")[1] == 10
    print("device bytes:", fresh)
    assert eng.get_option("device_bytes") == fresh
    assert fresh == PARENT_DEVICE_BYTES
    for name in ("emitters", "sinks", "emitted", "emit_skipped", "removed"):
        assert eng.get_option(name) == 0
    assert eng.get_option("sink_every") == 8
    # what the calls allocate is counted, and the clear calls give it back
    eng.add_emitter(**DISC)
    eng.add_sink((5.0, 5.0, 5.0), (6.0, 6.0, 6.0))
    eng.add_sink((-INF, -INF, -INF), (0.2, INF, INF))
    assert eng.get_option("device_bytes") == fresh + 4 * len(sr.layer_points(7, 7, 1))
    assert eng.remove_particles() > 0
    assert eng.get_option("device_bytes") > fresh + 4 * len(sr.layer_points(7, 7, 1))
    eng.clear_emitters()
    eng.clear_sinks()
    assert eng.get_option("device_bytes") == fresh and eng.get_option("emitters") == eng.get_option("sinks") == 0
    eng.close()


# ---- 13. the skin step ----
def test_no_skin_step_while_an_emitter_exists():
    from dieselfluid_amd import SPHEngine, scenes
    p, pos = scenes.dambreak_scene(16, math_mode=FAST)  # (the n3 = 6 scene has too few tiles for the skin step to be usable)
    p.capacity = p.n_particles + 64
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.reset_forces()
    eng.set_option("skin", 0.07)
    eng.add_emitter(**FACE, first_step=1000)  # (it exists; it never emits here)
    eng.wcsph_step(4)
    assert eng.get_option("skin_steps") == 0
    eng.clear_emitters()
    eng.wcsph_step(4)
    assert eng.get_option("skin_steps") > 0
    eng.add_sink((5.0, 5.0, 5.0), (6.0, 6.0, 6.0))  # (settles the episode) ... and a sink holds it back as well
    taken = eng.get_option("skin_steps")
    eng.wcsph_step(4)
    assert eng.get_option("skin_steps") == taken and eng.n == p.n_particles
    eng.close()


# ---- 14. refusals ----
def _unchanged(eng, n, pos):
    return (eng.n == n and eng.get_option("emitters") == 0 and eng.get_option("sinks") == 0 and eng.get_option("emitted") == 0
            and eng.get_option("removed") == 0 and _same(eng.download("positions", sorted_order=True)[:pos.shape[0]], pos))


def _every_new_call_is_refused(eng, code):
    from dieselfluid_amd import DslError
    calls = [lambda: eng.append_particles([[0.5, 0.5, 0.5]]), lambda: eng.add_emitter(**FACE), lambda: eng.emit(0),
             lambda: eng.add_sink((0, 0, 0), (1, 1, 1)), lambda: eng.remove_particles()]
    for call in calls:
        with pytest.raises(DslError, match=f"error {code}"):
            call()


def test_handles_that_cannot_have_sources_refuse_them_and_stay_as_they_were():
    from dieselfluid_amd import DslError, SPHEngine, scenes
    from dieselfluid_amd.engine import reference_params
    # a slab handle
    eng, p, pos = _dam(EXACT)
    eng.slab_config(0, 0.0, 2.0)
    _every_new_call_is_refused(eng, -4)
    assert "slab" in eng._L.dsl_last_error(eng._h).decode()
    eng.slab_config(-1, 0.0, 1.0)
    assert _unchanged(eng, N0, pos)
    eng.add_sink((0, 0, 0), (1, 1, 1))
    with pytest.raises(DslError, match="error -4"):
        eng.slab_config(0, 0.0, 2.0)
    eng.clear_sinks()
    eng.add_emitter(**FACE)
    with pytest.raises(DslError, match="error -4"):
        eng.slab_config(0, 0.0, 2.0)
    eng.close()
    # DSL_NEIGH_LSH_REF
    q = reference_params(6)
    q.neigh_mode, q.math_mode, q.capacity = 0, 0, CAP
    eng = SPHEngine(q, device=0)
    lat = scenes.lattice_positions(6)
    eng.upload("positions", lat)
    _every_new_call_is_refused(eng, -4)
    assert "LSH" in eng._L.dsl_last_error(eng._h).decode() and _unchanged(eng, N0, lat)
    eng.close()
    # boundary particles: fluid stays in front
    eng, p, pos = _dam(EXACT)
    eng.add_boundary_particles(_block(2, (3.0, 0.1, 0.1), 0.1))
    _every_new_call_is_refused(eng, -4)
    assert "boundary" in eng._L.dsl_last_error(eng._h).decode() and eng.n == N0 + 8 and eng.get_option("sinks") == 0
    eng.close()
    eng, p, pos = _dam(EXACT)
    eng.add_sink((5.0, 5.0, 5.0), (6.0, 6.0, 6.0))
    with pytest.raises(DslError, match="error -4"):
        eng.add_boundary_particles(_block(2, (3.0, 0.1, 0.1), 0.1))
    eng.clear_sinks()
    eng.append_particles([[2.0, 0.5, 0.5]])
    with pytest.raises(DslError, match="error -4"):  # (the count has changed)
        eng.add_boundary_particles(_block(2, (3.0, 0.1, 0.1), 0.1))
    assert eng.n == N0 + 1 and eng.params.n_boundary == 0
    eng.close()
    # after dsl_set_ids
    eng, p, pos = _dam(EXACT)
    eng.set_ids(np.arange(N0, dtype=np.int32) + 1000)
    _every_new_call_is_refused(eng, -4)
    assert "dsl_set_ids" in eng._L.dsl_last_error(eng._h).decode()
    assert _unchanged(eng, N0, pos)
    eng.close()


def test_bad_arguments_are_refused_and_change_nothing():
    from dieselfluid_amd import DslError
    eng, p, pos = _dam(EXACT)
    nan = float("nan")
    bad_emitters = [dict(nu=0), dict(nv=0), dict(period=0), dict(nu=1025, nv=1024), dict(u=(0.0, 0.0, 0.0)), dict(v=(0.0, 0.0, 0.0)),
                    dict(origin=(nan, 0.0, 0.0)), dict(u=(INF, 0.0, 0.0)), dict(velocity=(0.0, nan, 0.0)), dict(first_step=-1),
                    dict(max_layers=-1), dict(shape=2), dict(shape=-1)]
    for bad in bad_emitters:
        with pytest.raises(DslError, match="error -1"):
            eng.add_emitter(**{**FACE, **bad})
    bad_sinks = [((nan, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, nan, 1)), ((0, 2, 0), (1, 1, 1))]
    for lo, hi in bad_sinks:
        with pytest.raises(DslError, match="error -1"):
            eng.add_sink(lo, hi)
    with pytest.raises(DslError, match="error -1"):
        eng.emit(0)  # an unknown id
    for bad in (np.zeros((0, 3), f32), [[nan, 0.0, 0.0]], [[0.0, INF, 0.0]]):
        with pytest.raises(DslError, match="error -1"):
            eng.append_particles(bad)
    with pytest.raises(DslError, match="error -1"):
        eng.append_particles([[0.5, 0.5, 0.5]], [[0.0, nan, 0.0]])
    with pytest.raises(DslError, match="error -3"):
        eng.append_particles(np.full((CAP - N0 + 1, 3), 0.5, f32))
    assert "capacity" in eng._L.dsl_last_error(eng._h).decode()
    assert _unchanged(eng, N0, pos) and eng.remove_particles() == 0
    # the ninth emitter and the ninth sink; an emitter whose layers are used up
    for k in range(8):
        assert eng.add_emitter(**FACE, max_layers=1) == k and eng.add_sink((5.0, 5.0, 5.0), (6.0, 6.0, 6.0)) == k
    with pytest.raises(DslError, match="error -1"):
        eng.add_emitter(**FACE)
    with pytest.raises(DslError, match="error -1"):
        eng.add_sink((5.0, 5.0, 5.0), (6.0, 6.0, 6.0))
    assert eng.get_option("emitters") == 8 and eng.get_option("sinks") == 8 and eng.n == N0
    eng.emit(3)
    with pytest.raises(DslError, match="error -1"):
        eng.emit(3)
    with pytest.raises(DslError, match="error -1"):
        eng.emit(8)
    assert eng.n == N0 + 20
    # the largest face there is: 2^20 points are accepted (and would not fit this handle)
    eng.clear_emitters()
    assert eng.add_emitter(**{**FACE, "nu": 1024, "nv": 1024}) == 0
    with pytest.raises(DslError, match="error -3"):
        eng.emit(0)
    eng.close()
