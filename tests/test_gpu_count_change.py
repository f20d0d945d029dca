"""GPU: the step's fast paths on a handle whose particle count has changed (scenes and expected values:
tests/count_change_cases.py; their conditions: tests/test_count_change_cpu.py).

dsl_particles_append, dsl_particles_remove, the emitters and the sinks make the count a run-time quantity.  A change
invalidates the grid, the masks and the PCISPH query rows, but everything that is sized by capacity -- the skin lists, the
neighbour masks, the third position / velocity set, the cell keys, the tile tables, the recorder's staging frames -- still
holds what the last episode at the old count left past the new n, a removal borrows the neighbour build's scratch and flips
the ping-pong selectors, and an append leaves density 0 in the new slots.  Every test here

  1. brings a handle to a count change through a sequence that leaves such state behind,
  2. downloads the state after the change in host order,
  3. steps the handle K times, and
  4. compares with the CPU oracle stepped K times from that same downloaded state,

and asserts that the path it names was taken (skin step and rebuild counts, binning active, hits > 0, an interleaved removal).

Bars.  EXACT: the oracle's bits.  FAST: positions rel_err < 2e-6, densities < 2e-5, velocities max |dv| <
helpers.fast_velocity_tolerance(p, K) -- the bars of tests/test_gpu_skin.py and tests/test_gpu_variants.py.  Every FAST test
first holds a FRESH handle, given the same downloaded state, to the same bars (the premise: were it to miss them the scene
would be at fault, not the continued handle) and prints the errors of both handles.
"""
import numpy as np
import pytest

import count_change_cases as cc
import helpers
import sources_ref as sr

pytestmark = pytest.mark.gpu

EXACT, FAST = cc.EXACT, cc.FAST
TOL_X, TOL_RHO = 2e-6, 2e-5
STEP_KEYS = ("positions", "velocities", "densities")


# ---- shared pieces -----------------------------------------------------------------------------------------------------

def _engine(p, st, skin=0.0, option=""):
    """a handle of the state `st`: positions, velocities and, when it has them, forces (force_reset otherwise: the forces
    stay implicit, which the skin step needs)"""
    from dieselfluid_amd import SPHEngine
    eng = SPHEngine(p, device=0)
    if option:
        k, v = option.split("=")
        eng.set_option(k, float(v))
    eng.upload("positions", st["positions"])
    if "velocities" in st:
        eng.upload("velocities", st["velocities"])
    if "forces" in st:
        eng.upload("forces", st["forces"])
    else:
        eng.reset_forces()
    for k in cc.PCI:
        if k in st:
            eng.upload(k, st[k])
    if skin:
        eng.set_option("skin", skin)
    return eng


def _state(eng, names=("positions", "velocities")):
    return {k: eng.download(k) for k in names}


def _apply(eng, p, op, names):
    """one count change on the handle, checked against the rule (tests/sources_ref.py) on the state downloaded before it:
    'append' / 'append2' the block (the second one 7 layers further out), 'remove' the sink slab"""
    before = _state(eng, names)
    n = before["positions"].shape[0]
    if op == "remove":
        sink = cc.sink_slab()
        goes, want = cc.removed(before, sink)
        assert cc.removal_is_sound(goes, n), (n, int(goes.sum()))  # (interleaved, 5 % to 25 %, no multiple of 64 left)
        assert eng.add_sink(sink[0], sink[1]) == 0
        assert eng.remove_particles() == int(goes.sum())
        eng.clear_sinks()
    else:
        block = cc.append_block(ix0=7 if op == "append2" else 0)
        want = cc.appended(before, block, p)
        eng.append_particles(block)
    after = _state(eng, names)
    assert eng.n == want["positions"].shape[0] == eng.params.n_particles
    for k in names:
        assert cc.same(after[k], want[k]), (op, k)
    assert np.array_equal(np.sort(eng.download_ids()), np.arange(eng.n))
    return after


def _errors(eng, want):
    gx, gv, gr = (eng.download(k) for k in STEP_KEYS)
    return (helpers.rel_err(gx, want["positions"]), float(np.abs(gv.astype(np.float64) - want["velocities"]).max()),
            helpers.rel_err(gr, want["densities"]))


def _assert_fast(tag, eng, want, p, steps):
    ex, ev, er = _errors(eng, want)
    tol_v = helpers.fast_velocity_tolerance(p, steps)
    print(f"{tag}: positions {ex:.3e} (< {TOL_X:.0e}), velocities {ev:.3e} m/s (< {tol_v:.3e}), densities {er:.3e} (< {TOL_RHO:.0e})")
    assert ex < TOL_X and ev < tol_v and er < TOL_RHO, (tag, ex, ev, er)


def _assert_exact(tag, eng, want):
    for k in STEP_KEYS:
        assert cc.same(eng.download(k), want[k]), (tag, k)


# ---- 1. the skin step after an append, after a removal, and after both --------------------------------------------------

SEQUENCES = {"append": ("append",), "removal": ("remove",), "append_removal_append": ("append", "remove", "append2")}


def _skin_run(skin, ops, check):
    """six skin steps from the seeded velocities, the count changes `ops`, K = 10 skin steps.  The forces are not
    downloaded: that would make the implicit forces explicit and the next step a plain one; after a skin step every force
    is force_reset, which is what the oracle and the fresh handle start from."""
    p, pos = cc.scene(FAST)
    eng = _engine(p, dict(positions=pos, velocities=cc.seeded(p, pos.shape[0])), skin)
    eng.wcsph_step(6)
    assert eng.get_option("skin_steps") == 6 and eng.get_option("skin_rebuilds") >= 1
    for op in ops:
        st = _apply(eng, p, op, ("positions", "velocities"))
    n = eng.n
    assert n % 64 != 0 and n != pos.shape[0]
    built = eng.get_option("skin_rebuilds")
    eng.wcsph_step(cc.K_SKIN)
    steps, rebuilds = eng.get_option("skin_steps"), eng.get_option("skin_rebuilds") - built
    if check:
        print(f"skin {skin}, n = {n}: {steps:.0f} skin steps, {rebuilds:.0f} rebuilds in the {cc.K_SKIN} since the change")
    # every step a skin step; since the change the forced rebuild, at least one more, and at least one re-use step
    assert steps == 6 + cc.K_SKIN and 2 <= rebuilds <= cc.K_SKIN - 1, (steps, rebuilds)
    assert eng.get_option("skin_list_overflow") == 0 and eng.get_option("skin_suspensions") == 0 and eng.n == n
    if check:
        want = cc.oracle_wcsph(p, st, cc.K_SKIN)
        fresh = _engine(cc.with_count(p, n), st, skin)
        fresh.wcsph_step(cc.K_SKIN)
        assert fresh.get_option("skin_steps") == cc.K_SKIN and fresh.get_option("skin_rebuilds") >= 2
        _assert_fast("fresh handle    ", fresh, want, p, cc.K_SKIN)  # the premise
        fresh.close()
        _assert_fast("continued handle", eng, want, p, cc.K_SKIN)
    out = _state(eng, STEP_KEYS)
    eng.close()
    return out


@pytest.mark.parametrize("sequence", list(SEQUENCES))
@pytest.mark.parametrize("skin", [0.07, 0.2])
def test_skin_steps_after_a_count_change_match_the_oracle(skin, sequence):
    """The lists, the masks and the sorted set Z are sized by capacity and hold the old episode's entries past the new n;
    an append gives old particles new neighbours, a removal renumbers the host indices, and after append, removal, append
    the id and state selectors have each flipped an odd number of times.  Measured on an MI355X (fresh / continued handle,
    fraction of the bar): see the table at the end of this file."""
    a = _skin_run(skin, SEQUENCES[sequence], True)
    b = _skin_run(skin, SEQUENCES[sequence], False)
    for k in STEP_KEYS:  # two runs of the sequence end in the same bits
        assert cc.same(a[k], b[k]), k


# ---- 2. the fall-back forms after a count change, and 6. the field operators on that handle -----------------------------

# (tile_queue: 1, the default, turns the queue on from 8M particles; 0 is "never", 2 "always" -- the form that differs at this size)
FORMS = ["density_pair=0", "cell_keys=0", "tile_box=0", f"tile_box={2 | 2 << 8 | 2 << 16}", "persistent_blocks=8", "tile_queue=0",
         "tile_queue=2"]
FORM_NAMES = ("positions", "velocities", "forces")


def _forms_run(option, math_mode):
    """3 steps from rest, the removal, the append, K = 5 steps: (handle, params, the state after the changes)"""
    p, pos = cc.scene(math_mode)
    eng = _engine(p, dict(positions=pos, forces=cc.reset(p, pos.shape[0])), option=option)
    eng.wcsph_step(3)
    _apply(eng, p, "remove", FORM_NAMES)
    st = _apply(eng, p, "append", FORM_NAMES)
    assert eng.n % 64 != 0 and eng.n == st["positions"].shape[0]
    eng.wcsph_step(cc.K_FORMS)
    assert eng.get_option("skin_steps") == 0
    return eng, p, st


@pytest.mark.parametrize("option", FORMS)
@pytest.mark.parametrize("math_mode", [EXACT, FAST], ids=["exact", "fast"])
def test_fallback_forms_after_a_count_change_match_the_oracle(option, math_mode):
    """tests/test_gpu_variants.py's switches (and the tile queue's) at a count that moved down and up again: the
    lane-per-target density kernel, in-cell ordering in two passes, both tile orders, eight workgroups walking all the
    tiles, tiles dealt without the queue and always through it"""
    eng, p, st = _forms_run(option, math_mode)
    k, v = option.split("=")
    assert eng.get_option(k) == float(v)
    want = cc.oracle_wcsph(p, st, cc.K_FORMS)
    if math_mode == EXACT:
        _assert_exact(option, eng, want)
    else:
        fresh = _engine(cc.with_count(p, eng.n), st, option=option)
        fresh.wcsph_step(cc.K_FORMS)
        _assert_fast(f"{option}: fresh handle    ", fresh, want, p, cc.K_FORMS)  # the premise
        fresh.close()
        _assert_fast(f"{option}: continued handle", eng, want, p, cc.K_FORMS)
    eng.close()


# tests/test_gpu_field_ops.py's FAST tolerances: 5e-5 of max |reference|, times 1 for Div and Curl of the velocities and for
# Interpolate(density), times 2 for Laplacian(density)
FIELD_TOL = 5e-5
FIELD_FACTOR = {"div": 1, "curl": 1, "lap_density": 2, "interp_density": 1}


@pytest.mark.parametrize("option", ["", "cell_keys=0"], ids=["default", "cell_keys=0"])
@pytest.mark.parametrize("math_mode", [EXACT, FAST], ids=["exact", "fast"])
def test_field_operators_after_a_count_change(option, math_mode):
    """Div and Curl of the velocities, the Laplacian and Interpolate of the densities on the handle of the test above after
    its last step, against helpers.field_ops_f64 (float64, brute force over all particles) of the downloaded state, at the
    FAST tolerances of tests/test_gpu_field_ops.py in both math modes: 5e-5 of max |reference| for Div, Curl and
    Interpolate, twice that for the Laplacian.  The densities are an input of both sides, so only the operators' own
    float32 arithmetic is in the error.  (The Laplacian's bar is the widest in absolute terms: max |reference| is set by the
    particles on the faces of the free-standing block.)"""
    eng, p, st = _forms_run(option, math_mode)
    n = eng.n
    eng.density_all()
    x, v, rho = eng.download("positions"), eng.download("velocities"), eng.download("densities")
    assert rho.shape == (n,) and rho.min() > 0.0
    q = cc.field_queries(x, float(p.h))
    probe = np.arange(0, n, 7)
    probe = np.unique(np.concatenate([probe, np.arange(n - 294, n, 5)]))  # (appended particles among them)
    want = helpers.field_ops_f64(p, x, v, rho, probe, q)
    got = {"div": eng.field_div("velocities"), "curl": eng.field_curl("velocities"), "lap_density": eng.field_laplacian("densities"),
           "interp_density": eng.field_interpolate(q, "densities")}
    assert got["div"].shape == (n,) and got["curl"].shape == (n, 3) and got["lap_density"].shape == (n,)
    assert got["interp_density"].shape == (q.shape[0],)
    missed = []
    for k, f in FIELD_FACTOR.items():
        g = got[k] if k == "interp_density" else got[k][probe]
        w = want[k]
        assert np.isfinite(g).all() and np.mean(np.abs(w).reshape(len(w), -1).max(axis=1) != 0) > 0.5, k
        scale = float(np.abs(w).max())
        err = float(np.abs(g.astype(np.float64) - w).max())
        print(f"{option or 'default'} {k}: max |device - float64| = {err:.3e}, tolerance {f * FIELD_TOL * scale:.3e} (max |reference| = {scale:.3e})")
        if not err <= f * FIELD_TOL * scale:
            missed.append((k, err, f * FIELD_TOL * scale))
    assert not missed, missed
    eng.close()


# ---- the small scenes: emitters and sinks in the drivers ----------------------------------------------------------------

def _small(math_mode, pci=False):
    p, pos = cc.scene(math_mode, cc.SMALL_N3, cc.SMALL_CAP, pci=pci)
    eng = _engine(p, dict(positions=pos))
    return eng, p, pos


# ---- 3. binned PCISPH after a count change ------------------------------------------------------------------------------

PCI_NAMES = ("positions", "velocities") + cc.PCI
PCI_OPTIONS = ["", "pci_qincr=0", "pci_qrows=0", "pci_qpair=0", "pci_qtiled=0"]


def _pci_handle(math_mode, binning, option):
    eng, p, pos = _small(math_mode, pci=True)
    if option:
        k, v = option.split("=")
        eng.set_option(k, float(v))
    eng.pcisph_begin()
    eng.pcisph_set_binning(binning)
    eng.pcisph_step(3)  # (the query rows are live)
    assert eng.stats().steps == 3 and eng.n == 216
    eng.set_option("sink_every", 2)
    eng.add_emitter(**cc.FACE, first_step=3)
    eng.add_sink(cc.PCI_SINK[0], cc.PCI_SINK[1])
    return eng, p


@pytest.mark.parametrize("option", PCI_OPTIONS)
@pytest.mark.parametrize("binning", [1, 0], ids=["binned", "automatic"])
def test_binned_pcisph_steps_across_a_changing_count_equal_the_oracle(binning, option):
    """Three steps at 216 particles leave the query records, slots, rows and tiles of that count behind; then an emitter
    adds 20 particles a step (216 -> 256 is crossed) and a sink removes an interleaved handful at every second step.  After
    every step positions, velocities, densities, the predictor state, the iteration count and the error are those of an
    oracle that was given the downloaded state -- predictor state included -- with the reference's changes applied.  The
    forces are not downloaded (that would make them explicit and switch the sweep that fills them in off): after a
    step's Update every force is force_reset.  In DSL_MATH_EXACT a binned iteration sorts its queries into one array
    (k_pci_predict_bin, the scan, k_pci_query_scatter, k_pci_density_binned) whatever the DSL_OPT_PCI_* switches say: they
    choose among the DSL_MATH_FAST forms, which the next test runs.  What a case with a switch pins here is exactly that:
    the bits stay the oracle's and the handle holds not a byte more than the default one (no rows, no slots).  The emitted
    particles' predictors run ahead of them at 60 m/s, so the queries do leave their cells and tiles
    (tests/test_count_change_cpu.py), and in the automatic mode the library starts binning on the way (asserted; measured: at
    the look of step 8)."""
    eng, p = _pci_handle(EXACT, binning, option)
    emitter = cc.ref_emitter(cc.FACE, first_step=3)
    counts, removed, active = [], 0, []
    for s in range(3, 9):
        st, gone = cc.driver_changes(_state(eng, PCI_NAMES), s, p, emitter, [cc.PCI_SINK], 2)
        removed += gone
        want, info = cc.oracle_pcisph(p, st, 1)
        eng.pcisph_step(1)
        counts.append(eng.n)
        assert eng.n == st["positions"].shape[0], s
        for k in want:
            assert cc.same(eng.download(k), want[k]), (s, k)
        stats = eng.stats()
        assert (stats.pci_iters, np.float32(stats.pci_max_error)) == info and info[0] == 3, s
        active.append(eng.pcisph_binning()[1])
        assert eng.pcisph_binning() == (binning, True) if binning == 1 else eng.pcisph_binning()[0] == 0
    print("counts:", counts, "removed:", removed, "binning active after each step:", active)
    assert counts[0] < 256 < counts[-1] and removed > 0 and eng.get_option("removed") == removed
    assert active[-1] and (binning == 1 or not active[0])  # (automatic: the library starts binning inside the window)
    assert eng.get_option("emitted") == 120 and any(c % 64 for c in counts)
    if option:  # the switch is set, and DSL_MATH_EXACT holds nothing for it
        k, v = option.split("=")
        assert eng.get_option(k) == float(v)
        default, _ = _pci_handle(EXACT, binning, "")
        default.pcisph_step(6)
        assert eng.get_option("device_bytes") == default.get_option("device_bytes")
        default.close()
    eng.close()


QUERY_ROW_BYTES = 512  # a grid cell's row of 32 query slots, 16 bytes each (kernels_tiled.hpp: kQueryRow)


@pytest.mark.parametrize("option", PCI_OPTIONS, ids=lambda o: o or "default")
def test_fast_binned_pcisph_across_a_changing_count_stays_with_its_unbinned_twin(option):
    """DSL_MATH_FAST, where the DSL_OPT_PCI_* switches select kernels: the default (per-cell query rows kept inside a step, only
    the queries that changed cells moved: qrows, qslot, pci_rows_live), rows filled afresh in every iteration (pci_qincr=0),
    the sorted query array under the pair sweep (pci_qrows=0), one query per lane (pci_qpair=0), the global-memory sweep
    (pci_qtiled=0).  The handle that sorts its queries against the twin that never does (dsl_pcisph_set_binning(-1), the path
    tests/test_gpu_pci_drift.py and tests/test_gpu_sources.py pin), both through the same emitter and sink, to the FAST bars; the
    predictor state to the positions' bar.  The premise: a fresh unbinned handle given the twin's state before the last step
    takes the twin's step.  That the form ran: the query sort is launched in every iteration and never in the twin, the
    switch reads back as set (the library clears pci_qrows itself when the rows do not fit), and the handle holds exactly
    the rows and the slot array its form uses on top of a handle without rows.  The emitted particles' predictors run ahead
    of them at 60 m/s: by the last step more than half of the queries are in another cell than their particle and a fifth in
    another tile (tests/test_count_change_cpu.py)."""
    a, p = _pci_handle(FAST, 1, option)
    b, _ = _pci_handle(FAST, -1, "")
    for e in (a, b):
        e.timing_enable(1)
    a.pcisph_step(5); b.pcisph_step(5)
    st = _state(b, PCI_NAMES)
    a.pcisph_step(1); b.pcisph_step(1)
    assert a.n == b.n > 256 and a.get_option("removed") == b.get_option("removed") > 0
    assert a.pcisph_binning() == (1, True) and b.pcisph_binning() == (-1, False)
    sorts = a.timing("pci_predict")[1], b.timing("pci_predict")[1]
    print("query sorts launched (binned, twin):", sorts)
    assert sorts[0] > 0 and sorts[1] == 0  # (the twin's predictor is part of its sweep)
    flags = {k: a.get_option(k) for k in ("pci_qincr", "pci_qrows", "pci_qpair", "pci_qtiled")}
    assert flags == {k: (0.0 if option == f"{k}=0" else 1.0) for k in flags}, flags
    # what the form holds: rows with pci_qrows, pci_qpair and pci_qtiled all on, the slot array with pci_qincr besides
    norows, _ = _pci_handle(FAST, 1, "pci_qrows=0")
    norows.pcisph_step(6)  # (the same sinks' and layers' arrays)
    extra = a.get_option("device_bytes") - norows.get_option("device_bytes")
    rows, slots = QUERY_ROW_BYTES * a.stats().grid_cells, 4 * cc.SMALL_CAP
    print(f"{option or 'default'}: {extra:.0f} bytes on top of a handle without rows (rows {rows}, slots {slots})")
    # (the rows bring a few counters of their own with them: less than a page)
    held = {"": rows + slots, "pci_qincr=0": rows}.get(option, 0)
    assert held <= extra < held + (4096 if held else 1), (extra, held)
    norows.close()
    want = {k: b.download(k) for k in STEP_KEYS}
    # the premise, on the last step (step 8: the sink looks, then the emitter's layer)
    emitter = cc.ref_emitter(cc.FACE, first_step=8)
    st, _gone = cc.driver_changes(st, 8, p, emitter, [cc.PCI_SINK], 2)
    fresh = _engine(cc.with_count(p, st["positions"].shape[0]), st)
    fresh.pcisph_set_binning(-1)
    fresh.pcisph_step(1)
    _assert_fast("fresh unbinned handle, one step", fresh, want, p, 1)
    fresh.close()
    _assert_fast(f"binned handle ({option or 'default'}), six steps", a, want, p, 6)
    for k in cc.PCI:
        err = helpers.rel_err(a.download(k), b.download(k))
        print(f"{k}: {err:.3e} (< {TOL_X:.0e})")
        assert err < TOL_X, k
    assert a.stats().pci_iters == b.stats().pci_iters == 3
    a.close(); b.close()


# ---- 4. mesh and volume colliders with an emitter and a sink ------------------------------------------------------------

@pytest.mark.parametrize("collider", ["mesh", "mesh_indexed", "volume"])
def test_colliders_with_an_emitter_and_a_sink_take_the_reference_response(collider):
    """EXACT, n3 = 6, the emitter of tests/test_gpu_sources.py aimed at the collider, a sink draining at every second step:
    after every step positions and velocities are the oracle's step of the downloaded state (with the reference's
    removal and layer) followed by the collider's reference response, and the hit count is the reference's."""
    import collider_ref as cr
    import sdf_ref
    eng, p, pos = _small(EXACT)
    dt = float(p.dt)
    radius, rest = 0.5 * float(p.h), 0.3
    if collider == "volume":
        vol = cc.sphere_volume()
        eng.set_collider_volume(vol, cc.SPHERE_O, cc.SPHERE_S, radius=radius, restitution=rest)
        respond = lambda x, v: sdf_ref.collider_pass(vol, cc.SPHERE_O, cc.SPHERE_S, x, v, radius, rest)
    else:
        verts, normals = cc.plate()
        radius = 0.1
        eng.set_collider_mesh(verts, normals, radius, rest)
        if collider == "mesh_indexed":
            eng.set_option("collide_index", 1)
            assert eng.get_option("collide_index") == 1 and eng.get_option("collide_index_cells") > 0
        respond = lambda x, v: cr.respond(x, v, verts, normals, dt, radius, rest)
    eng.set_option("sink_every", 2)
    eng.add_emitter(**cc.FACE)
    eng.add_sink(cc.COL_SINK[0], cc.COL_SINK[1])
    emitter = cc.ref_emitter(cc.FACE)
    counts, hits, removed = [], [], 0
    for s in range(6):
        st, gone = cc.driver_changes(_state(eng), s, p, emitter, [cc.COL_SINK], 2)
        removed += gone
        ora = cc.oracle_wcsph(p, st, 1)
        x, v, hit = respond(ora["positions"], ora["velocities"])
        eng.wcsph_step(1)
        counts.append(eng.n)
        assert eng.n == x.shape[0], s
        assert cc.same(eng.download("positions"), x) and cc.same(eng.download("velocities"), v), s
        assert eng.get_option("collide_hits") == int(hit.sum()), s
        hits.append(int(hit.sum()))
    print("counts:", counts, "hits:", hits, "removed:", removed)
    assert max(hits) > 0 and removed > 20 and eng.get_option("removed") == removed
    assert len(set(counts)) >= 4 and eng.get_option("emitted") == 120
    # the queries after the last step: arrays of the new length, the reference's on the downloaded state
    x, v = eng.download("positions"), eng.download("velocities")
    if collider == "volume":
        got_d, got_n = eng.collider_volume_query()
        want_d, want_n = sdf_ref.collider_query(vol, cc.SPHERE_O, cc.SPHERE_S, x)
        assert got_d.shape == (eng.n,) and got_n.shape == (eng.n, 3)
        assert cc.same(got_d, want_d) and cc.same(got_n, want_n) and np.any(want_d != 0)
    else:
        got = eng.collider_query()
        want = cr.collide(x, v, verts, normals, dt, radius)[:4]
        assert got[0].shape == (eng.n,) and all(g.shape == (eng.n, 3) for g in got[1:])
        assert np.array_equal(got[0], want[0]) and (want[0] >= 0).any()
        for g, w in zip(got[1:], want[1:]):
            assert cc.same(g, w)
    eng.close()


# ---- 5. recorder frames across a shrinking and a growing count ----------------------------------------------------------

def _small_block(nx, origin, dx):
    i, j, k = np.meshgrid(np.arange(nx), np.arange(nx), np.arange(nx), indexing="ij")
    return (np.stack([i, j, k], axis=-1).reshape(-1, 3) * dx + np.asarray(origin)).astype(cc.f32)


@pytest.mark.parametrize("encoding", ["f32", "q16"])
@pytest.mark.parametrize("slots", [1, 4])
def test_recorder_frames_across_a_shrinking_and_a_growing_count(slots, encoding):
    """stride 3, both fields; Q16 with each frame's own bounds.  A frame at 336 particles, one after a removal down to
    about 100 -- a smaller m, planes that end elsewhere and padding in a new place, with slots = 1 inside the staging frame
    that held the larger one -- and one after an append: each is record_ref.build_frame of the state downloaded at that
    moment, byte for byte, and as long as dsl_record_frame_bytes says."""
    import record_ref as rr
    eng, p, pos = _small(EXACT)
    eng.add_emitter(**cc.FACE)
    eng.wcsph_step(6)
    eng.clear_emitters()
    enc = rr.Q16 if encoding == "q16" else rr.F32
    fields = rr.VELOCITY | rr.DENSITY
    spec = eng.set_recorder(stride=3, fields=fields, encoding=enc, slots=slots)
    assert spec.auto_box == (1 if encoding == "q16" else 0)
    want, counts, got = [], [], []

    def record():
        x, v, d = (eng.download(k) for k in STEP_KEYS)
        want.append(rr.build_frame(int(eng.stats().steps), x, v, d, stride=3, fields=fields, encoding=enc, dt=p.dt))
        counts.append(eng.n)
        eng.record_now()
        if slots == 1:  # (the ring's only slot: read before the next frame)
            got.append(eng.read_frame())

    record()
    goes = sr.sink_goes([cc.REC_SINK], eng.download("positions"))
    eng.add_sink(cc.REC_SINK[0], cc.REC_SINK[1])
    assert eng.remove_particles() == int(goes.sum())
    eng.clear_sinks()
    record()
    eng.append_particles(_small_block(5, (1.2, 0.1, 0.1), 1.0 / 6.0), np.tile(np.array([-1.0, 0.0, 0.2], cc.f32), (125, 1)))
    record()
    if slots > 1:
        assert eng.record_poll()[0] == 3
        got = [eng.read_frame() for _ in range(3)]
    print("counts:", counts)
    assert counts[0] == 336 and 64 < counts[1] < 160 and counts[2] == counts[1] + 125
    print("frame bytes:", [len(g) for g in got])
    assert len(got[1]) < len(got[2]) < len(got[0])  # (the planes end in three different places)
    for k in range(3):
        assert len(got[k]) == eng.record_frame_bytes(spec, counts[k]) == rr.frame_layout(counts[k], 3, fields, enc)["bytes"], k
        assert rr.parse_header(got[k])["n_particles"] == counts[k]
        assert got[k] == want[k], (k, counts[k])
    assert eng.record_poll()[2] == 0
    eng.close()


# Measured on an MI355X (the figures the tests print).  In every FAST test the fresh and the continued handle print the same
# figures: from the same state the two take the same steps, which is what a handle without stale state does.
#
#   test                                  positions (< 2e-6)   velocities, m/s (bar)        densities (< 2e-5)   rebuilds in 10
#   skin 0.07, append (n = 4390)          1.7e-7               3.5e-5 (< 7.9e-4)            3.6e-6               3
#   skin 0.07, removal (n = 3575)         2.4e-7               3.0e-5                       3.7e-6               3
#   skin 0.07, append, removal, append    1.6e-7               4.4e-5                       3.8e-6               3
#     (n = 4163)
#   skin 0.2, append                      1.7e-7               5.0e-5                       3.7e-6               2
#   skin 0.2, removal                     2.4e-7               2.5e-5                       4.5e-6               2
#   skin 0.2, append, removal, append     1.3e-7               3.6e-5                       2.9e-6               2
#   fall-back forms, FAST (n = 3857):
#     density_pair=0                      1.3e-7               2.1e-5 (< 4.0e-4)            3.9e-6
#     every other form                    1.3e-7               2.0e-5                       3.4e-6
#   binned PCISPH, FAST, each of 5 forms  0                    0 (< 1.6e-4)                 0
#
#   field operators (n = 3857), max |device - float64| / tolerance: Div 1.5e-6 / 7.0e-4, Curl 1.1e-6 / 1.7e-4, Laplacian
#   0.14 / 62, Interpolate 4.9e-4 / 7.8e-2
#
#   binned PCISPH, FAST: 18 query sorts in the 6 steps (0 in the twin); on top of a handle without rows the default form
#   holds 311424 bytes (rows 307200 + slots 4096 + counters), pci_qincr=0 307264, the three others 0
#
#   counts: PCISPH 236, 238, 258, 269, 289, 295 (41 removed); mesh 164, 184, 196, 216, 216, 236 with 44, 40, 30, 23, 23, 19
#   hits; volume 164, 184, 190, 210, 212, 232 with 61, 49, 28, 27, 28, 29 hits; recorder 336, 106, 231 particles in frames of
#   3456, 1408, 2560 bytes (F32) and 1920, 768, 1408 bytes (Q16)
