"""The conditions the scenes of tests/count_change_cases.py have to meet for tests/test_gpu_count_change.py to test what it
names, checked with the oracle alone (the oracle's trajectory stands in for the handle's: DSL_MATH_EXACT is the oracle bit
for bit, DSL_MATH_FAST to 2e-6 of the positions; the GPU tests assert the same conditions again on what they download)."""
import numpy as np
import pytest

import count_change_cases as cc
import sources_ref as sr


@pytest.fixture(scope="module")
def skin_start():
    """the skin tests' state at their count change: six steps from the seeded velocities"""
    p, pos = cc.scene(cc.FAST)
    st = dict(positions=pos, velocities=cc.seeded(p, pos.shape[0]))
    out = cc.oracle_wcsph(p, st, 6)
    return p, pos, dict(positions=out["positions"], velocities=out["velocities"])


@pytest.fixture(scope="module")
def forms_start():
    """the fall-back forms' state at their count change: three steps from rest"""
    p, pos = cc.scene(cc.EXACT)
    out = cc.oracle_wcsph(p, dict(positions=pos, velocities=np.zeros_like(pos)), 3)
    return p, pos, dict(positions=out["positions"], velocities=out["velocities"])


def test_the_append_block_stands_in_the_box_against_the_fluid(skin_start, forms_start):
    block = cc.append_block()
    assert block.shape == (294, 3) and cc.N3 ** 3 + 294 == 4390 and 4390 % 64 != 0 and 4096 < 17 * 256 < 4390 <= cc.CAP
    second = cc.append_block(ix0=7)
    for p, pos, st in (skin_start, forms_start):
        lo, hi = np.array(p.box_min[:]), np.array(p.box_max[:])
        dx, h = 1.0 / cc.N3, float(p.h)
        for b in (block, second):
            assert (b > lo).all() and (b < hi).all()
        assert float(block[:, 1].min()) == pytest.approx(0.5 * dx) and float(block[:, 0].min()) == pytest.approx(1.0 + 0.5 * dx)
        # old particles gain new neighbours: appended particles within h of an original one
        from scipy.spatial import cKDTree
        d, _ = cKDTree(st["positions"].astype(np.float64)).query(block.astype(np.float64))
        near = int((d < h).sum())
        print("appended particles within h of an original one:", near, "closest pair:", cc.min_distance(np.concatenate([st["positions"], block])) / dx, "dx")
        assert near >= 40
        assert cc.min_distance(np.concatenate([st["positions"], block, second])) > 0.5 * dx


def test_the_sink_removes_an_interleaved_share(skin_start, forms_start):
    for (p, pos, st), steps in ((skin_start, cc.K_SKIN), (forms_start, cc.K_FORMS)):
        goes, after = cc.removed(st, cc.sink_slab())
        n = st["positions"].shape[0]
        print("removed", int(goes.sum()), "of", n, "->", n - int(goes.sum()))
        assert cc.removal_is_sound(goes, n)
        # ... and on the state with the block behind it (the third skin sequence): the block stays, its indices move down
        both = cc.appended(st, cc.append_block(), p)
        goes2, after2 = cc.removed(both, cc.sink_slab())
        assert cc.removal_is_sound(goes2, n + 294) and not goes2[n:].any() and (sr.new_index(goes2)[n:] < np.arange(n, n + 294)).all()
        # the oracle alone runs on from there
        out = cc.oracle_wcsph(p, after, steps)
        assert all(np.isfinite(out[k]).all() for k in out) and out["densities"].min() > 0.0
        again = cc.appended(after2, cc.append_block(ix0=7), p)
        assert (again["positions"].shape[0]) % 64 != 0 and again["positions"].shape[0] <= cc.CAP
        out = cc.oracle_wcsph(p, again, steps)
        assert all(np.isfinite(out[k]).all() for k in out)


@pytest.mark.parametrize("skin", [0.07, 0.2])
def test_the_skin_window_after_each_change_holds_rebuilds_and_reuse_steps(skin_start, skin):
    p, pos, st = skin_start
    block, sink = cc.append_block(), cc.sink_slab()
    a = cc.appended(st, block, p)
    b = cc.removed(st, sink)[1]
    c = cc.appended(cc.removed(a, sink)[1], cc.append_block(ix0=7), p)
    for name, state in (("append", a), ("removal", b), ("append, removal, append", c)):
        _, path = cc.oracle_wcsph(p, state, cc.K_SKIN, trajectory=True)
        rb = cc.skin_rebuilds(p, state, path, skin)
        print(f"skin {skin}, {name}: rebuilds at steps {[k for k, r in enumerate(rb) if r]}")
        assert rb[0] and sum(rb) >= 2 and sum(rb) < cc.K_SKIN


def test_an_oracle_given_the_predictor_state_takes_the_step_of_the_run_it_came_from():
    """the PCISPH comparison's premise: positions, velocities, forces and the predictor state are all a step depends on"""
    p, pos = cc.scene(cc.EXACT, cc.SMALL_N3, cc.SMALL_CAP, pci=True)
    st = dict(positions=pos, velocities=np.zeros_like(pos), forces=cc.reset(p, pos.shape[0]), pci_positions=pos,
              pci_velocities=np.zeros_like(pos))
    three, info3 = cc.oracle_pcisph(p, st, 3)
    two, _ = cc.oracle_pcisph(p, st, 2)
    assert not cc.same(two["pci_positions"], two["positions"])  # (the predictor has drifted: the state is not redundant)
    two["forces"] = cc.reset(p, pos.shape[0])
    replay, info = cc.oracle_pcisph(p, two, 1)
    assert info == info3 and info[0] == 3
    for k in three:
        assert cc.same(replay[k], three[k]), k


def test_the_pcisph_scene_crosses_256_and_its_sink_removes_an_interleaved_handful():
    p, pos = cc.scene(cc.EXACT, cc.SMALL_N3, cc.SMALL_CAP, pci=True)
    st = dict(positions=pos, velocities=np.zeros_like(pos), pci_positions=pos, pci_velocities=np.zeros_like(pos))
    names = ("positions", "velocities") + cc.PCI
    out, _ = cc.oracle_pcisph(p, st, 3)
    st = {k: out[k] for k in names}
    emitter, counts, removed = cc.ref_emitter(cc.FACE, first_step=3), [], 0
    for s in range(3, 9):
        if s == 4:
            goes = sr.sink_goes([cc.PCI_SINK], st["positions"])
            idx = np.nonzero(goes)[0]
            assert 5 < goes.sum() < 36 and (~goes[idx[0]:idx[-1]]).any()  # kept and removed indices interleave
        st, gone = cc.driver_changes(st, s, p, emitter, [cc.PCI_SINK], 2)
        removed += gone
        out, info = cc.oracle_pcisph(p, st, 1)
        st = {k: out[k] for k in names}
        counts.append(st["positions"].shape[0])
        assert info[0] == 3 and all(np.isfinite(out[k]).all() for k in out)
    print("counts:", counts, "removed:", removed)
    assert counts[0] < 256 < counts[-1] <= cc.SMALL_CAP and removed > 0 and any(c % 64 for c in counts)
    # the binned sweeps have binning to do: the emitted particles' predictors run ahead of them, so queries sit in other
    # cells and other 4 x 4 x 4-cell tiles than their particles (and a few outside the grid)
    g0 = np.array(p.grid_min[:], dtype=np.float32)
    cell = lambda a: np.floor((a - g0) / np.float32(p.h))
    x, xp = st["positions"], st["pci_positions"]
    other_cell = int(np.any(cell(x) != cell(xp), axis=1).sum())
    other_tile = int(np.any(np.floor(cell(x) / 4) != np.floor(cell(xp) / 4), axis=1).sum())
    print("queries in another cell:", other_cell, "in another tile:", other_tile, "of", x.shape[0])
    assert other_cell > x.shape[0] // 2 and other_tile > x.shape[0] // 5


@pytest.mark.parametrize("collider", ["mesh", "volume"])
def test_the_collider_scenes_hit_while_the_count_moves(collider):
    import collider_ref as cr
    import sdf_ref
    p, pos = cc.scene(cc.EXACT, cc.SMALL_N3, cc.SMALL_CAP)
    if collider == "volume":
        vol = cc.sphere_volume()
        assert np.isfinite(vol).all() and (vol < 0).any()
        respond = lambda x, v: sdf_ref.collider_pass(vol, cc.SPHERE_O, cc.SPHERE_S, x, v, 0.5 * float(p.h), 0.3)
    else:
        verts, normals = cc.plate()
        assert verts.shape == (18, 3, 3)
        respond = lambda x, v: cr.respond(x, v, verts, normals, float(p.dt), 0.1, 0.3)
    st = dict(positions=pos, velocities=np.zeros_like(pos))
    emitter, counts, hits, removed = cc.ref_emitter(cc.FACE), [], [], 0
    for s in range(6):
        st, gone = cc.driver_changes(st, s, p, emitter, [cc.COL_SINK], 2)
        removed += gone
        out = cc.oracle_wcsph(p, st, 1)
        x, v, hit = respond(out["positions"], out["velocities"])
        st = dict(positions=x, velocities=v)
        counts.append(x.shape[0])
        hits.append(int(hit.sum()))
    print("counts:", counts, "hits:", hits, "removed:", removed)
    assert np.isfinite(x).all() and np.isfinite(v).all() and min(hits) > 0 and removed > 20 and len(set(counts)) >= 4


def test_the_recorder_scene_shrinks_to_about_100_and_its_frames_end_in_three_places():
    import record_ref as rr
    p, pos = cc.scene(cc.EXACT, cc.SMALL_N3, cc.SMALL_CAP)
    st = dict(positions=pos, velocities=np.zeros_like(pos))
    emitter = cc.ref_emitter(cc.FACE)
    for s in range(6):
        st, _ = cc.driver_changes(st, s, p, emitter, [], 0)
        out = cc.oracle_wcsph(p, st, 1)
        st = dict(positions=out["positions"], velocities=out["velocities"])
    n = st["positions"].shape[0]
    left = int((~sr.sink_goes([cc.REC_SINK], st["positions"])).sum())
    assert n == 336 and 64 < left < 160
    for enc in (rr.F32, rr.Q16):
        a, b, c = (rr.frame_layout(k, 3, rr.VELOCITY | rr.DENSITY, enc)["bytes"] for k in (n, left, left + 125))
        assert b < c < a
