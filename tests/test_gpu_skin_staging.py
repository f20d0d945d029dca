"""Dealt staging of the skin step's tile kernels (kernels_tiled.hpp "DEALT staging": k_density_list, k_force_list and the
wide candidate sweep hand a tile's quads of four records to lanes by the prefix TileMeta::qprefix).  Every scene forces
the skin (0.07, FAST), is held to the oracle with the bars of tests/test_gpu_skin.py over a window with re-use steps and
rebuilds, must give the same bits twice, and ASSERTS the staged row lengths and per-tile quad counts it is there for --
computed here in numpy from the uploaded positions (the first build sorts exactly those) and the grid geometry, so that
a scene cannot silently stop exercising its path."""
import numpy as np
import pytest

import helpers
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
FAST = 1
SKIN = 0.07
f32 = np.float32
# kernels_tiled.hpp / kernels_skin.hpp: tile of 4 x 4 x 3 cells plus a one-cell halo, staged rows of 6 cells, 4 pad
# records behind each of the 36 row slots, image of 2304 records, 512 quad slots per pass (256 lanes x 2 in the sweep)
TB, TBZ, TH, TROWS, TPAD, TCAP, QSLOTS = 4, 3, 6, 36, 4, 2304, 512


def staged_tiles(p, pos, skin=SKIN):
    """The non-empty tiles of the skin step's grid over `pos`: a list of dicts with the 36 staged rows' lengths
    (`len`, row r = rz * 6 + ry), first slots (`gs`), the tile's quads and staged records (pads included), plus the
    number of particles.  The cell rule is the library's: floor((x - grid_min) / edge) clamped, edge = h (1 + skin),
    float32; slots are the particles in cell order, x fastest."""
    edge = f32(f32(p.h) * (f32(1.0) + f32(skin)))
    inv = f32(1.0) / edge
    gmin = np.array(p.grid_min[:], dtype=f32)
    gmax = np.array(p.grid_max[:], dtype=f32)
    dims = np.maximum(np.ceil((gmax - gmin) * inv).astype(np.int64), 1)
    c = np.floor((pos.astype(f32) - gmin[None, :]) * inv)
    c = np.clip(c, 0, (dims - 1)[None, :]).astype(np.int64)
    nx, ny, nz = (int(d) for d in dims)
    cell = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
    count = np.bincount(cell, minlength=nx * ny * nz)
    start = np.concatenate([[0], np.cumsum(count)])
    cnt3 = count.reshape(nz, ny, nx)
    tiles = []
    for tz in range((nz + TBZ - 1) // TBZ):
        for ty in range((ny + TB - 1) // TB):
            for tx in range((nx + TB - 1) // TB):
                if cnt3[tz * TBZ:(tz + 1) * TBZ, ty * TB:(ty + 1) * TB, tx * TB:(tx + 1) * TB].sum() == 0:
                    continue
                ln, gs = np.zeros(TROWS, dtype=np.int64), np.zeros(TROWS, dtype=np.int64)
                xa, xb = min(max(tx * TB - 1, 0), nx), min(max(tx * TB - 1 + TH, 0), nx)
                for rz in range(TBZ + 2):
                    for ry in range(TH):
                        y, z = ty * TB - 1 + ry, tz * TBZ - 1 + rz
                        if 0 <= y < ny and 0 <= z < nz:
                            row = (z * ny + y) * nx
                            gs[rz * TH + ry] = start[row + xa]
                            ln[rz * TH + ry] = start[row + xb] - start[row + xa]
                tiles.append({"len": ln, "gs": gs, "quads": int(((ln + 3) // 4).sum()),
                              "records": int(ln.sum()) + TPAD * TROWS})
    return tiles, pos.shape[0]


def params_for(n3, n, h_over_dx=2.0):
    from dieselfluid_amd import scenes
    p, _ = scenes.dambreak_scene(n3, h_over_dx=h_over_dx, math_mode=FAST, positions=False)
    p.n_particles = n
    return p


def block_scene(n3, h_over_dx=2.0):
    from dieselfluid_amd import scenes
    return scenes.dambreak_scene(n3, h_over_dx=h_over_dx, math_mode=FAST)


def sheet_scene():
    """Two layers half an h apart in x, staggered by half a spacing in y; lines 0.8 cells apart in y (a cell row holds
    one or two of a layer's) and 1.7 cells apart in z (cell layers with no line at all lie between occupied ones)."""
    n3 = 32
    p = params_for(n3, 0)
    edge = float(p.h) * (1.0 + SKIN)
    ey, ez = 0.8 * edge, 1.7 * edge
    pts = []
    for layer in range(2):
        for j in range(28):
            for k in range(8):
                pts.append((0.30 + layer * 0.5 * float(p.h), 0.05 + (j + 0.5 * layer) * ey, 0.04 + k * ez))
    pos = np.asarray(pts, dtype=f32)
    p.n_particles = pos.shape[0]
    return p, pos


def run_and_check(p, pos, steps=10, expect_overflow=0):
    """`steps` skin steps with seeded velocities (|v| dt up to ~0.012 h per step: s h / 2 is outrun every third step or
    so), twice; the oracle once.  The bars are test_gpu_skin.py's (_check)."""
    from dieselfluid_amd import SPHEngine
    n = pos.shape[0]
    cs = float(np.sqrt(p.eos_w / p.mass))
    vel = helpers.seeded_velocities(n, scale=0.03 * cs)
    frc = np.tile(np.array(p.force_reset[:], dtype=f32), (n, 1))
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, vel=vel, force=frc)
    ora.wcsph_step(steps)
    runs = []
    for _ in range(2):
        eng = SPHEngine(p, device=0)
        eng.upload("positions", pos)
        eng.upload("velocities", vel)
        eng.reset_forces()
        eng.set_option("skin", SKIN)
        eng.wcsph_step(steps)
        assert eng.get_option("skin_steps") == steps
        assert eng.get_option("skin_rebuilds") >= 2
        assert eng.get_option("skin_list_overflow") == expect_overflow
        gx, gv, gr = eng.download("positions"), eng.download("velocities"), eng.download("densities")
        eng.close()
        ex = helpers.rel_err(gx, ora.positions())
        ev = float(np.abs(gv.astype(np.float64) - ora.velocities()).max())
        er = helpers.rel_err(gr, ora.densities())
        print(f"n={n} rel err positions {ex:.3e} (2e-6) velocities abs {ev:.3e} "
              f"({helpers.fast_velocity_tolerance(p, steps):.3e}) densities {er:.3e} (2e-5)")
        assert ex < 2e-6
        assert ev < helpers.fast_velocity_tolerance(p, steps)
        assert er < 2e-5
        runs.append((gx, gv, gr))
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def row_lengths(tiles):
    return np.concatenate([t["len"] for t in tiles])


def test_lattice_rows_of_one_two_and_three_passes():
    """The bench scene in small: jittered 24^3 block, h = 2 dx.  Cells 2.14 dx wide give staged rows of 12-13 lattice
    columns times 2 or 3 lattice lines each way: at most 56 records (one pass of the old dealing), 57-112 (two) and more
    than 112 (three) all occur, and every tile's quads fit one pass of the dealt form."""
    p, pos = block_scene(24)
    tiles, _ = staged_tiles(p, pos)
    ln = row_lengths(tiles)
    assert ((ln > 0) & (ln <= 56)).any() and ((ln > 56) & (ln <= 112)).any() and (ln > 112).any()
    assert len(tiles) > 1 and max(t["quads"] for t in tiles) <= QSLOTS
    assert max(t["records"] for t in tiles) <= TCAP
    run_and_check(p, pos)


def test_denser_block_takes_a_second_pass_of_the_dealing():
    """h = 2.1 dx: a full tile stages about 2050 records in more than 512 quads -- more than the block has quad slots,
    so the dealing takes its second pass -- and still fits the LDS image (no tile takes the global path)."""
    p, pos = block_scene(24, h_over_dx=2.1)
    tiles, _ = staged_tiles(p, pos)
    assert any(t["quads"] > QSLOTS and t["records"] <= TCAP for t in tiles)
    assert max(t["records"] for t in tiles) <= TCAP
    run_and_check(p, pos)


def test_sheet_rows_of_one_two_three_records_and_empty_rows_between():
    """A two-layer sheet: staged rows of 1, 2 and 3 records (a lone partial quad each), and tiles in which rows without
    a record lie between rows that have some -- the quad prefix stands still over them and the row search must skip
    them."""
    p, pos = sheet_scene()
    tiles, _ = staged_tiles(p, pos)
    ln = row_lengths(tiles)
    assert (ln == 1).any() and (ln == 2).any() and (ln == 3).any()

    def gap(t):
        occ = np.flatnonzero(t["len"] > 0)
        return occ.size >= 2 and (t["len"][occ[0]:occ[-1]] == 0).any()
    assert any(gap(t) for t in tiles)
    assert len(tiles) > 1 and max(t["quads"] for t in tiles) <= QSLOTS
    run_and_check(p, pos)


def test_last_staged_row_ends_at_the_arrays_last_slot():
    """A 14^3 block: the staged row that holds the grid's last occupied cells ends at slot n - 1 with a partial last
    quad, whose load reads up to three elements past the particles -- never stored."""
    p, pos = block_scene(14)
    tiles, n = staged_tiles(p, pos)
    ends = [(int(t["gs"][r] + t["len"][r]), int(t["len"][r])) for t in tiles for r in range(TROWS) if t["len"][r] > 0]
    assert any(e == n and l % 4 != 0 for e, l in ends)
    assert max(t["records"] for t in tiles) <= TCAP
    run_and_check(p, pos)
