"""The 12-bit list entries of the skin step (kernels_skin.hpp: a chunk is eight 12-bit record indices in 12 bytes, field k
in bits 12k .. 12k+11, field 0 of a first chunk the count, 0xfff the mark of a particle without a list).  The scenes are
chosen for where such an entry can go wrong, and every property a scene is there for is ASSERTED in numpy from the
uploaded positions -- the first build's reference positions -- and the grid geometry, so that a scene cannot silently
stop exercising it:

  * record indices of 2048 and more (bit 11 of an entry), which only a tile whose image holds more than 2048 of its at
    most 2304 records has;
  * a tile of more than 512 targets: the targets beyond a block share lanes, the shared pass decodes all eight places;
  * lists of 1 to 5 entries in tiles of at most 256 targets (shared pass only): the fields that straddle words at the
    very start of a list, with the count beside them;
  * lists beyond 95 entries next to listed ones: the count field's sentinel;
  * both list builders.

Every case is held to the oracle with the bars of tests/test_gpu_skin.py over a window with re-use steps and rebuilds and
must give the same bits twice.

A jittered 24^3 block at h = 2.1 dx with skin 0.1 -- the first guess for an image beyond 2048 records -- stages MORE than
2304 records in its two middle tiles (1134 particles without lists: the library would leave the skin step).  Used
instead: 24^3 at h = 2.05 dx (images of 2158 and 2095 records, 511 and 542 targets) and 20^3 at h = 2.15 dx (2300 and 2104
records, 700 targets each), both with skin 0.1 and no tile beyond the budget."""
import functools

import numpy as np
import pytest

import helpers
from oracle import pyoracle as po
from test_gpu_list_walk import MAX_FIELDS, walked_fields
from test_gpu_skin_staging import TB, TBZ, TCAP, TH, TPAD, TROWS, block_scene, sheet_scene

pytestmark = pytest.mark.gpu
f32 = np.float32
STEPS = 10
BIT11 = 2048
MIN_ENTRIES = 16  # of a kind, as tests/test_gpu_list_walk.py asks per class

# name: (scene, skin)
SCENES = {
    "image_beyond_2048_records": (lambda: block_scene(24, h_over_dx=2.05), 0.1),
    "image_at_the_budget_700_targets": (lambda: block_scene(20, h_over_dx=2.15), 0.1),
    "two_layer_sheet": (sheet_scene, 0.07),
    "lists_beyond_95_entries": (lambda: block_scene(16, h_over_dx=2.75), 0.07),
}


def tile_images(p, pos, skin):
    """The non-empty tiles of the skin step's grid over `pos`, as the library lays them out: per tile its `targets`
    (particle indices), the number of staged `records` (pads included) and `high`, the particles of staged cells whose
    FIRST record has index >= 2048 -- whatever the order inside a cell, their entries have bit 11 set.  Cells:
    floor((x - grid_min) / edge) clamped, edge = h (1 + skin) in float32; slots are the particles in cell order, x
    fastest; a tile is 4 x 4 x 3 cells and stages 6 x 5 rows of 6 cells, every row slot followed by 4 pad records."""
    edge = f32(f32(p.h) * (f32(1.0) + f32(skin)))
    inv = f32(1.0) / edge
    gmin = np.array(p.grid_min[:], dtype=f32)
    gmax = np.array(p.grid_max[:], dtype=f32)
    dims = np.maximum(np.ceil((gmax - gmin) * inv).astype(np.int64), 1)
    c = np.floor((pos.astype(f32) - gmin[None, :]) * inv)
    c = np.clip(c, 0, (dims - 1)[None, :]).astype(np.int64)
    nx, ny, nz = (int(d) for d in dims)
    cell = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
    order = np.argsort(cell, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=nx * ny * nz))])
    tile_of = ((c[:, 2] // TBZ) * ((ny + TB - 1) // TB) + c[:, 1] // TB) * ((nx + TB - 1) // TB) + c[:, 0] // TB
    tiles = []
    for tz in range((nz + TBZ - 1) // TBZ):
        for ty in range((ny + TB - 1) // TB):
            for tx in range((nx + TB - 1) // TB):
                targets = np.flatnonzero(tile_of == (tz * ((ny + TB - 1) // TB) + ty) * ((nx + TB - 1) // TB) + tx)
                if targets.size == 0:
                    continue
                xa, xb = min(max(tx * TB - 1, 0), nx), min(max(tx * TB - 1 + TH, 0), nx)
                lds, high = 0, []
                for rz in range(TBZ + 2):
                    for ry in range(TH):
                        y, z = ty * TB - 1 + ry, tz * TBZ - 1 + rz
                        if 0 <= y < ny and 0 <= z < nz:
                            row = (z * ny + y) * nx
                            for x in range(xa, xb):
                                if lds + start[row + x] - start[row + xa] >= BIT11:
                                    high.append(order[start[row + x]:start[row + x + 1]])
                            lds += int(start[row + xb] - start[row + xa])
                        lds += TPAD
                lds += TPAD * (TROWS - (TBZ + 2) * TH)  # (the row slots behind the fifth layer are empty)
                tiles.append({"targets": targets, "records": lds,
                              "high": np.concatenate(high) if high else np.zeros(0, dtype=np.int64)})
    return tiles, float(edge)


def entries_with_bit_11(tile, pos, edge):
    """listed pairs (target of the tile, record of index >= 2048), counted 1 % inside the cut-off: the float32 test of
    the build may move a pair or two across h (1 + s)"""
    if tile["records"] <= BIT11 or tile["records"] > TCAP or tile["high"].size == 0:
        return 0
    x = pos.astype(np.float64)
    d = x[tile["targets"]][:, None, :] - x[tile["high"]][None, :, :]
    near = (d * d).sum(axis=2) < (0.99 * edge) ** 2
    near &= tile["targets"][:, None] != tile["high"][None, :]
    return int(near.sum())


def entry_counts(pos, edge):
    from scipy.spatial import cKDTree
    x = pos.astype(np.float64)
    return np.asarray(cKDTree(x).query_ball_point(x, edge, return_length=True), dtype=np.int64) - 1


@functools.lru_cache(maxsize=None)
def scene(name, seeded=True):
    """(params, positions, velocities, the oracle's positions / velocities / densities after STEPS steps): computed once
    per scene and shared, read-only.  `seeded`: velocities that outrun the skin every third step or so; else from rest."""
    make, _ = SCENES[name]
    p, pos = make()
    n = pos.shape[0]
    cs = float(np.sqrt(p.eos_w / p.mass))
    # (|v| dt up to ~0.012 h per step: rebuilds inside the window)
    vel = helpers.seeded_velocities(n, scale=0.03 * cs) if seeded else np.zeros_like(pos)
    frc = np.tile(np.array(p.force_reset[:], dtype=f32), (n, 1))
    ora = po.OracleSPH.from_state(helpers.oracle_params(p), pos, vel=vel, force=frc)
    ora.wcsph_step(STEPS)
    out = (p, pos, vel, ora.positions().copy(), ora.velocities().copy(), ora.densities().copy())
    for a in out[1:]:
        a.setflags(write=False)
    return out


def run(name, list_build=None, expect_overflow=0, seeded=True):
    """STEPS skin steps of the scene; the bars are test_gpu_skin.py's (_check).  Returns the downloaded state."""
    from dieselfluid_amd import SPHEngine
    p, pos, vel, ox, ov, orho = scene(name, seeded)
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.upload("velocities", vel)
    eng.reset_forces()
    eng.set_option("skin", SCENES[name][1])
    if list_build is not None:
        eng.set_option("list_build", list_build)
        assert eng.get_option("list_build") == list_build
    eng.wcsph_step(STEPS)
    assert eng.get_option("skin_steps") == STEPS
    assert (2 if seeded else 1) <= eng.get_option("skin_rebuilds") < STEPS
    assert eng.get_option("skin_list_overflow") == expect_overflow
    gx, gv, gr = eng.download("positions"), eng.download("velocities"), eng.download("densities")
    eng.close()
    ex = helpers.rel_err(gx, ox)
    ev = float(np.abs(gv.astype(np.float64) - ov).max())
    er = helpers.rel_err(gr, orho)
    print(f"{name}: n={pos.shape[0]} rel err positions {ex:.3e} (2e-6) velocities abs {ev:.3e} "
          f"({helpers.fast_velocity_tolerance(p, STEPS):.3e}) densities {er:.3e} (2e-5)")
    assert ex < 2e-6
    assert ev < helpers.fast_velocity_tolerance(p, STEPS)
    assert er < 2e-5
    return gx, gv, gr


def same_bits(a, b):
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("name", ["image_beyond_2048_records", "image_at_the_budget_700_targets"])
def test_entries_with_bit_11_and_a_tile_of_more_than_512_targets(name):
    """A tile whose image holds more than 2048 and at most 2304 records, with targets that list records of index 2048 and
    more; a tile of more than 512 targets, whose last targets take the shared pass; no tile beyond the budget."""
    p, pos = scene(name)[:2]
    tiles, edge = tile_images(p, pos, SCENES[name][1])
    assert max(t["records"] for t in tiles) <= TCAP
    high = [entries_with_bit_11(t, pos, edge) for t in tiles]
    print(f"{name}: (targets, records, entries with bit 11) " +
          str([(t["targets"].size, t["records"], h) for t, h in zip(tiles, high) if t["records"] > BIT11]))
    assert max(high) >= MIN_ENTRIES
    assert any(t["targets"].size > 512 and t["records"] > BIT11 for t in tiles)
    assert int(entry_counts(pos, edge).max()) + 1 < MAX_FIELDS - 2  # (nowhere near: skin_list_overflow stays 0)
    same_bits(run(name), run(name))


def test_lists_of_one_to_five_entries_in_the_shared_pass():
    """The two-layer sheet: no tile has more than 256 targets, so every list is walked by the shared pass, and a list
    holds 1 to 5 entries -- the count, the first entries and the far-away record share the first chunk's first words."""
    name = "two_layer_sheet"
    p, pos = scene(name)[:2]
    tiles, edge = tile_images(p, pos, SCENES[name][1])
    assert len(tiles) > 1 and max(t["targets"].size for t in tiles) <= 256
    x = pos.astype(np.float64)
    from scipy.spatial import cKDTree
    tree = cKDTree(x)
    lo = np.asarray(tree.query_ball_point(x, 0.99 * edge, return_length=True)) - 1
    up = np.asarray(tree.query_ball_point(x, 1.01 * edge, return_length=True)) - 1
    print(f"{name}: entries per list {np.unique(up, return_counts=True)}")
    assert int(lo.min()) >= 1 and int(up.max()) <= 5
    assert np.array_equal(lo, up)  # (no pair near the cut-off: the lengths are what this says)
    assert len(np.unique(up)) >= 3
    same_bits(run(name), run(name))


def test_the_sentinel_marks_lists_beyond_95_entries():
    """The 16^3, h = 2.75 dx block of tests/test_gpu_list_walk.py (skin 0.07): full passes in which some targets' lists do
    not fit and take the global-memory sweep next to listed ones; skin_list_overflow reports them, as that file expects."""
    name = "lists_beyond_95_entries"
    p, pos = scene(name)[:2]
    fields, full, no_image = walked_fields(p, pos, skin=SCENES[name][1])
    assert int(no_image.sum()) * 64 <= pos.shape[0]
    too_long = int((fields[full] > MAX_FIELDS).sum())
    assert too_long >= 16 and too_long * 2 < int(full.sum())
    same_bits(run(name, expect_overflow=1), run(name, expect_overflow=1))


def longest_run(p, pos, skin):
    """the most records in three consecutive cells of a cell row: what a mask-word pair of the sweep stands for"""
    edge = f32(f32(p.h) * (f32(1.0) + f32(skin)))
    inv = f32(1.0) / edge
    gmin = np.array(p.grid_min[:], dtype=f32)
    gmax = np.array(p.grid_max[:], dtype=f32)
    dims = np.maximum(np.ceil((gmax - gmin) * inv).astype(np.int64), 1)
    c = np.floor((pos.astype(f32) - gmin[None, :]) * inv)
    c = np.clip(c, 0, (dims - 1)[None, :]).astype(np.int64)
    cnt = np.zeros((int(dims[2]), int(dims[1]), int(dims[0]) + 2), dtype=np.int64)
    np.add.at(cnt, (c[:, 2], c[:, 1], c[:, 0] + 1), 1)
    return int((cnt[:, :, :-2] + cnt[:, :, 1:-1] + cnt[:, :, 2:]).max())


def test_both_list_builders_pack_the_same_chunks():
    """list_build = 0 (the first form, chunks held in LDS) and 1 (lock step) end in the same bits on a scene with an image
    beyond 2048 records: entries with bit 11, all eight places, the count.  The two builders order the entries of a run
    of more than 64 records differently (kernels_skin.hpp), so the scene has none -- from rest, where the particles
    hardly move in the window: asserted at the uploaded and at the final positions."""
    name = "image_beyond_2048_records"
    p, pos = scene(name, seeded=False)[:2]
    assert longest_run(p, pos, SCENES[name][1]) <= 64
    a, b = run(name, list_build=1, seeded=False), run(name, list_build=0, seeded=False)
    assert longest_run(p, a[0], SCENES[name][1]) <= 64
    same_bits(a, b)
