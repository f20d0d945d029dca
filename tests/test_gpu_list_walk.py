"""The full pass of the list walks (kernels_skin.hpp "Walking a list": k_force_list walks a wave's lists as straight-line
code over up to 12 chunks with an exit after every 32-bit word, k_density_list in a loop with an exit after every half
chunk).  What can go wrong sits at those exits and at the chunk loads around them, so the scenes
are chosen by LIST LENGTH: jittered blocks whose h / dx puts the lists at 3 to 12 chunks, ending in either half of their
last chunk, plus one whose longest lists do not fit (those particles take the global-memory sweep next to listed ones).
Every scene forces the skin (0.07, FAST), is held to the oracle with the bars of tests/test_gpu_skin.py over a window
with re-use steps and rebuilds, must give the same bits twice (run_and_check of tests/test_gpu_skin_staging.py), and
ASSERTS the list lengths it is there for -- computed here in numpy from the uploaded positions, which are the first
build's reference positions -- so that a scene cannot silently stop exercising its exits.

A list's length in fields is 1 + #{ j != i : |x_i - x_j| < h (1 + s) } (field 0 is the count); a wave walks the longest of
its 64 lists, which is one of these values.  Only tiles with more than 256 targets have a full pass, and only tiles whose
staged image fits the LDS budget have lists at all: above h = 2.15 dx a tile in the middle of a large block does not, so
the long lists come from blocks of 16^3 and 18^3, whose tiles all lie at the block's faces.

Lists of one and two chunks need more than 256 targets in a tile with fewer than 16 neighbours each; no block of a
jittered lattice has them, and they are reached through the shared pass (walk_shared) only, which is not the code under
test here."""
import numpy as np
import pytest

from test_gpu_skin_staging import SKIN, TB, TBZ, TCAP, TPAD, TROWS, block_scene, run_and_check

pytestmark = pytest.mark.gpu
f32 = np.float32
FIELDS, MAX_FIELDS = 8, 96  # kernels_skin.hpp: kLEntries, kLMaxChunks * kLEntries
LO, HI = 0, 1  # the list ends in the first / second half of its last chunk

# (block edge in particles, h / dx, targets without a list expected): the (chunks, half) classes the scene must hold
SCENES = {
    "three_to_five_chunks": ((24, 1.9, 0), {(3, LO), (3, HI), (4, HI), (5, LO)}),
    "three_to_seven_chunks": ((24, 2.1, 0), {(3, LO), (3, HI), (4, LO), (4, HI), (5, LO), (5, HI), (6, LO), (6, HI), (7, LO)}),
    "six_to_ten_chunks": ((18, 2.3, 0), {(6, LO), (6, HI), (7, LO), (7, HI), (8, LO), (8, HI), (9, LO), (9, HI), (10, LO)}),
    "ten_to_twelve_chunks": ((16, 2.65, 0), {(10, LO), (10, HI), (11, HI), (12, LO)}),
    "longest_lists_and_overflow": ((16, 2.75, 1), {(11, LO), (12, HI)}),
}
MIN_PARTICLES = 16  # per class: the float32 cut-off test of the build may move a pair or two across h (1 + s)


def walked_fields(p, pos, skin=SKIN):
    """(fields, full, no_image): per particle the length of its list in fields, whether a full pass walks it -- its tile
    holds more than 256 targets and stages at most TCAP records (pads included) -- and whether its tile stages more than
    that.  Cells as in the library: floor((x - grid_min) / edge) clamped, edge = h (1 + skin) in float32; a tile is
    4 x 4 x 3 cells and stages one more cell on every side."""
    from scipy.spatial import cKDTree
    edge = f32(f32(p.h) * (f32(1.0) + f32(skin)))
    inv = f32(1.0) / edge
    gmin = np.array(p.grid_min[:], dtype=f32)
    gmax = np.array(p.grid_max[:], dtype=f32)
    dims = np.maximum(np.ceil((gmax - gmin) * inv).astype(np.int64), 1)
    c = np.floor((pos.astype(f32) - gmin[None, :]) * inv)
    c = np.clip(c, 0, (dims - 1)[None, :]).astype(np.int64)
    nx, ny, nz = (int(d) for d in dims)
    cnt3 = np.zeros((nz, ny, nx), dtype=np.int64)
    np.add.at(cnt3, (c[:, 2], c[:, 1], c[:, 0]), 1)
    shape = ((nz + TBZ - 1) // TBZ, (ny + TB - 1) // TB, (nx + TB - 1) // TB)
    targets, records = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
    for tz, ty, tx in np.ndindex(*shape):
        z, y, x = tz * TBZ, ty * TB, tx * TB
        targets[tz, ty, tx] = cnt3[z:z + TBZ, y:y + TB, x:x + TB].sum()
        records[tz, ty, tx] = cnt3[max(z - 1, 0):z + TBZ + 1, max(y - 1, 0):y + TB + 1, max(x - 1, 0):x + TB + 1].sum() \
            + TPAD * TROWS
    tile = (c[:, 2] // TBZ, c[:, 1] // TB, c[:, 0] // TB)
    x64 = pos.astype(np.float64)
    fields = cKDTree(x64).query_ball_point(x64, float(edge), return_length=True)  # (the particle itself: field 0)
    return np.asarray(fields, dtype=np.int64), (targets[tile] > 256) & (records[tile] <= TCAP), records[tile] > TCAP


def classes_of(fields):
    """{(chunks, half): particles} of lists that fit"""
    f = fields[fields <= MAX_FIELDS]
    keys, counts = np.unique(np.stack([(f + FIELDS - 1) // FIELDS, ((f - 1) % FIELDS) // (FIELDS // 2)], axis=1), axis=0,
                             return_counts=True)
    return {(int(k[0]), int(k[1])): int(n) for k, n in zip(keys, counts)}


def test_the_scenes_cover_three_to_twelve_chunks_in_both_halves():
    """The file's scenes together: every chunk count 3 ... 12, each ending in its first and in its second half."""
    covered = set().union(*(want for _, want in SCENES.values()))
    assert covered >= {(ch, half) for ch in range(3, 13) for half in (LO, HI)}


@pytest.mark.parametrize("name", list(SCENES))
def test_full_pass_walks(name):
    (n3, h_over_dx, overflow), want = SCENES[name]
    p, pos = block_scene(n3, h_over_dx=h_over_dx)
    fields, full, no_image = walked_fields(p, pos)
    # (a tile beyond the LDS budget has no lists; more than one particle in 64 there and the library leaves the skin step)
    assert int(no_image.sum()) * 64 <= pos.shape[0]
    have = classes_of(fields[full])
    print(f"{name}: n={pos.shape[0]} full-pass targets {int(full.sum())} classes {sorted(have.items())} "
          f"beyond {MAX_FIELDS} fields: {int((fields[full] > MAX_FIELDS).sum())}")
    for cls in sorted(want):
        assert have.get(cls, 0) >= MIN_PARTICLES, (cls, have.get(cls, 0))
    too_long = int((fields[full] > MAX_FIELDS).sum())
    if overflow:  # lists beyond 95 entries: those targets take the global-memory sweep in a pass that walks the others' lists
        assert too_long >= MIN_PARTICLES and too_long * 2 < int(full.sum())
    else:
        assert int((fields > MAX_FIELDS - 2).sum()) == 0  # (nowhere near: skin_list_overflow stays 0)
    run_and_check(p, pos, expect_overflow=overflow)
