"""GPU: the slab band messages, record by record.

dsl_slab_pack / dsl_slab_pack_band (k_slab_count, k_slab_offsets, k_slab_write), dsl_slab_append / dsl_slab_append2
(k_slab_append, k_slab_bump) and dsl_get_count (k_count_owned) against numpy.  A message is a copy -- header counts,
then records in slot order -- so every comparison here is an equality of uint32 words: no tolerance anywhere, and no
record is left out of a comparison.  One process, no transport: a single engine is configured as a slab of a block it
holds entirely, the particles outside [lo, hi) are ghosts by definition.

Every message buffer is filled with helpers.SLAB_SENTINEL before a pack and is allocated for the UNclamped record
counts plus a guard tail, so a kernel that writes a record it should have dropped still writes inside the allocation
and the test fails by comparison.

Out of scope: dsl_slab_image_shift is reachable through the attached driver only;
test_gpu_slab.py::test_native_step_driver_matches_the_python_protocol covers it."""
import numpy as np
import pytest
import torch

from helpers import SLAB_SENTINEL, slab_message_reference
from test_slab_cpu import _vel_fn

pytestmark = pytest.mark.gpu

GUARD = 64                  # words behind every message that nobody may touch
REC, REC_PCI, REC_X = 7, 13, 4
SPLIT_BAND, SPLIT_INNER = 1, 2
INF = float("inf")
# the unit scene: h = 1 and dyadic planes and widths, so every threshold is exact in float32
LO, HI, WF, W = -4.0, 4.0, 1.0, 2.0      # thresholds -3, -2, 2, 3
HALF = 8.0                                # grid box [-8, 8]^3: 16^3 = 4096 cells


# ---- plumbing --------------------------------------------------------------------------------------------------

def _unit_params(n, capacity=0, math_mode=1):
    from dieselfluid_amd import scenes
    p, _ = scenes.dambreak_scene(4, math_mode=math_mode, positions=False)
    p.n_particles, p.capacity, p.h = int(n), int(capacity), 1.0
    for a in range(3):
        p.box_min[a] = p.grid_min[a] = -HALF
        p.box_max[a] = p.grid_max[a] = HALF
    return p


def _engine(p, pos, vel=None, ids=None, slab=None):
    """an engine on torch's current stream (the message tensors live there), loaded and configured as a slab"""
    from dieselfluid_amd import SPHEngine
    eng = SPHEngine(p)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.upload("positions", pos)
    if vel is not None:
        eng.upload("velocities", vel)
    if ids is not None:
        eng.set_ids(ids)
    eng.reset_forces()
    if slab is not None:
        eng.slab_config(*slab)
    return eng


def _state(eng):
    """(positions, velocities, ids) in slot order"""
    return (eng.download("positions", sorted_order=True), eng.download("velocities", sorted_order=True),
            eng.download_ids())


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Buf:
    """a message buffer: a torch device tensor used as plain memory, sentinel-filled"""

    def __init__(self, words):
        self.t = torch.empty(int(words), dtype=torch.int32, device="cuda")
        self.fill()

    def fill(self):
        self.t.fill_(int(SLAB_SENTINEL))

    def set(self, words):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(words).view(np.int32)))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def words(self):
        return self.t.cpu().numpy().view(np.uint32)  # (synchronises torch's current stream: the engine's)


def _alloc_words(counts, cap_full, cap_x, rec):
    """the buffer size rule: room for every record the state holds, whatever the capacities say, plus the guard"""
    nf = max(cap_full, counts["lo"][0], counts["hi"][0])
    nx = max(cap_x, counts["lo"][1], counts["hi"][1])
    return (nf + 1) * rec + nx * REC_X + GUARD


def _counts(state, axis, lo, hi, wf, w):
    r = slab_message_reference(*state, axis, lo, hi, wf, w, 0, 0)
    return {s: r[s]["counts"] for s in ("lo", "hi")}


def _assert_message(got, side_ref, what):
    """the whole allocation: header, records, and the sentinel everywhere else, guard tail included"""
    want = np.full(got.shape, SLAB_SENTINEL, np.uint32)
    want[:side_ref["words"].size] = side_ref["words"]
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError(f"{what}: {bad.size} of {got.size} words differ, the first at word {bad[0]}: "
                             f"got {got[bad[0]]:#010x}, want {want[bad[0]]:#010x}; header got "
                             f"{got[:2].view(np.int32).tolist()}, want {want[:2].view(np.int32).tolist()}")


def _pack_and_check(eng, axis, lo, hi, wf, w, caps=None, want=(True, True), rec=REC, pci=(None, None), what=""):
    """packs the current state and compares both buffers with the reference; returns (reference, state, words)"""
    state = _state(eng)
    counts = _counts(state, axis, lo, hi, wf, w)
    if caps is None:  # a little more than needed: unused records exist and must stay untouched
        caps = (max(counts["lo"][0], counts["hi"][0]) + 3, max(counts["lo"][1], counts["hi"][1]) + 5)
    ref = slab_message_reference(*state, axis, lo, hi, wf, w, caps[0], caps[1], rec=rec, pci_pos=pci[0], pci_vel=pci[1])
    bufs = [_Buf(_alloc_words(counts, caps[0], caps[1], rec)) for _ in range(2)]
    ptrs = [b.ptr if on else 0 for b, on in zip(bufs, want)]
    eng.slab_pack(wf, w, ptrs[0], ptrs[1], caps[0], caps[1])
    eng.sync()
    words = {}
    for side, b, on in zip(("lo", "hi"), bufs, want):
        words[side] = b.words()
        if on:
            _assert_message(words[side], ref[side], f"{what} {side} message")
        else:
            assert np.all(words[side] == SLAB_SENTINEL), f"{what}: the {side} buffer was not asked for but was written"
    return ref, state, words


def _cloud(n, seed, lo=-5.0, hi=5.0):
    """n seeded particles, uniform in [lo, hi)^3, with velocities and shuffled global ids"""
    rng = np.random.default_rng(seed)
    pos = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    vel = (rng.random((n, 3)) - 0.5).astype(np.float32)
    ids = (rng.permutation(n) * 3 + 11).astype(np.int32)
    return pos, vel, ids


# ---- pack: dsl_slab_pack ---------------------------------------------------------------------------------------

def _tie_scene(axis):
    """a jittered 10^3 block around the slab, and in the middle of the slot order particles whose axis coordinate is
    exactly a plane or a threshold, the float below it, the float above it, and one NaN"""
    rng = np.random.default_rng(2024 + axis)
    g = np.arange(10, dtype=np.float32) * np.float32(1.1) - np.float32(4.95)
    block = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    block = (block + (rng.random(block.shape) * 0.6 - 0.3)).astype(np.float32)
    marks = []
    for t in (LO, HI, LO + WF, LO + W, HI - W, HI - WF):
        t = np.float32(t)
        marks += [t, np.nextafter(t, np.float32(-INF)), np.nextafter(t, np.float32(INF))]
    marks.append(np.float32(np.nan))
    hand = (rng.random((len(marks), 3)) * 6.0 - 3.0).astype(np.float32)
    hand[:, axis] = np.array(marks, np.float32)
    pos = np.concatenate([block[:500], hand, block[500:]])
    n = pos.shape[0]
    vel = (rng.random((n, 3)) - 0.5).astype(np.float32)
    ids = (rng.permutation(n) + 100).astype(np.int32)
    return pos, vel, ids, np.arange(500, 500 + len(marks))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_pack_thresholds_and_ties(axis):
    pos, vel, ids, hand = _tie_scene(axis)
    n = pos.shape[0]
    eng = _engine(_unit_params(n, n + 100), pos, vel, ids, slab=(axis, LO, HI))
    ref, state, _ = _pack_and_check(eng, axis, LO, HI, WF, W, what=f"axis {axis}")
    assert np.array_equal(_u32(state[0]), _u32(pos)) and np.array_equal(state[2], ids)  # slot order is upload order
    # where the hand-placed particles must be, spelled out (the reference is checked here as well).  Per threshold t:
    # t itself, the float below, the float above; then the NaN.
    where = []
    for i in hand:
        w = [f"{s}.{k}" for s in ("lo", "hi") for k in ("full", "xonly") if i in ref[s][k]]
        where.append(",".join(w))
    assert where == [
        "lo.full", "lo.full", "lo.full",          # the lower plane: ghosts and owned alike are within width_full
        "hi.full", "hi.full", "hi.full",          # the upper plane
        "lo.xonly", "lo.full", "lo.xonly",        # lo + width_full: p < t is full
        "", "lo.xonly", "",                       # lo + width: p < t is position-only
        "hi.xonly", "", "hi.xonly",               # hi - width: p >= t is position-only
        "hi.full", "hi.xonly", "hi.full",         # hi - width_full: p >= t is full
        "",                                       # NaN: no band
    ]
    st = eng.slab_status()
    assert st[0] == 0
    assert st[2:] == (max(ref["lo"]["counts"][0], ref["hi"]["counts"][0]), max(ref["lo"]["counts"][1], ref["hi"]["counts"][1]))
    eng.close()


@pytest.mark.parametrize("spare", [0, 777])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049, 5 * 2048 + 17])
def test_pack_ragged_sizes(n, spare):
    """live counts around the wave and the pack block (2048 slots), capacity equal to and above the live count.  The
    planes are such that the zero-filled slots behind the live ones WOULD be band members (0 < lo + width)."""
    lo, hi = -1.0, 7.0
    pos, vel, ids = _cloud(n, 7 * n + spare, -2.0, 8.0)
    if n == 1:
        pos[0, 2] = -0.5  # the only particle is a record
    eng = _engine(_unit_params(n, n + spare), pos, vel, ids, slab=(2, lo, hi))
    ref, _, _ = _pack_and_check(eng, 2, lo, hi, WF, W, what=f"n {n} capacity {n + spare}")
    total = sum(ref[s]["counts"][k] for s in ("lo", "hi") for k in (0, 1))
    assert total >= 1 and (n < 63 or total > n // 4)
    assert eng.n == n and eng.slab_status()[0] == 0
    eng.close()


def test_pack_empty_band():
    n = 3000
    pos, vel, ids = _cloud(n, 3, -1.9, 1.9)  # all of it between lo + width and hi - width
    eng = _engine(_unit_params(n), pos, vel, ids, slab=(1, LO, HI))
    ref, _, words = _pack_and_check(eng, 1, LO, HI, WF, W, caps=(40, 50), what="empty band")
    for side in ("lo", "hi"):
        assert ref[side]["counts"] == (0, 0)
        assert words[side][:2].tolist() == [0, 0]
        assert np.all(words[side][2:] == SLAB_SENTINEL)
    assert eng.slab_status() == (0, 0, 0, 0)
    eng.close()


@pytest.mark.parametrize("side", ["lo", "hi"])
def test_pack_one_sided(side):
    """dev_lo only / dev_hi only: the other buffer is untouched, the high-water marks are the asked side's.  The lower
    band of this scene holds about twice what the upper one holds, so neither case can pass on the other side's counts."""
    n = 4500
    pos, vel, ids = _cloud(n, 17)
    pos[: n // 3, 0] = np.abs(pos[: n // 3, 0]) * np.float32(-1.0)  # more particles below
    eng = _engine(_unit_params(n, n + 9), pos, vel, ids, slab=(0, LO, HI))
    want = (side == "lo", side == "hi")
    ref, _, _ = _pack_and_check(eng, 0, LO, HI, WF, W, want=want, what=f"{side} only")
    other = "hi" if side == "lo" else "lo"
    assert ref[side]["counts"] != ref[other]["counts"] and min(ref[side]["counts"]) > 100
    assert eng.slab_status(reset_high_water=True) == (0, 0) + ref[side]["counts"]
    # ... and both sides after the reset: the maximum of the two
    ref, _, _ = _pack_and_check(eng, 0, LO, HI, WF, W, what="both sides")
    assert eng.slab_status() == (0, 0, max(ref["lo"]["counts"][0], ref["hi"]["counts"][0]),
                                 max(ref["lo"]["counts"][1], ref["hi"]["counts"][1]))
    eng.close()


@pytest.mark.parametrize("lo,hi", [(-INF, HI), (LO, INF), (-INF, INF)])
def test_pack_domain_ends(lo, hi):
    n = 2500
    pos, vel, ids = _cloud(n, 23)
    eng = _engine(_unit_params(n), pos, vel, ids, slab=(2, lo, hi))
    ref, _, words = _pack_and_check(eng, 2, lo, hi, WF, W, what=f"[{lo}, {hi})")
    for side, plane in (("lo", lo), ("hi", hi)):
        if np.isinf(plane):
            assert ref[side]["counts"] == (0, 0) and words[side][:2].tolist() == [0, 0]
            assert np.all(words[side][2:] == SLAB_SENTINEL)
        else:
            assert min(ref[side]["counts"]) > 100
    assert eng.n_owned() == n if (np.isinf(lo) and np.isinf(hi)) else eng.n_owned() < n
    eng.close()


@pytest.mark.parametrize("lo,hi", [(-1.5, 1.5), (-0.5, 0.5)])
def test_pack_thin_slab(lo, hi):
    """hi - lo < 2 width: [hi - width, lo + width) belongs to both messages -- as position-only records for the
    3-wide slab, as full records for the 1-wide one (hi - lo < 2 width_full as well)"""
    n = 4100
    pos, vel, ids = _cloud(n, 31, -3.0, 3.0)
    eng = _engine(_unit_params(n), pos, vel, ids, slab=(1, lo, hi))
    ref, _, _ = _pack_and_check(eng, 1, lo, hi, WF, W, what=f"thin slab [{lo}, {hi})")
    kind = "xonly" if hi - lo > 2 * WF else "full"
    both = np.intersect1d(ref["lo"][kind], ref["hi"][kind])
    p = pos[:, 1]
    expect = np.nonzero((p >= np.float32(-0.5)) & (p < np.float32(0.5)))[0]
    assert both.size > 300 and np.array_equal(both, expect)
    eng.close()


def _scattered_lattice(n3, spacing, seed):
    rng = np.random.default_rng(seed)
    g = (np.arange(n3, dtype=np.float32) - np.float32(0.5 * (n3 - 1))) * np.float32(spacing)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    pos = (pos + (rng.random(pos.shape) - 0.5) * 0.3 * spacing).astype(np.float32)
    pos = pos[rng.permutation(pos.shape[0])]
    n = pos.shape[0]
    return pos, (rng.random((n, 3)) - 0.5).astype(np.float32), (rng.permutation(n) * 2 + 5).astype(np.int32)


@pytest.mark.parametrize("math_mode", [0, 1])
def test_pack_scattered_and_cell_order(math_mode):
    """slot order scattered against cell order: uploaded in a random permutation the band members sit in every pack
    block; after the neighbour build the bands are a few contiguous slot runs.  Both packs must match."""
    lo, hi = -2.5, 2.5
    pos, vel, ids = _scattered_lattice(16, 0.5, 41)  # 4096 particles in [-4, 4]^3, about 8 per cell
    n = pos.shape[0]
    eng = _engine(_unit_params(n, 3 * 2048 + 5, math_mode), pos, vel, ids, slab=(0, lo, hi))
    _, before, _ = _pack_and_check(eng, 0, lo, hi, WF, W, what="upload order")
    eng.nn()
    ref, after, _ = _pack_and_check(eng, 0, lo, hi, WF, W, what="cell order")
    assert eng.n == n and not np.array_equal(before[2], after[2])
    o0, o1 = np.argsort(before[2]), np.argsort(after[2])
    assert np.array_equal(before[2][o0], after[2][o1])
    assert np.array_equal(_u32(before[0][o0]), _u32(after[0][o1])) and np.array_equal(_u32(before[1][o0]), _u32(after[1][o1]))
    assert min(ref["lo"]["counts"] + ref["hi"]["counts"]) > 300
    eng.close()


def test_pack_large_shape():
    """capacity 257 x 2048: k_slab_offsets gives each of its threads two pack blocks, threads 129.. are idle, thread
    128 has one block, and the offsets of waves 1 and 2 start from the sums of the waves before them"""
    cap, n = 257 * 2048, 526000
    pos, vel, ids = _cloud(n, 53)
    eng = _engine(_unit_params(n, cap), pos, vel, ids, slab=(2, LO, HI))
    ref, _, _ = _pack_and_check(eng, 2, LO, HI, WF, W, what="526k slots")
    assert min(ref["lo"]["counts"] + ref["hi"]["counts"]) > 40000
    # the last pack block (slots 524288..) holds records of every category
    for s in ("lo", "hi"):
        assert ref[s]["full"][-1] >= 256 * 2048 and ref[s]["xonly"][-1] >= 256 * 2048
    eng.close()


_CAP_PAIRS = {"exact": lambda nf, nx: (nf, nx), "full-1": lambda nf, nx: (nf - 1, nx), "x-1": lambda nf, nx: (nf, nx - 1),
              "full=0": lambda nf, nx: (0, nx), "x=0": lambda nf, nx: (nf, 0), "3,2": lambda nf, nx: (3, 2)}


@pytest.mark.parametrize("side", ["lo", "hi"])
@pytest.mark.parametrize("pair", list(_CAP_PAIRS))
def test_pack_caps(pair, side):
    """one fixed state, capacities set from the counts (nf, nx) of one side; both messages are packed and each is
    clamped where ITS counts exceed the pair: header clamped, the first records in slot order kept, the sentinel intact
    everywhere else"""
    n = 2600
    pos, vel, ids = _cloud(n, 61)
    pos[: n // 4, 1] = np.abs(pos[: n // 4, 1])  # the two sides differ
    eng = _engine(_unit_params(n, n + 50), pos, vel, ids, slab=(1, LO, HI))
    counts = _counts((pos, vel, ids), 1, LO, HI, WF, W)
    caps = _CAP_PAIRS[pair](*counts[side])
    ref, _, words = _pack_and_check(eng, 1, LO, HI, WF, W, caps=caps, what=f"caps {caps}")
    hw_f, hw_x = max(counts["lo"][0], counts["hi"][0]), max(counts["lo"][1], counts["hi"][1])
    over = max([c for s in ("lo", "hi") for c, cap in zip(counts[s], caps) if c > cap], default=0)
    if pair != "exact":
        assert over > 0
    for s in ("lo", "hi"):
        assert words[s][:2].view(np.int32).tolist() == [min(counts[s][0], caps[0]), min(counts[s][1], caps[1])]
    assert eng.slab_status(reset_high_water=True) == (over, 0, hw_f, hw_x)
    assert eng.slab_status() == (over, 0, 0, 0)
    assert eng.slab_overflow() == over
    eng.close()


# ---- PCISPH: 13-float records ----------------------------------------------------------------------------------

def _pci_scene(n3=12):
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(n3, math_mode=1)
    p.pci_max_iters, p.eos_w, p.delta, p.pci_max_error = 4, p.eos_w / 4, 1.0e-7, 1.0
    vel = (0.5 * _vel_fn(np.arange(n3 ** 3), pos, 2)).astype(np.float32)
    return p, pos, vel


def _pci_sender():
    """12^3 dam-break after pcisph_begin and one step (the predictor state has left the particles), then a slab along z"""
    p, pos, vel = _pci_scene()
    n = pos.shape[0]
    lo, hi = 3.0 * p.h, 4.0 * p.h   # thin enough for both messages to hold full and position-only records
    eng = _engine(p, pos, vel, (np.random.default_rng(3).permutation(n) + 7).astype(np.int32))
    eng.pcisph_begin()
    eng.pcisph_step(1)
    eng.slab_config(2, lo, hi)
    pci = (eng.download("pci_positions", sorted_order=True), eng.download("pci_velocities", sorted_order=True))
    return eng, p, lo, hi, pci


def test_pack_pcisph_records():
    eng, p, lo, hi, pci = _pci_sender()
    assert eng.slab_record_floats() == REC_PCI
    state = _state(eng)
    assert not np.array_equal(_u32(pci[0]), _u32(state[0]))  # (words 7..12 are not a copy of words 0..5)
    counts = _counts(state, 2, lo, hi, p.h, 2 * p.h)
    caps = (max(counts["lo"][0], counts["hi"][0]) + 2, max(counts["lo"][1], counts["hi"][1]) + 2)
    assert eng.slab_message_floats(*caps) == (caps[0] + 1) * REC_PCI + caps[1] * REC_X
    ref, _, words = _pack_and_check(eng, 2, lo, hi, p.h, 2 * p.h, caps=caps, rec=REC_PCI, pci=pci, what="pcisph")
    for s in ("lo", "hi"):
        nf, nx = ref[s]["counts"]
        assert nf > 100 and nx > 100
        full = words[s][REC_PCI:(nf + 1) * REC_PCI].reshape(nf, REC_PCI)
        assert np.array_equal(full[:, 7:10], _u32(pci[0][ref[s]["full"]]))
        assert np.array_equal(full[:, 10:13], _u32(pci[1][ref[s]["full"]]))
        x = words[s][(caps[0] + 1) * REC_PCI:][:nx * REC_X].reshape(nx, REC_X)
        assert np.array_equal(x[:, 0:3], _u32(state[0][ref[s]["xonly"]])) and np.array_equal(x[:, 3], _u32(state[2][ref[s]["xonly"]]))
    eng.close()


# ---- append: dsl_slab_append / dsl_slab_append2 ------------------------------------------------------------------

def _decode(words, cap_full, cap_x, rec=REC):
    """the records of a message as the receiver has to store them: (pos, vel, ids, pci_pos, pci_vel), full records
    first, then the position-only ones with zero velocity (and, rec = 13, their own position as the predicted one).
    Header counts outside [0, cap] count as 0 / cap."""
    nf, nx = (int(v) for v in words[:2].view(np.int32))
    nf, nx = min(max(nf, 0), cap_full), min(max(nx, 0), cap_x)
    f = words[rec:(nf + 1) * rec].reshape(nf, rec)
    x = words[(cap_full + 1) * rec:][:nx * REC_X].reshape(nx, REC_X)
    zero = np.zeros((nx, 3), np.uint32)
    pos = np.concatenate([f[:, 0:3], x[:, 0:3]])
    vel = np.concatenate([f[:, 3:6], zero])
    ids = np.concatenate([f[:, 6], x[:, 3]]).view(np.int32)
    if rec == REC_PCI:
        return pos, vel, ids, np.concatenate([f[:, 7:10], x[:, 0:3]]), np.concatenate([f[:, 10:13], zero])
    return pos, vel, ids, None, None


def _append_and_check(recv, expect, msgs, cap_full, cap_x, plane, rec=REC, how="append2", fits=True):
    """appends `msgs` = (a, b) (numpy words or None) to `recv`, whose slot-order state is `expect` (a dict of uint32 /
    int32 arrays), and compares the whole new state; returns it"""
    bufs = [None if m is None else _Buf(m.size) for m in msgs]
    for b, m in zip(bufs, msgs):
        if b is not None:
            b.set(m)
    ptrs = [0 if b is None else b.ptr for b in bufs]
    if how == "append":
        assert ptrs[1] == 0
        recv.slab_append(ptrs[0], cap_full, cap_x)
    else:
        recv.slab_append2(ptrs[0], ptrs[1], cap_full, cap_x)
    recv.sync()
    new = {k: v for k, v in expect.items()}
    if fits:
        for m in msgs:
            if m is None:
                continue
            pos, vel, ids, pp, pv = _decode(m, cap_full, cap_x, rec)
            new = {"pos": np.concatenate([new["pos"], pos]), "vel": np.concatenate([new["vel"], vel]),
                   "ids": np.concatenate([new["ids"], ids]),
                   "pci_pos": None if pp is None else np.concatenate([new["pci_pos"], pp]),
                   "pci_vel": None if pv is None else np.concatenate([new["pci_vel"], pv])}
    _assert_state(recv, new, plane)
    for b, m in zip(bufs, msgs):  # an append reads its messages, nothing else
        if b is not None:
            assert np.array_equal(b.words(), m)
    return new


def _expect_of(eng, rec=REC):
    pos, vel, ids = _state(eng)
    e = {"pos": _u32(pos), "vel": _u32(vel), "ids": ids, "pci_pos": None, "pci_vel": None}
    if rec == REC_PCI:
        e["pci_pos"] = _u32(eng.download("pci_positions", sorted_order=True))
        e["pci_vel"] = _u32(eng.download("pci_velocities", sorted_order=True))
    return e


def _numpy_owned(pos_words, plane):
    axis, lo, hi = plane
    p = np.ascontiguousarray(pos_words).view(np.float32)
    with np.errstate(invalid="ignore"):
        return int(np.count_nonzero(np.isfinite(p).all(axis=1) & (p[:, axis] >= np.float32(lo)) & (p[:, axis] < np.float32(hi))))


def _assert_state(eng, expect, plane):
    n = expect["ids"].shape[0]
    assert eng.n == n
    got = _expect_of(eng, REC_PCI if expect["pci_pos"] is not None else REC)
    for k, v in expect.items():
        if v is not None:
            assert np.array_equal(got[k], v), f"{k} differ after the append"
    assert eng.n_owned() == _numpy_owned(expect["pos"], plane)


def _sender_messages(caps_of=None):
    """a packed pair of messages of the unit scene along x (checked against the reference on the way)"""
    n = 3000
    pos, vel, ids = _cloud(n, 71)
    eng = _engine(_unit_params(n), pos, vel, ids, slab=(0, LO, HI))
    counts = _counts((pos, vel, ids), 0, LO, HI, WF, W)
    caps = caps_of(counts) if caps_of else (max(counts["lo"][0], counts["hi"][0]) + 4, max(counts["lo"][1], counts["hi"][1]) + 6)
    ref, _, _ = _pack_and_check(eng, 0, LO, HI, WF, W, caps=caps, what="sender")
    eng.close()
    return ref["lo"]["words"], ref["hi"]["words"], caps, counts


def _receiver(m0, capacity, plane, seed=83):
    pos, vel, ids = _cloud(m0, seed)
    ids = ids + 100000  # (no id of the sender's)
    return _engine(_unit_params(m0, capacity), pos, vel, ids, slab=plane)


def test_append_one_message_then_the_other_then_both():
    """a alone (dsl_slab_append), b alone with a = NULL (dsl_slab_append2), then (a, b) in one call, on one receiver: old
    slots unchanged to the bit, a's full records, a's position-only records with zero velocity, then b's; ids intact;
    the owned count is the count of positions inside the receiver's [lo, hi) -- the receiver's planes cut through both
    messages' full records, so some of those are migrants (owned) and the rest ghosts"""
    a, b, caps, counts = _sender_messages()
    plane = (0, -3.5, 3.25)
    per = {s: counts[s][0] + counts[s][1] for s in ("lo", "hi")}
    m0 = 700
    recv = _receiver(m0, m0 + 2 * (per["lo"] + per["hi"]) + 10, plane)
    e = _expect_of(recv)
    own0 = recv.n_owned()
    assert own0 == _numpy_owned(e["pos"], plane) and 0 < own0 < m0
    e = _append_and_check(recv, e, (a, None), *caps, plane, how="append")
    assert e["ids"].shape[0] == m0 + per["lo"]
    own1 = recv.n_owned()
    assert own0 < own1 < own0 + per["lo"]  # migrants and ghosts
    e = _append_and_check(recv, e, (None, b), *caps, plane)
    assert e["ids"].shape[0] == m0 + per["lo"] + per["hi"]
    e = _append_and_check(recv, e, (a, b), *caps, plane)
    assert e["ids"].shape[0] == m0 + 2 * (per["lo"] + per["hi"])
    assert recv.slab_status()[0] == 0
    recv.close()


def test_append_exact_fit_and_one_record_too_many():
    a, b, caps, counts = _sender_messages()
    plane = (0, -3.5, 3.25)
    total = sum(counts[s][k] for s in ("lo", "hi") for k in (0, 1))
    m0 = 300
    # n + records == capacity: everything is appended
    recv = _receiver(m0, m0 + total, plane)
    e = _append_and_check(recv, _expect_of(recv), (a, b), *caps, plane)
    assert recv.n == recv.capacity == m0 + total and recv.slab_status()[0] == 0
    recv.close()
    # one slot short: nothing is appended, the state and the count stay, the status word holds the total asked for
    recv = _receiver(m0, m0 + total - 1, plane)
    _append_and_check(recv, _expect_of(recv), (a, b), *caps, plane, fits=False)
    assert recv.n == m0
    assert recv.slab_status(reset_high_water=True)[0] == m0 + total
    assert recv.slab_status()[0] == m0 + total
    # ... and the single-message entry point likewise
    recv.close()
    na = counts["lo"][0] + counts["lo"][1]
    recv = _receiver(m0, m0 + na - 1, plane)
    _append_and_check(recv, _expect_of(recv), (a, None), *caps, plane, how="append", fits=False)
    assert recv.n == m0 and recv.slab_status()[0] == m0 + na
    recv.close()


@pytest.mark.parametrize("which", ["full<0", "x<0"])
def test_append_clamps_out_of_range_header_counts(which):
    """hand-written headers: a count of -5 is 0 records, a count of cap + 7 is cap records (slab_counts).  The
    capacities are the exact counts, so all cap records exist; the receiver has room for exactly the clamped total."""
    a, _, caps, counts = _sender_messages(caps_of=lambda c: c["lo"])
    assert caps == counts["lo"] and min(caps) > 100
    bad = a.copy()
    hdr = np.array([-5, caps[1] + 7] if which == "full<0" else [caps[0] + 7, -5], np.int32)
    bad[:2] = hdr.view(np.uint32)
    clamped = caps[1] if which == "full<0" else caps[0]
    plane = (0, -3.5, 3.25)
    m0 = 200
    recv = _receiver(m0, m0 + clamped, plane)
    e = _append_and_check(recv, _expect_of(recv), (bad, None), *caps, plane)
    assert recv.n == m0 + clamped and recv.slab_status()[0] == 0
    # the records that arrived are the ones of that category, all of them
    want = _decode(a, *caps)
    rows = slice(caps[0], None) if which == "full<0" else slice(0, caps[0])
    assert np.array_equal(e["ids"][m0:], want[2][rows])
    recv.close()


def test_append_pcisph_records():
    """13-float records: a full record keeps its predictor state, a position-only record gets its own position and
    zero velocity there"""
    eng, p, lo, hi, pci = _pci_sender()
    state = _state(eng)
    counts = _counts(state, 2, lo, hi, p.h, 2 * p.h)
    caps = (max(counts["lo"][0], counts["hi"][0]) + 2, max(counts["lo"][1], counts["hi"][1]) + 2)
    ref, _, _ = _pack_and_check(eng, 2, lo, hi, p.h, 2 * p.h, caps=caps, rec=REC_PCI, pci=pci, what="pcisph sender")
    eng.close()
    a, b = ref["lo"]["words"], ref["hi"]["words"]
    total = sum(counts[s][k] for s in ("lo", "hi") for k in (0, 1))
    # the receiver: the first 500 particles of the same scene, predictor state = their own state
    q, pos, vel = _pci_scene()
    m0 = 500
    q.n_particles, q.capacity = m0, m0 + total
    plane = (2, 3.5 * p.h, 6.0 * p.h)  # cuts through the upper message's full records
    recv = _engine(q, pos[:m0], vel[:m0], np.arange(m0, dtype=np.int32) + 50000)
    recv.pcisph_begin()
    recv.slab_config(*plane)
    assert recv.slab_record_floats() == REC_PCI
    e = _expect_of(recv, REC_PCI)
    e = _append_and_check(recv, e, (a, b), *caps, plane, rec=REC_PCI)
    assert recv.n == recv.capacity
    nf, nx = counts["lo"]
    blk = slice(m0, m0 + nf + nx)
    assert np.array_equal(e["pci_pos"][blk][nf:], e["pos"][blk][nf:]) and not e["pci_vel"][blk][nf:].any()
    assert not np.array_equal(e["pci_pos"][blk][:nf], e["pos"][blk][:nf])
    recv.close()


# ---- the life cycle of a ghost -----------------------------------------------------------------------------------

@pytest.mark.parametrize("math_mode", [0, 1])
def test_ghost_life_cycle(math_mode):
    """a 16^3 dam-break held by one engine, [lo, hi) on cell planes inside the block: the step turns every slot outside
    [lo, hi) into NaN, a pack made then holds none of them, the next neighbour build drops them"""
    from dieselfluid_amd import scenes
    n3 = 16
    p, pos = scenes.dambreak_scene(n3, math_mode=math_mode)
    n = n3 ** 3
    vel = _vel_fn(np.arange(n), pos, 2).astype(np.float32)
    ids = (np.random.default_rng(9).permutation(n) + 1).astype(np.int32)
    plane = (2, 0.25, 0.75)  # h = 1/8, grid origin -h: cell planes
    wf, w = p.h, 2 * p.h
    eng = _engine(p, pos, vel, ids, slab=plane)
    assert eng.n_owned() == _numpy_owned(_u32(pos), plane)
    eng.nn()
    eng.density_all()
    before = _state(eng)
    assert eng.n == n and eng.n_owned() == _numpy_owned(_u32(before[0]), plane)
    inside = (before[0][:, 2] >= np.float32(plane[1])) & (before[0][:, 2] < np.float32(plane[2]))
    assert 0 < inside.sum() < n
    eng.force_pass()
    after = _state(eng)
    assert eng.n == n and np.array_equal(after[2], before[2])
    assert np.all(np.isnan(after[0][~inside])) and np.all(np.isfinite(after[0][inside]))
    assert eng.n_owned() == _numpy_owned(_u32(after[0]), plane)
    ref, _, _ = _pack_and_check(eng, 2, plane[1], plane[2], wf, w, what="after the step")
    packed = np.concatenate([ref[s][k] for s in ("lo", "hi") for k in ("full", "xonly")])
    assert packed.size > 1000 and np.all(inside[packed])
    eng.nn()
    last = _state(eng)
    assert eng.n == int(inside.sum()) and np.array_equal(np.sort(last[2]), np.sort(after[2][inside]))
    assert np.all(np.isfinite(last[0])) and eng.n_owned() == _numpy_owned(_u32(last[0]), plane)
    eng.close()


# ---- split step: dsl_slab_pack_band ------------------------------------------------------------------------------

def _split_scene():
    from dieselfluid_amd import scenes
    n3 = 32
    p, pos = scenes.dambreak_scene(n3, math_mode=1)
    vel = _vel_fn(np.arange(n3 ** 3), pos, 2).astype(np.float32)
    # h = 1/16, grid origin -h: planes on cell planes, 12 cell layers apart; width + margin = 4 layers per side
    return p, pos, vel, (2, 0.125, 0.875)


def _record_ids(ref, state):
    return {(s, k): np.sort(state[2][ref[s][k]]) for s in ("lo", "hi") for k in ("full", "xonly")}


def test_pack_band_in_the_split_step():
    """three split steps (both ping-pong halves serve as the output, and from the second step on the output half
    holds the values of two steps earlier in the slots the band pass does not write): the band pack, made between the two
    force launches, must be the reference of the state the whole step leaves.  Then the same steps unsplit on a fresh
    engine: the same particles in every message of every step."""
    p, pos, vel, plane = _split_scene()
    wf, w = p.h, 2 * p.h
    eng = _engine(p, pos, vel, slab=plane)
    eng.slab_split(w, 2 * p.h)
    n = pos.shape[0]
    split_ids = []
    for step in range(3):
        eng.nn()
        eng.density_all()
        eng.force_pass_split(SPLIT_BAND)
        bufs = [_Buf((n + 1) * REC + n * REC_X + GUARD) for _ in range(2)]
        eng.slab_pack_band(wf, bufs[0].ptr, bufs[1].ptr, n, n, 0)
        eng.force_pass_split(SPLIT_INNER)
        eng.sync()
        state = _state(eng)
        ref = slab_message_reference(*state, 2, plane[1], plane[2], wf, w, n, n)
        for s, b in zip(("lo", "hi"), bufs):
            _assert_message(b.words(), ref[s], f"split step {step}, {s} message")
            assert min(ref[s]["counts"]) > 1000
        assert eng.slab_status()[:2] == (0, 0)
        # interior layers exist: particles that are in no message
        assert sum(ref[s]["counts"][k] for s in ("lo", "hi") for k in (0, 1)) < np.isfinite(state[0][:, 2]).sum() - 4000
        split_ids.append(_record_ids(ref, state))
    eng.close()
    eng = _engine(p, pos, vel, slab=plane)
    for step in range(3):
        eng.nn()
        eng.density_all()
        eng.force_pass()
        ref, state, _ = _pack_and_check(eng, 2, plane[1], plane[2], wf, w, what=f"unsplit step {step}")
        mine = _record_ids(ref, state)
        for key in mine:
            assert np.array_equal(mine[key], split_ids[step][key]), f"step {step}: {key} holds other particles than in the split step"
    # (the bands change from step to step: what the old-coordinate filter lets through matters)
    assert any(not np.array_equal(split_ids[0][k], split_ids[2][k]) for k in split_ids[0])
    eng.close()
