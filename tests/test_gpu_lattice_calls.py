"""GPU: what the lattice entry points share on the host side -- dsl_field_volume, dsl_surface_extract, dsl_field_surface,
dsl_surface_extract_indexed, dsl_field_surface_indexed, dsl_mesh_distance_volume and dsl_collider_set_volume.  Three seams
that the units' own suites (which compare the kernels' bits) leave open: the full text of every refusal of a bad lattice, the
bytes that every library-owned array adds to DSL_OPT_DEVICE_BYTES when a call grows it, and which per-phase times read zero.
Everything runs on an 8-particle handle and lattices of 3 x 3 x 3 and 9 x 5 x 4 voxels."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INVALID = -1  # DSL_ERR_INVALID
SMALL, LARGER = (3, 3, 3), (9, 5, 4)
ENTRIES = ("dsl_field_volume", "dsl_surface_extract", "dsl_field_surface", "dsl_surface_extract_indexed",
           "dsl_field_surface_indexed", "dsl_mesh_distance_volume", "dsl_collider_set_volume")
CAP = 2048  # triangles and vertices: 8 x 4 x 3 cubes hold at most 1152 triangles
# one triangle across the lattices' box [0, 1]^3
TRIANGLE = np.array([[0.1, 0.2, 0.3], [0.9, 0.3, 0.4], [0.4, 0.8, 0.7]], dtype=np.float32)
MS_OPTIONS = ("surface_count_ms", "surface_scan_ms", "surface_emit_ms", "surface_mesh_vcount_ms", "surface_mesh_vscan_ms",
              "surface_mesh_vemit_ms", "surface_mesh_iemit_ms", "sdf_distance_ms", "sdf_sign_ms")


def _lattice(dims):
    """the lattice over [0, 1]^3 with these dims"""
    return (0.0, 0.0, 0.0), tuple(1.0 / (n - 1) for n in dims), dims


class Rig:
    """an 8-particle handle with its densities, and one caller per entry point that takes the three lattice pointers as
    tuples or None (NULL); every other argument is valid"""

    def __init__(self):
        import torch
        from dieselfluid_amd import SPHEngine, scenes
        p, pos = scenes.dambreak_scene(2)  # 8 particles at 0.25 and 0.75 per axis, h = 1
        self.eng = SPHEngine(p, device=0)
        self.eng.upload("positions", pos)
        self.eng.density_all()
        self.L, self.h = self.eng._L, self.eng._h
        # a device volume that crosses iso = 0 in both lattices (x fastest): i + j + k - 2.5
        self.dvol = {}
        for dims in (SMALL, LARGER):
            k, j, i = np.meshgrid(*(np.arange(n, dtype=np.float32) for n in dims[::-1]), indexing="ij")
            self.dvol[dims] = torch.from_numpy((i + j + k - np.float32(2.5)).reshape(-1)).cuda()
        self.scratch = torch.zeros(256, dtype=torch.float32, device="cuda")
        self.host_f = np.zeros(9 * CAP, dtype=np.float32)
        self.host_n = np.zeros(3 * CAP, dtype=np.float32)
        self.host_i = np.zeros(3 * CAP, dtype=np.int32)
        self.counts = (C.c_int64 * 2)(0, 0)
        # (into a buffer of the test's own: the neighbour grid is built here, and no array of the library's grows yet)
        self.eng.field_volume(*_lattice(SMALL), dev_out=self.scratch.data_ptr())
        self.eng.sync()
        rho = self.scratch[:27].cpu().numpy()
        assert rho.min() < rho.max()
        self.iso = 0.5 * float(rho.min() + rho.max())  # the densities' surface: between the centre and the corners

    def close(self):
        self.eng.close()

    def bytes(self):
        return self.eng.get_option("device_bytes")

    def call(self, name, o, s, d, caps=True, unsigned=False):
        """(return code, dsl_last_error) of one call of the entry point `name` on the lattice (o, s, d)"""
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        po = (C.c_float * 3)(*o) if o is not None else None
        ps = (C.c_float * 3)(*s) if s is not None else None
        pd = (C.c_int32 * 3)(*d) if d is not None else None
        L, h = self.L, self.h
        dvol = self.dvol.get(tuple(d) if d is not None else SMALL, self.dvol[SMALL])
        hf, hn, hi = self.host_f.ctypes.data_as(fp), self.host_n.ctypes.data_as(fp), self.host_i.ctypes.data_as(ip)
        cap = CAP if caps else 0
        if name == "dsl_field_volume":
            rc = L.dsl_field_volume(h, 3, po, ps, pd, None, hf)
        elif name == "dsl_surface_extract":
            rc = L.dsl_surface_extract(h, C.c_void_p(dvol.data_ptr()), po, ps, pd, C.c_float(0.0),
                                       C.c_void_p(self.scratch.data_ptr()) if caps else None, None, 16 if caps else 0, None, self.counts)
        elif name == "dsl_field_surface":
            rc = L.dsl_field_surface(h, 3, po, ps, pd, C.c_float(self.iso), hf, hn, cap, self.counts)
        elif name == "dsl_surface_extract_indexed":
            rc = L.dsl_surface_extract_indexed(h, C.c_void_p(dvol.data_ptr()), po, ps, pd, C.c_float(0.0),
                                               C.c_void_p(self.scratch.data_ptr()) if caps else None, None, 16 if caps else 0,
                                               C.c_void_p(self.scratch[128:].data_ptr()) if caps else None, 16 if caps else 0, None,
                                               self.counts)
        elif name == "dsl_field_surface_indexed":
            rc = L.dsl_field_surface_indexed(h, 3, po, ps, pd, C.c_float(self.iso), hf, hn, cap, hi, cap, self.counts)
        elif name == "dsl_mesh_distance_volume":
            rc = L.dsl_mesh_distance_volume(h, TRIANGLE.ctypes.data_as(fp), 1, po, ps, pd, C.c_float(float("inf")),
                                            1 if unsigned else 0, None, hf)
        else:
            rc = L.dsl_collider_set_volume(h, None, hf, po, ps, pd, C.c_float(0.1), C.c_float(0.0), 0)
        return rc, L.dsl_last_error(h).decode()


@pytest.fixture
def rig():
    r = Rig()
    yield r
    r.close()


# ---- 1. refusals: the full text, the first fault, and nothing moved -----------------------------------------------------
def _refusal_text(name, fault):
    """what the library says: dsl_field_surface and dsl_field_surface_indexed leave the lattice to dsl_field_volume's check"""
    who = "dsl_field_volume" if name in ("dsl_field_surface", "dsl_field_surface_indexed") else name
    collider = name == "dsl_collider_set_volume"
    if fault == "null":
        return who + (": origin and step must not be NULL" if collider else ": origin, step and dims must not be NULL")
    if fault == "many" and "indexed" in name:
        return name + ": dims holds more than 2^28 voxels"
    return who + {"dims": ": every entry of dims must be >= " + ("2" if collider else "1"),
                  "many": ": dims holds more than 2^30 voxels",
                  "step": ": every entry of step must be finite and > 0",
                  "origin": ": every entry of origin must be finite"}[fault]


def _bad_lattices(name):
    """(origin, step, dims, fault): every way one lattice can be wrong, and one that is wrong twice"""
    o, s, d = _lattice(SMALL)
    inf, nan = float("inf"), float("nan")
    low = 1 if name == "dsl_collider_set_volume" else 0
    cases = [(None, s, d, "null"), (o, None, d, "null"), (o, s, None, "null"),
             (o, s, (3, low, 3), "dims"), (o, s, (low, 3, 3), "dims"), (o, s, (3, 3, low), "dims"),
             (o, s, (1024, 1024, 1025), "many"),
             (o, (0.0, 0.5, 0.5), d, "step"), (o, (0.5, -0.5, 0.5), d, "step"), (o, (0.5, 0.5, nan), d, "step"),
             (o, (inf, 0.5, 0.5), d, "step"),
             ((nan, 0.0, 0.0), s, d, "origin"), ((0.0, inf, 0.0), s, d, "origin"), ((0.0, 0.0, -inf), s, d, "origin"),
             # two faults: the axes are checked in turn, so the step of axis 0 is met before the dims of axis 1
             (o, (nan, 0.5, 0.5), (3, 0, 3), "step")]
    return cases


@pytest.mark.parametrize("name", ENTRIES)
def test_a_bad_lattice_is_refused_with_the_full_text_and_the_next_call_is_unaffected(rig, name):
    o, s, d = _lattice(SMALL)
    rc, text = rig.call(name, o, s, d)
    assert rc == 0, text
    before = rig.bytes()
    for bo, bs, bd, fault in _bad_lattices(name):
        rc, text = rig.call(name, bo, bs, bd)
        if name == "dsl_collider_set_volume" and bd is None:  # not a refusal there: dims = NULL removes the collider
            assert rc == 0 and rig.eng.get_option("collider_volume") == 0
        else:
            assert rc == INVALID and text == _refusal_text(name, fault), (bo, bs, bd, rc, text)
        rc, text = rig.call(name, o, s, d)
        assert rc == 0, (bo, bs, bd, text)
        assert rig.bytes() == before, (bo, bs, bd)
    if name == "dsl_collider_set_volume":
        assert rig.eng.get_option("collider_volume") == 27


# ---- 2. accounting: every array's share of DSL_OPT_DEVICE_BYTES ----------------------------------------------------------
def _scan_len(n):
    """the levels of the 64-bit scan over n values, one behind the other: 256 values per workgroup and level"""
    total = level = n
    while level > 256:
        level = -(-level // 256)
        total += level
    return total


def _bricks(dims, cubes=False):
    """bricks of 8 x 8 x 4 voxels (or cubes) that cover the lattice"""
    nx, ny, nz = (n - 1 if cubes else n for n in dims)
    return -(-nx // 8) * -(-ny // 8) * -(-nz // 4)


class Model:
    """what the arrays must hold: one that is large enough stays, one that is not is replaced by exactly what is asked for"""

    def __init__(self):
        self.have = {}

    def grow(self, name, count, item):
        """bytes added by reserving `count` items of `item` bytes"""
        old = self.have.get(name, 0)
        if count <= old:
            return 0
        self.have[name] = count
        return (count - old) * item

    def once(self, name, count, item):
        """a counter block: allocated at first use with the library's 64 bytes of padding, never grown"""
        if name in self.have:
            return 0
        self.have[name] = count
        return count * item + 64


def _expected(model, rig, name, dims):
    """the bytes the call just made must have added, from the counts it returned"""
    nvox = dims[0] * dims[1] * dims[2]
    g, once = model.grow, model.once
    n = 0
    if name in ("dsl_field_volume", "dsl_field_surface", "dsl_field_surface_indexed"):
        n += g("vol_stage", nvox, 4)
    if name in ("dsl_surface_extract", "dsl_field_surface", "dsl_surface_extract_indexed", "dsl_field_surface_indexed"):
        n += once("surf_ctr", 2, 8) + g("surf_scan", _scan_len(_bricks(dims, cubes=True)), 8)
    if name == "dsl_field_surface":
        T = rig.counts[0]
        assert 0 < T <= CAP
        n += g("surf_stage", 12 * T, 4)
    if name in ("dsl_surface_extract_indexed", "dsl_field_surface_indexed"):
        n += once("mesh_ctr", 2, 8) + g("mesh_scan", _scan_len(_bricks(dims)), 8) + g("mesh_words", nvox, 4)
    if name == "dsl_field_surface_indexed":
        V, T = rig.counts[0], rig.counts[1]
        assert 0 < V <= CAP and 0 < T <= CAP
        n += g("mesh_stage", 6 * V + 3 * T, 4)
    if name == "dsl_mesh_distance_volume":  # one triangle; band = +inf: every brick lists it
        nb = _bricks(dims)
        n += g("sdf_stage", nvox, 4) + g("sdf_verts", 9, 4) + g("sdf_rec", 4, 16) + g("sdf_box", 6, 4)
        n += g("sdf_scan", _scan_len(nb), 8) + once("sdf_ctr", 4, 8) + g("sdf_list", nb, 4) + g("sdf_marks", nvox, 4)
    if name == "dsl_collider_set_volume":
        n += g("colv_vol", nvox, 4) + once("col_hits", 1, 4)
    return n


def test_every_array_adds_its_bytes_once_and_a_larger_lattice_replaces_them(rig):
    model = Model()
    for step_no, dims in enumerate((SMALL, SMALL, LARGER, SMALL)):
        for name in ENTRIES:
            before = rig.bytes()
            rc, text = rig.call(name, *_lattice(dims))
            assert rc == 0, (name, dims, text)
            want = _expected(model, rig, name, dims)
            grew = rig.bytes() - before
            assert grew == want, (name, dims, step_no, grew, want)
            if step_no in (1, 3):  # the same call again, and a smaller lattice behind a larger one: nothing moves
                assert grew == 0, (name, dims, grew)
        # the volume collider in rigid motion: six partial sums per workgroup of 256 slots, and the six accumulator words
        before = rig.bytes()
        rig.eng.set_collider_volume_motion(trans=(0.0, 0.0, 0.0))
        assert rig.bytes() - before == model.grow("colv_partial", 6, 4) + model.once("colv_acc", 6, 4)
    assert model.have["vol_stage"] == 180 and model.have["mesh_scan"] == 2 and model.have["sdf_marks"] == 180


# ---- 3. the per-phase times: zero unless the phase ran with timing on ------------------------------------------------------
def _ms(rig):
    return {k: rig.eng.get_option(k) for k in MS_OPTIONS}


def _run_all(rig, caps, unsigned):
    o, s, d = _lattice(LARGER)
    for name in ("dsl_surface_extract", "dsl_surface_extract_indexed", "dsl_mesh_distance_volume"):
        rc, text = rig.call(name, o, s, d, caps=caps, unsigned=unsigned)
        assert rc == 0, text


def test_phase_times_are_zero_without_timing_and_for_the_phases_that_did_not_run(rig):
    _run_all(rig, caps=True, unsigned=False)
    assert all(v == 0.0 for v in _ms(rig).values()), _ms(rig)
    rig.eng.timing_enable(True)
    # every phase runs
    o, s, d = _lattice(LARGER)
    assert rig.call("dsl_surface_extract", o, s, d)[0] == 0
    soup = _ms(rig)
    assert soup["surface_count_ms"] > 0.0 and soup["surface_scan_ms"] > 0.0 and soup["surface_emit_ms"] > 0.0, soup
    assert all(soup[k] == 0.0 for k in MS_OPTIONS if not k.startswith("surface_") or "mesh" in k), soup
    _run_all(rig, caps=True, unsigned=False)
    every = _ms(rig)
    # (the indexed call runs the triangle count and its scan, and no triangle emit)
    assert all(every[k] > 0.0 for k in MS_OPTIONS if k != "surface_emit_ms") and every["surface_emit_ms"] == 0.0, every
    # counting calls and an unsigned volume: the emit phases and the sign phase did not run
    assert rig.call("dsl_surface_extract", o, s, d, caps=False)[0] == 0
    assert rig.eng.get_option("surface_emit_ms") == 0.0 and rig.eng.get_option("surface_count_ms") > 0.0
    _run_all(rig, caps=False, unsigned=True)
    some = _ms(rig)
    idle = ("surface_emit_ms", "surface_mesh_vemit_ms", "surface_mesh_iemit_ms", "sdf_sign_ms")
    assert all(some[k] == 0.0 for k in idle) and all(some[k] > 0.0 for k in MS_OPTIONS if k not in idle), some
    # timing off again: the next calls leave nothing to read
    rig.eng.timing_enable(False)
    _run_all(rig, caps=True, unsigned=False)
    assert all(v == 0.0 for v in _ms(rig).values()), _ms(rig)
