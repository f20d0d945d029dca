"""Sources and sinks without a GPU: the rule as tests/sources_ref.py states it (the ellipse mask against a float64 geometric
test and its order, the schedule by hand, the removal's renumbering as a property, NaN under both sink kinds, "never empty"),
and the names and arities of the new calls across the header, the ctypes table, the C++ mirror and the Go stub."""
import ctypes as C
import os
import re

import numpy as np

import sources_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_ellipse_mask_is_the_inscribed_ellipse_in_layer_order():
    """Every nu, nv <= 12: a point is kept when its centre lies in the closed ellipse with the rectangle's half axes nu / 2 and
    nv / 2 around the lattice's centre -- ((a - ca) / (nu / 2))^2 + ((b - cb) / (nv / 2))^2 <= 1 in float64.  Every quantity of
    the integer test is below 2^53, and points on the ellipse itself (the equality) are compared in exact rationals, so the
    float64 test may be asked for the same answer everywhere else: its margin is checked to be far from rounding."""
    from fractions import Fraction
    for nu in range(1, 13):
        for nv in range(1, 13):
            pts = sr.layer_points(nu, nv, 1)
            kept = {(int(a), int(b)) for a, b in pts}
            assert len(kept) == pts.shape[0] > 0
            for b in range(nv):
                for a in range(nu):
                    q = ((a - (nu - 1) / 2.0) / (nu / 2.0)) ** 2 + ((b - (nv - 1) / 2.0) / (nv / 2.0)) ** 2
                    exact = Fraction(2 * a - (nu - 1), nu) ** 2 + Fraction(2 * b - (nv - 1), nv) ** 2
                    if exact == 1:
                        want = True
                    else:
                        assert abs(q - 1.0) > 1e-9
                        want = q <= 1.0
                    assert ((a, b) in kept) == want, (nu, nv, a, b)
            # the centre is kept, so no mask is empty; b ascending, inside it a ascending
            assert ((nu - 1) // 2, (nv - 1) // 2) in kept
            key = pts[:, 1] * nu + pts[:, 0]
            assert np.all(np.diff(key) > 0)
            # the rectangle keeps every point, in the same order
            rect = sr.layer_points(nu, nv, 0)
            assert rect.shape[0] == nu * nv and np.array_equal(rect[:, 1] * nu + rect[:, 0], np.arange(nu * nv))


def test_a_layers_coordinates_round_every_product_and_sum_once():
    o, u, v = (0.1, 0.7, -0.3), (0.013, 0.002, 0.0), (0.001, 0.0, 0.017)
    got = sr.layer_positions(o, u, v, 5, 4, 0)
    assert got.dtype == np.float32 and got.shape == (20, 3)
    f = np.float32
    for k, (a, b) in enumerate(sr.layer_points(5, 4, 0)):
        for c in range(3):
            want = f(f(f(o[c]) + f(f(a) * f(u[c]))) + f(f(b) * f(v[c])))
            assert got[k, c].view(np.uint32) == want.view(np.uint32)
    # not the fused or float64 value everywhere: the rule is observable
    wide = (np.float64(f(o[0])) + 4 * np.float64(f(u[0])) + 3 * np.float64(f(v[0])))
    assert got[19, 0] == f(f(f(o[0]) + f(f(4) * f(u[0]))) + f(f(3) * f(v[0]))) and abs(float(got[19, 0]) - wide) < 1e-6


def test_the_schedule_by_hand():
    """period 3, first_step 2, max_layers 2 -- and a layer that does not fit is skipped, counted, and is no layer"""
    def em(**kw):
        return sr.Emitter((0, 0, 0), (1, 0, 0), (0, 0, 1), 5, 4, (0, -1, 0), **kw)
    s = sr.Schedule(100, 1000, [em(period=3, first_step=2, max_layers=2)])
    fired = [t for t in range(12) if s.step(t)]
    assert fired == [2, 5] and s.n == 140 and s.emitted == 40 and s.skipped == 0
    # capacity 130: the layer of step 2 fits (120), the one of step 5 does not; it stays due at 8 (not counted as a layer)
    s = sr.Schedule(100, 130, [em(period=3, first_step=2, max_layers=2)])
    fired = [t for t in range(8) if s.step(t)]
    assert fired == [2] and s.n == 120 and s.skipped == 1 and s.emitters[0].layers == 1
    assert s.step(8, removed=30) == [0] and s.n == 110 and s.emitters[0].layers == 2  # a sink made room
    assert s.step(11) == [] and s.skipped == 1  # max_layers reached: not due, so nothing is skipped either
    # two emitters in id order; the second does not fit behind the first
    s = sr.Schedule(100, 130, [em(), em()])
    assert s.step(0) == [0] and s.skipped == 1 and s.n == 120
    # the sinks' cadence
    assert [t for t in range(10) if sr.Schedule(1, 1, every=4).looks(t)] == [0, 4, 8]
    assert not any(sr.Schedule(1, 1, every=0).looks(t) for t in range(10))


def test_removal_renumbers_survivors_in_host_order():
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000):
        for frac in (0.0, 0.3, 0.9, 1.0):
            goes = rng.random(n) < frac
            idx = sr.new_index(goes)
            keep = sr.survivors(goes)
            if goes.all():
                assert list(keep) == [0] and idx[0] == 0 and (idx[1:] == -1).all()
                continue
            assert np.array_equal(keep, np.nonzero(~goes)[0])
            for i in range(n):  # the new index is the number of survivors with a smaller old index
                assert idx[i] == (-1 if goes[i] else int((~goes[:i]).sum()))
            x = rng.random((n, 3)).astype(np.float32)
            rho = rng.random(n).astype(np.float32)
            out = sr.compact(goes, {"positions": x, "densities": rho})
            assert np.array_equal(out["positions"], x[~goes]) and np.array_equal(out["densities"], rho[~goes])


def test_a_nan_coordinate_is_never_inside():
    inf = np.inf
    x = np.array([[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, 0.5, np.nan], [2.0, 0.5, 0.5], [1.0, 0.5, 0.5], [0.0, 0.5, 0.5]], np.float32)
    box = ((0, 0, 0), (1, 1, 1))
    assert list(sr.sink_goes([(*box, 0)], x)) == [True, False, False, False, False, True]   # [min, max): 1.0 is out, 0.0 in
    assert list(sr.sink_goes([(*box, 1)], x)) == [False, True, True, True, True, False]     # an outside sink removes a NaN
    half = ((-inf, -inf, -inf), (0.75, inf, inf))
    assert list(sr.sink_goes([(*half, 0)], x)) == [True, False, False, False, False, True]
    assert list(sr.sink_goes([(*box, 0), (*box, 1)], x)) == [True] * 6  # some sink takes it


def test_a_removal_never_empties_the_state():
    x = np.full((5, 3), 0.5, np.float32)
    goes = sr.sink_goes([((0, 0, 0), (1, 1, 1), 0)], x)
    assert goes.all()
    out = sr.compact(goes, {"positions": x, "ids": np.arange(5)})
    assert out["positions"].shape == (1, 3) and list(out["ids"]) == [0]


def test_new_particles_state():
    st = {"positions": np.zeros((2, 3), np.float32), "velocities": np.ones((2, 3), np.float32), "forces": np.ones((2, 3), np.float32),
          "densities": np.ones(2, np.float32), "pci_positions": np.ones((2, 3), np.float32)}
    out = sr.append_state(st, [[1, 2, 3]], (0, -1, 0), (0, -9, 0))
    assert out["positions"].shape == (3, 3) and list(out["forces"][2]) == [0, -9, 0] and out["densities"][2] == 0
    assert list(out["pci_positions"][2]) == [1, 2, 3] and list(out["velocities"][2]) == [0, -1, 0]


def test_the_bindings_agree_on_the_new_names():
    from dieselfluid_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "dslsph.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {"dsl_particles_append": 4, "dsl_emitter_add": 3, "dsl_emitters_clear": 1, "dsl_emit": 2, "dsl_sink_add": 3,
            "dsl_sinks_clear": 1, "dsl_particles_remove": 2}
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(dsl_(?:particles_|emit|sink)\w*)\s*\(([^)]*)\)", code)}
    assert {k: len(v.split(",")) for k, v in decl.items()} == want
    assert {k: len(_lib.EXPORTS[k][1]) for k in want} == want
    opts = {"emitters": 88, "sinks": 89, "emitted": 90, "emit_skipped": 91, "removed": 92, "sink_every": 93}
    for name, value in opts.items():
        assert re.search(r"\bDSL_OPT_%s\s*=\s*%d\b" % (name.upper(), value), code), name
        assert engine.SPHEngine.OPTIONS[name] == value
    assert re.search(r"\bDSL_K_SOURCES\s*=\s*19\b", code) and re.search(r"\bDSL_K_END\s*=\s*20\b", code)
    assert engine.KERNEL_IDS["sources"] == 19
    assert re.search(r"#define\s+DSL_MAX_EMITTERS\s+8\b", code) and re.search(r"#define\s+DSL_MAX_SINKS\s+8\b", code)
    for name in ("append_particles", "add_emitter", "clear_emitters", "emit", "add_sink", "clear_sinks", "remove_particles"):
        assert callable(getattr(engine.SPHEngine, name))
    assert "sources.hip" in _lib.UNITS
    # the structs: the header's field order and sizes (a C compiler lays dsl_emitter out with first_step on an 8-byte boundary)
    assert [f[0] for f in _lib.Emitter._fields_] == ["origin", "u", "v", "nu", "nv", "shape", "velocity", "period", "first_step",
                                                     "max_layers"]
    assert C.sizeof(_lib.Emitter) == 80 and _lib.Emitter.first_step.offset == 64 and C.sizeof(_lib.Sink) == 28
    go = open(os.path.join(ROOT, "bindings", "go", "dslsph", "dslsph.go")).read()
    for name in ["C." + k + "(" for k in want] + ["C.DSL_OPT_%s)" % k.upper() for k in opts] + [
            "C.DSL_K_SOURCES)", "func (e *Engine) AppendParticles(", "func (e *Engine) AddEmitter(", "func (e *Engine) ClearEmitters(",
            "func (e *Engine) Emit(", "func (e *Engine) AddSink(", "func (e *Engine) ClearSinks(", "func (e *Engine) RemoveParticles("]:
        assert name in go, name
    hpp = open(os.path.join(ROOT, "dieselfluid_amd", "host", "dieselfluid.hpp")).read()
    for name in [k + "(" for k in want] + ["struct Emitter", "struct Sink", "AppendParticles(", "AddEmitter(", "ClearEmitters(", "Emit(",
                                            "AddSink(", "ClearSinks(", "RemoveParticles(", "DSL_OPT_SINK_EVERY,"]:
        assert name in hpp, name
