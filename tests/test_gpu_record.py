"""GPU: the frame recorder (include/dslsph.h: dsl_recorder_set, dsl_record_now, dsl_record_poll / peek / release / read;
csrc/record.hip) held bit for bit to tests/record_ref.py, the numpy restatement of the build-defined rule, and to
dsl_download.  No tolerances anywhere.  The scene is the n3 = 6 dam-break (216 particles) with capacity 1024 unless said
otherwise: a few hundred particles, where the count still crosses a wave (64) and a workgroup (256).

The capture refusal (a step that would record while the caller's stream is being captured returns DSL_ERR_UNSUPPORTED) is
not exercised here: it would need a capture that is then abandoned with an error inside it; it is covered by review of
record_frame_due, which asks hipStreamIsCapturing exactly as sources_step does.  DSL_ERR_NOMEM from dsl_recorder_set needs a
host that is out of pinned memory and is covered by review as well."""
import ctypes as C

import numpy as np
import pytest

import helpers
import record_ref as rr

pytestmark = pytest.mark.gpu

f32 = np.float32
EXACT, FAST = 0, 1
CAP = 1024
N0 = 216
ALL = rr.VELOCITY | rr.DENSITY
INF = float("inf")
FACE = dict(origin=(0.15, 1.08, 0.12), u=(0.16, 0.0, 0.012), v=(0.01, 0.004, 0.17), nu=5, nv=4, velocity=(0.0, -60.0, 0.0))


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _dam(math_mode, pci=False, n3=6, skin=0.0, vel=None):
    from dieselfluid_amd import SPHEngine, scenes
    p, pos = scenes.dambreak_scene(n3, math_mode=math_mode)
    p.capacity = max(CAP, n3 ** 3)
    if pci:  # (as tests/test_gpu_sources.py sets PCISPH up on this scene: every iteration runs)
        p.pci_max_iters = 3
        p.eos_w = p.eos_w / 3
        p.delta = 1.0e-7
        p.pci_max_error = -1.0
    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    if vel is not None:
        eng.upload("velocities", vel)
    eng.reset_forces()
    eng.set_option("skin", skin)
    return eng, p, pos


def _state(eng):
    n = eng.n_fluid
    return eng.download("positions")[:n], eng.download("velocities"), eng.download("densities")


def _ref(eng, p, step, **kw):
    """the reference's frame of the engine's current state"""
    x, v, d = _state(eng)
    return rr.build_frame(step, x, v, d, dt=p.dt, **kw)


def _refused(code, word, fn, *a, **kw):
    from dieselfluid_amd import DslError
    with pytest.raises(DslError) as e:
        fn(*a, **kw)
    assert "error %d:" % code in str(e.value) and word in str(e.value), str(e.value)


# ---- 1. one frame, float32, everything ----
def test_a_float32_frame_is_the_three_downloads_and_the_reference_header():
    from dieselfluid_amd import animation
    eng, p, _ = _dam(EXACT)
    eng.wcsph_step(5)
    ids = eng.download_ids()
    assert not np.array_equal(ids, np.arange(N0))  # (the slots are not in host order: the pack has a map to follow)
    spec = eng.set_recorder(fields=("velocities", "densities"), slots=2)
    eng.record_now()
    assert eng.record_poll()[0] == 1
    got = eng.read_frame()
    x, v, d = _state(eng)
    assert d.all()
    assert len(got) == eng.record_frame_bytes(spec, N0) == rr.frame_layout(N0, 1, ALL, rr.F32)["bytes"] == 128 + 2688 + 2688 + 896
    fr = animation.decode_frame(got)
    assert _same(fr["positions"], x) and _same(fr["velocities"], v) and _same(fr["densities"], d)
    want = rr.build_frame(5, x, v, d, fields=ALL, dt=p.dt)
    assert got == want
    h = rr.parse_header(got)
    assert (h["magic"], h["header_bytes"], h["frame_bytes"], h["step"], h["n_particles"], h["count"], h["stride"], h["fields"],
            h["encoding"], h["auto_box"]) == (0x464C5344, 128, len(got), 5, N0, N0, 1, 3, 0, 0)
    assert h["finite"] == N0 and h["dt"] == f32(p.dt) and h["zero"] == bytes(24)
    assert _same(h["bounds_min"], x.min(axis=0)) and _same(h["bounds_max"], x.max(axis=0))  # (no zero among them: min is decided)
    assert not h["box_min"].any() and not h["box_max"].any()
    eng.close()


# ---- 2. strides ----
@pytest.mark.parametrize("stride", [3, 7, N0 + 5])
def test_a_strided_frame_is_the_decimated_download(stride):
    from dieselfluid_amd import animation
    eng, p, _ = _dam(EXACT)
    eng.wcsph_step(5)
    eng.set_recorder(stride=stride, fields=ALL)
    eng.record_now()
    got = eng.read_frame()
    x, v, d = _state(eng)
    fr = animation.decode_frame(got)
    assert fr["count"] == -(-N0 // stride) and fr["n_particles"] == N0
    assert _same(fr["positions"], eng.download_decimated("positions", stride))
    assert _same(fr["velocities"], eng.download_decimated("velocities", stride)) and _same(fr["velocities"], v[::stride])
    assert _same(fr["densities"], d[::stride])
    assert got == rr.build_frame(5, x, v, d, stride=stride, fields=ALL, dt=p.dt)
    eng.close()


# ---- 3. Q16 on crafted positions ----
def _crafted():
    """x carries the clamps and the ties against the box [0, 65535 * 2^-17] (scale exactly 2^17); y is -0.0 or +0.0 everywhere
    (the two extremes of the axis: the key order decides minimum and maximum, and hi - lo = 0 gives scale 0); z is one value
    (hi == lo bit for bit); particle 7 has a NaN y"""
    rng = np.random.default_rng(11)
    x = np.zeros((N0, 3), f32)
    x[:, 0] = rng.uniform(-0.1, 0.7, N0).astype(f32)
    x[0, 0], x[1, 0] = -1.0, 1.0                                       # below and above the box: 0 and 65535
    x[2, 0], x[3, 0] = f32(1000.5) * f32(2.0 ** -17), f32(1001.5) * f32(2.0 ** -17)  # exact ties: 1000 and 1002
    x[4, 0], x[5, 0] = 0.0, f32(65535.0) * f32(2.0 ** -17)             # the box's ends
    x[:, 1] = np.where(rng.random(N0) < 0.5, f32(-0.0), f32(0.0))
    x[10, 1], x[11, 1] = -0.0, 0.0
    x[7, 1] = np.nan
    x[:, 2] = 0.25
    v = rng.normal(0.0, 3.0, (N0, 3)).astype(f32)
    v[0], v[1], v[2] = (1.0e-6, -1.0e-6, 2.0 ** -25), (1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -1.0 - 2.0 ** -11), (7.0e4, -7.0e4, 65519.996)
    v[3] = (65520.0, 2.0 ** -24, 3.0e-8)
    d = rng.uniform(900.0, 1100.0, N0).astype(f32)
    d[0], d[1], d[2] = 1.0e-6, 1.0 + 2.0 ** -11, 7.0e4
    return x, v, d


@pytest.mark.parametrize("box", ["fixed", "auto"])
def test_q16_frames_are_the_references_on_clamps_ties_nan_and_signed_zeros(box):
    from dieselfluid_amd import animation
    eng, p, _ = _dam(EXACT)
    x, v, d = _crafted()
    eng.upload("positions", x)
    eng.upload("velocities", v)
    eng.upload("densities", d)
    bx = ((0.0, -0.0, 0.25), (float(f32(65535.0) * f32(2.0 ** -17)), 0.0, 0.25)) if box == "fixed" else None
    eng.set_recorder(fields=ALL, encoding="q16", box=bx)
    eng.record_now()
    got = eng.read_frame()
    want = rr.build_frame(0, x, v, d, fields=ALL, encoding=rr.Q16, box=bx, dt=p.dt)
    h, lay = rr.parse_header(got), rr.frame_layout(N0, 1, ALL, rr.Q16)
    q = np.frombuffer(got, np.uint16, 3 * N0, lay["pos"]).reshape(N0, 3)
    hv = np.frombuffer(got, np.uint16, 3 * N0, lay["vel"]).reshape(N0, 3)
    hd = np.frombuffer(got, np.uint16, N0, lay["rho"])
    print("header", h, "q[:12]", q[:12].tolist(), "v[:4]", [[hex(t) for t in r] for r in hv[:4]], "d[:3]", [hex(t) for t in hd[:3]])
    # the rule's corners, stated by hand: they hold for the reference and therefore for the library
    assert h["finite"] == N0 - 1 and h["auto_box"] == (0 if bx else 1)
    assert _bits(h["bounds_min"])[1] == 0x80000000 and _bits(h["bounds_max"])[1] == 0 and _bits(h["bounds_min"])[2] == _bits(h["bounds_max"])[2]
    assert h["bounds_min"][0] == -1.0 and h["bounds_max"][0] == 1.0
    assert not q[:, 1].any() and not q[:, 2].any()  # (scale 0 on both axes; the NaN falls to 0 as well)
    if bx:
        assert q[0, 0] == 0 and q[1, 0] == 65535 and q[2, 0] == 1000 and q[3, 0] == 1002 and q[4, 0] == 0 and q[5, 0] == 65535
    else:
        assert q[0, 0] == 0 and q[1, 0] == 65535 and _same(h["box_min"], h["bounds_min"]) and _same(h["box_max"], h["bounds_max"])
    assert list(hv[0]) == [0x0011, 0x8011, 0x0000] and list(hv[1]) == [0x3C00, 0x3C02, 0xBC00] and list(hv[2]) == [0x7C00, 0xFC00, 0x7BFF]
    assert list(hv[3]) == [0x7C00, 0x0001, 0x0001] and list(hd[:3]) == [0x0011, 0x3C00, 0x7C00]
    assert got == want
    fr = animation.decode_frame(got)
    assert _same(fr["positions"][:, 0], rr.q16_decode(q[:, 0], h["box_min"][0], h["box_max"][0]))
    assert eng.get_option("record_frames") == 1 and eng.stats().steps == 0  # (one-shot: no step followed)
    eng.close()


# ---- 4. counts across a wave and a workgroup ----
@pytest.mark.parametrize("n3,extra", [(6, 60), (8, 0)], ids=["276", "512"])
def test_counts_that_cross_a_wave_and_fill_two_workgroups(n3, extra):
    eng, p, _ = _dam(EXACT, n3=n3)
    eng.wcsph_step(3)
    if extra:
        rng = np.random.default_rng(3)
        eng.append_particles(rng.uniform(1.2, 1.8, (extra, 3)).astype(f32), rng.normal(0, 1, (extra, 3)).astype(f32))
    n = n3 ** 3 + extra
    assert eng.n == n == (276 if extra else 512)
    for kw in (dict(fields=ALL), dict(fields=ALL, stride=3), dict(fields=ALL, encoding=rr.Q16), dict(fields=rr.DENSITY, encoding=rr.Q16, stride=5)):
        eng.set_recorder(slots=1, **{k: v for k, v in kw.items()})
        eng.record_now()
        assert eng.read_frame() == _ref(eng, p, 3, **kw), kw
    eng.close()


def test_boundary_particles_and_lsh_ref_record_the_fluid_only():
    from dieselfluid_amd import SPHEngine
    eng, p, _ = _dam(EXACT)
    g = np.linspace(0.0, 1.0, 5, dtype=f32)
    wall = np.stack(np.meshgrid(g, f32(-0.1), g, indexing="ij"), axis=-1).reshape(-1, 3).astype(f32)
    eng.add_boundary_particles(wall)
    eng.wcsph_step(2)
    assert eng.n == N0 + 25 and eng.n_fluid == N0
    eng.set_recorder(fields=ALL, stride=2)
    eng.record_now()
    assert eng.read_frame() == _ref(eng, p, 2, fields=ALL, stride=2)
    eng.close()
    from dieselfluid_amd.engine import reference_params
    from oracle import pyoracle as po
    pos = helpers.jittered_lattice(8, 0.3)

    def lsh():
        q = reference_params(8)
        q.neigh_mode, q.math_mode = 0, EXACT  # DSL_NEIGH_LSH_REF
        e = SPHEngine(q, device=0)
        e.set_hash_vectors(po.default_hash_vectors(5))
        e.upload("positions", pos)
        return e, q

    eng, p = lsh()
    eng.set_recorder(fields=ALL, every=2, slots=2)
    eng.wcsph_step(3)
    fresh, _ = lsh()
    assert eng.read_frame() == _ref(fresh, p, 0, fields=ALL)
    fresh.wcsph_step(2)
    assert eng.read_frame() == _ref(fresh, p, 2, fields=ALL)
    fresh.close()
    eng.close()


# ---- 5. the schedule ----
def _advance(eng, how, steps):
    if how == "one":
        eng.wcsph_step(steps)
    elif how == "twelve":
        for _ in range(steps):
            eng.wcsph_step(1)
    elif how == "pci-one":
        eng.pcisph_step(steps)
    elif how == "pci-twelve":
        for _ in range(steps):
            eng.pcisph_step(1)
    else:  # the phases a host drives itself
        for _ in range(steps):
            eng.pcisph_phase(0)
            for _ in range(3):
                eng.pcisph_phase(1)
                eng.pcisph_phase(2)
            eng.pcisph_phase(3)


@pytest.mark.parametrize("mode", ["wcsph-exact", "wcsph-fast", "pcisph"])
def test_frames_fall_at_steps_2_5_8_however_the_steps_are_grouped(mode):
    pci = mode == "pcisph"
    math = FAST if mode == "wcsph-fast" else EXACT
    # every frame against a fresh handle stepped s steps and downloaded
    want = {}
    for s in (2, 5, 8):
        fresh, p, _ = _dam(math, pci=pci)
        if pci:
            fresh.pcisph_begin()
        _advance(fresh, "pci-one" if pci else "one", s)
        want[s] = _ref(fresh, p, s, fields=ALL)
        fresh.close()
    for how in (("pci-one", "pci-twelve", "pci-phases") if pci else ("one", "twelve")):
        eng, p, _ = _dam(math, pci=pci)
        if pci:
            eng.pcisph_begin()
        eng.set_recorder(every=3, first_step=2, max_frames=3, fields=ALL, slots=4)
        _advance(eng, how, 12)
        eng.sync()
        assert eng.record_poll() == (3, 3, 0), how
        for s in (2, 5, 8):
            assert eng.read_frame() == want[s], (how, s)
        assert eng.record_poll() == (3, 0, 0) and eng.stats().steps == 12
        eng.close()


# ---- 6. the ring ----
def test_the_ring_drops_whole_frames_and_hands_them_out_in_order():
    eng, p, _ = _dam(EXACT)
    want = {}
    fresh, _, _ = _dam(EXACT)
    for s in range(8):
        want[s] = _ref(fresh, p, s)
        fresh.wcsph_step(1)
    fresh.close()
    eng.set_recorder(slots=2, max_frames=4)
    eng.wcsph_step(5)  # frames 0 and 1 land, 2, 3 and 4 find no released slot
    eng.sync()
    assert eng.record_poll() == (2, 2, 3)
    assert (eng.get_option("record_frames"), eng.get_option("record_ready"), eng.get_option("record_dropped")) == (2, 2, 3)
    _refused(-3, "released", eng.record_now)  # DSL_ERR_NOMEM: the ring is full, and nothing changed
    assert eng.record_poll() == (2, 2, 3)
    view = eng.peek_frame()
    first = bytes(view)
    assert first == want[0]
    eng.release_frame()
    eng.wcsph_step(1)  # step 5's frame takes the released slot: the drops did not use max_frames up
    peeked = eng.peek_frame()
    held = bytes(peeked)
    assert held == want[1]
    eng.wcsph_step(2)  # 6 and 7 dropped; the peeked frame stays as it is
    eng.sync()
    assert bytes(peeked) == held and eng.record_poll() == (3, 2, 5)
    assert eng.read_frame() == want[1] and eng.read_frame() == want[5]  # FIFO
    eng.record_now()  # the fourth and last frame: a one-shot frame counts towards max_frames
    assert eng.read_frame() == _ref(eng, p, 8)
    _refused(-1, "max_frames", eng.record_now)
    eng.wcsph_step(2)
    eng.sync()
    assert eng.record_poll() == (4, 0, 5)  # (used up: nothing recorded, nothing dropped)
    eng.close()


# ---- 7. inside a skin episode ----
def test_frames_inside_a_skin_episode_follow_the_devices_map():
    n3 = 16
    from dieselfluid_amd import scenes
    p0, _ = scenes.dambreak_scene(n3, math_mode=FAST)
    vel = helpers.seeded_velocities(n3 ** 3, scale=0.03 * float(np.sqrt(p0.eos_w / p0.mass)))
    want = {}
    for s in range(11):
        fresh, p, _ = _dam(FAST, n3=n3, skin=0.1, vel=vel)
        fresh.wcsph_step(s)
        if s:
            assert fresh.get_option("skin_steps") == s
        want[s] = _ref(fresh, p, s, fields=ALL)
        fresh.close()
    eng, p, _ = _dam(FAST, n3=n3, skin=0.1, vel=vel)
    eng.set_recorder(fields=ALL, slots=12)
    eng.wcsph_step(10)
    steps, rebuilds = eng.get_option("skin_steps"), eng.get_option("skin_rebuilds")
    assert steps == 10 and 2 <= rebuilds < 10, (steps, rebuilds)  # (the recorder kept the episode alive; the map flipped on the device)
    eng.sync()
    assert eng.record_poll() == (10, 10, 0)
    for s in range(10):
        assert eng.read_frame() == want[s], s
    assert eng.get_option("skin_steps") == 10  # (reading frames settles nothing)
    assert _ref(eng, p, 10, fields=ALL) == want[10]  # the final state is the one of a run without a recorder
    eng.close()


# ---- 8. read-only, and off ----
def test_a_recorder_changes_no_bit_of_the_run_and_frees_what_it_took():
    runs = []
    for rec in (False, True):
        eng, p, _ = _dam(EXACT)
        eng.wcsph_step(1)
        base = eng.get_option("device_bytes")
        if rec:
            spec = eng.set_recorder(fields=ALL, slots=16)
            took = eng.get_option("device_bytes") - base
            assert took == 2 * eng.record_frame_bytes(spec, CAP) + 32
            eng.set_recorder(None)
            assert eng.get_option("device_bytes") == base
            eng.set_recorder(fields=ALL, slots=16)
        assert eng.add_emitter(**FACE) == 0 and eng.add_sink((-INF, -INF, -INF), (INF, 0.1, INF)) == 0
        eng.set_option("sink_every", 2)
        counts = []
        for _ in range(12):
            counts.append(eng.n)
            eng.wcsph_step(1)
        if rec:
            eng.sync()
            assert eng.record_poll() == (12, 12, 0)
            seen = [rr.parse_header(eng.read_frame())["n_particles"] for _ in range(12)]
            assert seen == counts  # (frame s: N before step s's sinks and emitters)
            assert len(set(seen)) > 6
        else:
            assert eng.get_option("device_bytes") >= base and eng.record_poll() == (0, 0, 0)
        runs.append((counts, _state(eng)))
        eng.close()
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert _same(a, b)


def test_device_bytes_do_not_move_without_a_recorder():
    eng, p, _ = _dam(EXACT)
    eng.wcsph_step(2)
    base = eng.get_option("device_bytes")
    eng.wcsph_step(2)
    assert eng.get_option("device_bytes") == base
    for name in ("record_frames", "record_dropped", "record_ready", "record_pack_ms", "record_copy_ms"):
        assert eng.get_option(name) == 0
    eng.timing_enable(1)
    eng.set_recorder(fields=ALL)
    eng.wcsph_step(1)
    assert eng.get_option("record_pack_ms") > 0 and eng.get_option("record_copy_ms") > 0
    eng.timing_enable(0)
    eng.read_frame()
    eng.wcsph_step(1)
    assert eng.get_option("record_pack_ms") == 0 and eng.get_option("record_copy_ms") == 0
    eng.close()


# ---- 9. refusals ----
def test_every_refusal_names_its_field_and_changes_nothing():
    from dieselfluid_amd import SPHEngine
    eng, p, _ = _dam(EXACT)
    spec = SPHEngine.recorder_spec
    good = eng.set_recorder(fields=ALL, slots=2)
    eng.record_now()
    for word, kw in (("every", dict(every=0)), ("stride", dict(stride=0)), ("slots", dict(slots=0)), ("slots", dict(slots=65)),
                     ("first_step", dict(first_step=-1)), ("max_frames", dict(max_frames=-1)), ("fields", dict(fields=4)),
                     ("encoding", dict(encoding=2)), ("box_min", dict(encoding="q16", box=((0, 0, 1), (1, 1, 0)))),
                     ("box_min", dict(encoding="q16", box=((0, 0, 0), (1, INF, 1)))),
                     ("box_min", dict(encoding="q16", box=((0, float("nan"), 0), (1, 1, 1))))):
        bad = spec(**kw)
        assert eng.record_frame_bytes(bad, N0) == 0, kw
        _refused(-1, word, eng.set_recorder, bad)
    assert eng.record_frame_bytes(good, 0) == 0 and eng.record_frame_bytes(good, N0) > 0
    assert eng.record_poll() == (1, 1, 0) or eng.record_poll()[0] == 1  # the recorder that was set is still there, with its frame
    # a bytes argument that is too small, then the frame itself
    buf = (C.c_uint8 * 4096)()
    assert eng._L.dsl_record_read(eng._h, buf, 100) == -1 and b"bytes" in eng._L.dsl_last_error(eng._h)
    frame = eng.read_frame()
    assert frame == _ref(eng, p, 0, fields=ALL)
    for fn in (eng.peek_frame, eng.read_frame, eng.release_frame):  # nothing to give
        _refused(-1, "no unreleased frame", fn)
    eng.set_recorder(None)
    for fn in (eng.peek_frame, eng.read_frame, eng.release_frame):
        _refused(-1, "no unreleased frame", fn)
    _refused(-1, "no recorder", eng.record_now)
    # a slab handle, both ways round
    eng.set_recorder(fields=ALL)
    _refused(-4, "recorder", eng.slab_config, 0, -10.0, 10.0)
    eng.set_recorder(None)
    eng.slab_config(0, -10.0, 10.0)
    _refused(-4, "slab", eng.set_recorder, spec())
    eng.slab_config(-1, -10.0, 10.0)
    eng.set_recorder(fields=ALL)  # (out of slab mode it works again)
    eng.record_now()
    assert eng.read_frame() == frame
    # host order gone
    eng.set_ids(np.arange(N0, dtype=np.int32)[::-1].copy())
    _refused(-4, "dsl_set_ids", eng.record_now)
    _refused(-4, "dsl_set_ids", eng.wcsph_step, 1)
    _refused(-4, "dsl_set_ids", eng.set_recorder, spec())
    assert eng.stats().steps == 0
    eng.set_recorder(None)
    eng.wcsph_step(1)
    eng.close()
