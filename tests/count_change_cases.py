"""The scenes and the oracle-side expected values of tests/test_gpu_count_change.py: the step's fast paths on a handle whose
particle count has changed (include/dslsph.h: dsl_particles_append, dsl_particles_remove, emitters and sinks in the drivers).
tests/test_count_change_cpu.py asserts the conditions these scenes have to meet, with the oracle alone.

  skin and fall-back scenes   the 16^3 dam-break (4096 particles) with capacity 6144: the smallest scene in which the skin
                              step is usable
  append block                7 x 7 x 6 = 294 particles at spacing dx, on the floor, against the fluid's free face x = 1
                              (`ix0` lattice layers further out for a second block): 4096 + 294 = 4390, no multiple of 64,
                              beyond 4352 = 17 x 256
  removal                     one sink, the slab 6.5 dx <= x < 8.5 dx: two half layers and a whole one, so which host indices
                              go is decided by the jitter and kept and removed indices interleave
  small scenes                the n3 = 6 dam-break (216 particles) with capacity 1024, as tests/test_gpu_sources.py
"""
import numpy as np

import helpers
import sources_ref as sr
from oracle import pyoracle as po

f32 = np.float32
EXACT, FAST = 0, 1
INF = float("inf")
N3, CAP = 16, 6144
SMALL_N3, SMALL_CAP = 6, 1024
BLOCK_DIMS = (7, 7, 6)                   # x, z, y: 294 particles
K_SKIN, K_FORMS = 10, 5                  # steps after the count change
SEED_SCALE = 0.05                        # the skin tests' seeded velocities, in sound speeds
SKIN_PREDICT = 0.8                       # DSL_OPT_SKIN_PREDICT's default (engine.hpp: kSkinPredict)
SKIN_TAU_STEPS = 16.0                    # kernels_skin.hpp: kSkinTauSteps
PCI = ("pci_positions", "pci_velocities")


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def scene(math_mode, n3=N3, capacity=CAP, pci=False):
    """(params, positions) of the n3^3 dam-break with room for `capacity` particles; pci: PCISPH set up as tests/test_gpu_sources.py
    and tests/test_gpu_developed.py do on this scene (every iteration runs)"""
    from dieselfluid_amd import scenes
    p, pos = scenes.dambreak_scene(n3, math_mode=math_mode)
    p.capacity = capacity
    if pci:
        p.pci_max_iters = 3
        p.eos_w = p.eos_w / 3
        p.delta = 1.0e-7
        p.pci_max_error = -1.0
    return p, pos


def with_count(p, n):
    """a copy of the parameters for a fresh handle of n particles"""
    q = type(p).from_buffer_copy(p)
    q.n_particles = int(n)
    return q


def reset(p, n):
    return np.tile(np.array(p.force_reset[:], dtype=f32), (int(n), 1))


def seeded(p, n):
    """the seeded velocities of test_skin_steps_match_the_oracle_over_reuse_and_rebuild, at 0.05 c_s instead of its 0.03:
    |v| dt up to ~0.02 h per step.  The window here starts after six steps, in which viscosity has taken a third of them:
    at 0.03 c_s a skin of 0.2 (budget 0.1 h) sees no second rebuild within ten steps (tests/test_count_change_cpu.py holds
    the rebuild rule to this scale)"""
    cs = float(np.sqrt(p.eos_w / p.mass))
    return helpers.seeded_velocities(int(n), scale=SEED_SCALE * cs)


def append_block(n3=N3, ix0=0):
    """(294, 3) float32: the lattice ((ix0 + a + 0.5) dx + 1, (b + 0.5) dx, (c + 0.5) dx), a < 7, b < 6, c < 7"""
    dx = 1.0 / n3
    nx, nz, ny = BLOCK_DIMS
    a, b, c = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    abc = np.stack([a + ix0, b, c], axis=-1).reshape(-1, 3).astype(np.float64)
    return ((abc + 0.5) * dx + np.array([1.0, 0.0, 0.0])).astype(f32)


def sink_slab(n3=N3, lo=6.5, hi=8.5):
    """(box_min, box_max, outside) of the removal's sink: lo dx <= x < hi dx, the whole box in y and z"""
    dx = 1.0 / n3
    return ((lo * dx, -INF, -INF), (hi * dx, INF, INF), 0)


def removal_is_sound(goes, n):
    """the removal's conditions on the flags `goes` of n particles: 5 % to 25 % go, the removed host indices are no suffix
    of the range and interleave with kept ones, and the count that is left is no multiple of 64"""
    goes = np.asarray(goes, dtype=bool)
    gone = int(goes.sum())
    idx = np.nonzero(goes)[0]
    kept_between = int((~goes[idx[0]:idx[-1] + 1]).sum()) if gone else 0
    runs = int(np.count_nonzero(np.diff(goes.astype(np.int8)) == 1)) + int(goes[0]) if gone else 0
    return (goes.shape[0] == n and 0.05 * n <= gone <= 0.25 * n and idx[-1] != n - 1 and kept_between > 0 and runs >= 8
            and (n - gone) % 64 != 0)


def appended(st, block, p):
    """the state with `block` behind it, at rest (sources_ref.append_state)"""
    return sr.append_state(st, block, None, p.force_reset[:])


def removed(st, sink):
    """(goes, the state after the sink acted)"""
    goes = sr.sink_goes([sink], st["positions"])
    return goes, sr.compact(goes, st)


def oracle_from(p, st):
    """an oracle system of the state `st` (positions, velocities and, when it has them, forces: force_reset otherwise)"""
    x = st["positions"]
    frc = st["forces"] if "forces" in st else reset(p, x.shape[0])
    return po.OracleSPH.from_state(helpers.oracle_params(p), x, vel=st["velocities"], force=frc)


def oracle_wcsph(p, st, steps, trajectory=False):
    """positions, velocities and densities `steps` WCSPH steps of the oracle after `st`; trajectory: the list of
    (positions, velocities) after every step as well"""
    ora = oracle_from(p, st)
    path = []
    for _ in range(steps):
        ora.wcsph_step(1)
        if trajectory:
            path.append((ora.positions(), ora.velocities()))
    out = dict(positions=ora.positions(), velocities=ora.velocities(), densities=ora.densities())
    ora.close()
    return (out, path) if trajectory else out


def oracle_pcisph(p, st, steps=1):
    """one PCISPH system of the oracle that starts from `st` WITH its predictor state (written through the oracle's array
    views: dslo_pcisph_begin only copies positions and velocities into it), stepped `steps` times.  Returns the state and
    (iterations, error) of the last step"""
    ora = oracle_from(p, st)
    ora.delta = p.delta
    ora.pcisph_begin()
    ora._view(ora._L.dslo_pci_positions, 3)[:] = po.f32(st["pci_positions"]).reshape(-1, 3)
    ora._view(ora._L.dslo_pci_velocities, 3)[:] = po.f32(st["pci_velocities"]).reshape(-1, 3)
    ora.pcisph_step(steps)
    out = dict(positions=ora.positions(), velocities=ora.velocities(), densities=ora.densities(),
               pci_positions=ora.pci_positions(), pci_velocities=ora.pci_velocities())
    info = (int(ora.pci_iters), f32(ora.pci_error))
    ora.close()
    return out, info


def skin_rebuilds(p, st, path, skin, predict=SKIN_PREDICT):
    """Which of the len(path) skin steps after the state `st` rebuild, by the library's rule (kernels_skin.hpp:
    k_skin_decide) on the oracle's trajectory `path`: the first step of an episode rebuilds; a build's reference positions
    are x + tau v with tau = min(predict * budget / max |v|, 16 dt) (0 at an episode's first build, where max |v| is not
    known yet); a step rebuilds when, after the step before it, a particle is further than budget = s h / 2 (1 - 1e-3)
    from its reference.  A model in float64 -- good for 'are there rebuilds and re-use steps', not for their exact places."""
    h, dt = float(p.h), float(p.dt)
    budget = 0.5 * skin * h * (1.0 - 1.0e-3)
    x, v = st["positions"].astype(np.float64), st["velocities"].astype(np.float64)
    out, ref, vmax = [], None, None
    for xn, vn in path:
        far = ref is None or np.sqrt(((x - ref) ** 2).sum(axis=1)).max() > budget
        if far:
            tau = 0.0 if not vmax else min(predict * budget / vmax, SKIN_TAU_STEPS * dt)
            ref = x + tau * v
        out.append(bool(far))
        x, v = xn.astype(np.float64), vn.astype(np.float64)
        vmax = float(np.sqrt((v * v).sum(axis=1)).max())
    return out


def min_distance(x):
    from scipy.spatial import cKDTree
    d, _ = cKDTree(np.asarray(x, dtype=np.float64)).query(x, k=2)
    return float(d[:, 1].min())


def field_queries(pos, h, seed=17):
    """query points for Interpolate: ~150 between particles (up to h / 4 off one), ~50 exactly on particles, the appended
    block's among both, and 50 more than h outside the fluid"""
    rng = np.random.default_rng(seed)
    n = pos.shape[0]
    a = pos[:: max(n // 150, 1)]
    between = a + ((rng.random(a.shape) - 0.5) * 0.5 * h).astype(f32)
    on = pos[1:: max(n // 50, 1)]
    out = (np.array([2.5, 1.0, 1.0]) + 1.5 * h + rng.random((50, 3)) * 3 * h).astype(f32)
    return np.ascontiguousarray(np.concatenate([between, on, pos[-5:], out]), dtype=f32)


# ---- the small scenes (n3 = 6) ----
# the emitter of tests/test_gpu_sources.py: 20 particles a layer, 216 -> 256 after two layers, 276 after three
FACE = dict(origin=(0.15, 1.08, 0.12), u=(0.16, 0.0, 0.012), v=(0.01, 0.004, 0.17), nu=5, nv=4, velocity=(0.0, -60.0, 0.0))


def ref_emitter(d, **kw):
    return sr.Emitter(d["origin"], d["u"], d["v"], d["nu"], d["nv"], d["velocity"], shape=d.get("shape", 0), **kw)


def driver_changes(st, s, p, emitter, sinks, every):
    """what the step drivers do to the state `st` (host order) at the start of step s: the sinks when s % every == 0, then
    the emitter's layer when it is due (tests/sources_ref.py).  Returns (state, removed)"""
    gone = 0
    if sinks and every and s % every == 0:
        goes = sr.sink_goes(sinks, st["positions"])
        gone = int(goes.sum())
        if gone:
            st = sr.compact(goes, st)
    if emitter is not None and emitter.due(s):
        st = sr.append_state(st, emitter.points, emitter.velocity, p.force_reset[:])
        emitter.layers += 1
    return st, gone


# the sinks of the small scenes
PCI_SINK = ((-INF, -INF, -INF), (0.5 / SMALL_N3, INF, INF), 0)  # through the first lattice layer in x: about half of it goes
COL_SINK = ((0.7, -INF, -INF), (INF, INF, INF), 0)              # the block's far end in x, and what the emitter sends there
REC_SINK = ((0.3, -INF, -INF), (INF, INF, INF), 0)              # all but the first two lattice layers in x


def plate():
    """a horizontal plate through the top of the block, under the emitter's face: 18 triangles"""
    from dieselfluid_amd import scenes
    return scenes.quad_mesh((-0.1, 0.9, -0.1), (-0.1, 0.9, 1.1), (1.3, 0.9, 1.1), (1.3, 0.9, -0.1), (0.0, 1.0, 0.0), subdiv=3)


SPHERE_C, SPHERE_R = np.array([0.5, 0.75, 0.4]), 0.25  # a sphere in the top of the block, its pole just under the face
SPHERE_O, SPHERE_S, SPHERE_D = (0.1, 0.35, 0.0), (0.05, 0.05, 0.05), (17, 17, 17)


def sphere_volume():
    import sdf_ref
    x, y, z = (a.astype(np.float64) for a in sdf_ref.axes(SPHERE_O, SPHERE_S, SPHERE_D))
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return (np.sqrt((xx - SPHERE_C[0]) ** 2 + (yy - SPHERE_C[1]) ** 2 + (zz - SPHERE_C[2]) ** 2) - SPHERE_R).astype(f32)
