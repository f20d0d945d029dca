"""Shared test helpers: map the product's dsl_params onto the oracle's parameter block
(the two structs are defined independently on purpose) and build seeded inputs."""
import numpy as np

from oracle import pyoracle as po


def oracle_params(p, mode=po.NEIGH_GRID, order=po.ORDER_CELL, n3=0):
    """dieselfluid_amd.Params -> oracle Params (field by field)."""
    q = po.params_reference(4)
    q.n3 = n3
    q.neigh_mode, q.neigh_order = mode, order
    # the engine's ref_density is the final D0(); NewParticleArray would multiply by mass again
    # (particle_array.go:26), so hand it over through SetReferenceDensity (particle_array.go:35-37)
    q.d0_override = p.ref_density
    for name in ("h", "mass", "ref_density", "mu", "dt", "eos_w", "eos_gamma", "eos_d0_grad", "pressure_sign",
                 "visc_running_mass", "wcsph_pressure_force", "wcsph_viscosity", "pci_max_iters", "pci_max_error",
                 "walls", "restitution", "xsph_eps", "st_kappa"):
        setattr(q, name, getattr(p, name))
    for name in ("force_reset", "external", "box_min", "box_max", "grid_min", "grid_max"):
        for a in range(3):
            getattr(q, name)[a] = getattr(p, name)[a]
    return q


def jittered_lattice(n3, amp=0.2, seed=1234, origin=(0.0, 0.0, 0.0)):
    """sph.Init lattice plus a seeded uniform jitter of +-amp*step (SURVEY 8c fixture 2)."""
    pos = po.lattice_positions(n3, origin)
    rng = np.random.default_rng(seed)
    step = np.float32(2.0 / n3)
    jit = (rng.random(pos.shape, dtype=np.float32) * np.float32(2) - np.float32(1)) * np.float32(amp) * step
    return (pos + jit).astype(np.float32)


def seeded_velocities(n, scale=0.1, seed=99):
    rng = np.random.default_rng(seed)
    return ((rng.random((n, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(2 * scale)).astype(np.float32)


def rel_err(a, b, floor=0.0):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = max(np.max(np.abs(b)), floor, 1e-30)
    return float(np.max(np.abs(a - b)) / scale)


def brute_force_step_f64(p, x, v, probe, near, force=None):
    """One WCSPH step of the build's fused force+integrate kernel, in float64, by brute force, for
    the particles `probe` (index array) of the state (x, v); `near` lists every particle within 2h of
    a probe particle.  The formulas are the reference's (std_kernel.go:33-76, model.go:92-101,
    sph_field.go:155-200,251-269 without the running-mass product, fluid.go:175-197) plus the
    build-defined wall box.  `force`: the force each probe particle carries into the step, one row per
    probe (an uploaded per-particle field); None: force_reset, the state after an Update.  The
    running-mass viscosity (visc_running_mass = 1) is accepted for mass == 1, where its product
    (force + t) * m is the plain sum.  Returns (rho_probe, x_new, v_new).  Independent of the oracle
    and of the engine: numpy only."""
    h, m = float(p.h), float(p.mass)
    PI = 3.141592653589
    A, B, Ck = 315.0 / (64.0 * PI * h ** 3), -45.0 / (PI * h ** 4), 90.0 / (PI * h ** 5)
    xn, vn = x[near].astype(np.float64), v[near].astype(np.float64)
    # densities of every particle within h of a probe particle
    xp = x[probe].astype(np.float64)
    close = np.zeros(xn.shape[0], dtype=bool)
    for k in range(xp.shape[0]):
        close |= ((xn - xp[k]) ** 2).sum(axis=1) < h * h
    rho_n = np.full(xn.shape[0], np.nan)
    for k in np.nonzero(close)[0]:
        d2 = ((xn - xn[k]) ** 2).sum(axis=1)
        msk = (d2 < h * h) & (d2 > 0)
        rho_n[k] = m * A * ((1.0 - d2[msk] / (h * h)) ** 2).sum()

    def pterm(rho):
        r = np.maximum(rho, float(p.eos_d0_grad)) / float(p.eos_d0_grad)
        return (float(p.eos_w) / float(p.eos_gamma)) * (r ** float(p.eos_gamma) - 1.0) / (rho * rho)

    pos_of = {int(g): k for k, g in enumerate(near)}
    rho_p = np.empty(xp.shape[0])
    x_new, v_new = np.empty_like(xp), np.empty_like(xp)
    dt = float(p.dt)
    for k, g in enumerate(probe):
        i = pos_of[int(g)]
        d = xn - xn[i]
        d2 = (d * d).sum(axis=1)
        msk = (d2 < h * h) & (d2 > 0)
        r = np.sqrt(d2[msk])
        rho_p[k] = rho_n[i]
        if force is None:
            F = np.array([float(p.force_reset[a]) for a in range(3)])
        else:
            F = np.asarray(force[k], dtype=np.float64).copy()
        if p.wcsph_pressure_force:
            grad = (d[msk] / r[:, None]) * (-(B * (1.0 - r / h) ** 2))[:, None]  # Grad = dir * (-O1D)
            G = ((pterm(rho_n[i]) + pterm(rho_n[msk]))[:, None] * grad).sum(axis=0)
            F = F + float(p.pressure_sign) * rho_n[i] * m * G
        if p.wcsph_viscosity:
            assert not p.visc_running_mass or float(p.mass) == 1.0, "the running-mass product is order-dependent for m != 1"
            V = (m * (vn[msk] - vn[i]) / rho_n[msk][:, None] * (Ck * (1.0 - r / h))[:, None]).sum(axis=0)
            F = F + float(p.mu) * V
        F = F + np.array([float(p.external[a]) for a in range(3)])
        vv = vn[i] + (F / m) * dt
        xx = xn[i] + vv * dt
        if p.walls:
            for a in range(3):
                if xx[a] < float(p.box_min[a]):
                    xx[a] = float(p.box_min[a])
                    if vv[a] < 0:
                        vv[a] = -vv[a] * float(p.restitution)
                if xx[a] > float(p.box_max[a]):
                    xx[a] = float(p.box_max[a])
                    if vv[a] > 0:
                        vv[a] = -vv[a] * float(p.restitution)
        x_new[k], v_new[k] = xx, vv
    return rho_p, x_new, v_new


def field_ops_f64(p, x, v_or_f, rho, probe, queries=None):
    """Div, Curl, Laplacian and Interpolate (sph_field.go:124-135,203-294) in float64, by brute force over all
    particles, for the particles `probe` (index array) of the state (x, v_or_f, rho) and at the points `queries`.
    `v_or_f` is the tensor field (velocities or forces, one row per particle), `rho` the float32 densities the
    operators read (they are an input here, not recomputed); the pressure field is the Tait EOS of those densities
    (field_types.go:39-42, model.go:92-101) with the scene's own eos_d0_grad, eos_w and eos_gamma and p0 = 0.  The
    kernel is std_kernel.go:33-76: F = A (1 - r^2/h^2)^2, Grad = dir * (-B (1 - r/h)^2), O2D = C (1 - r/h), all for
    r < h, with dir = (x_j - x_i) / r and dir = 0 at r = 0 (vector.go:322-331).  No boundary particles.

      Div_i  = sum_j (m / rho_j) t_j . Grad_ij          Curl_i = sum_j (m / rho_j) t_j x Grad_ij          (j != i)
      Lap_i  = sum_j m (f_j - f_i) / rho_j O2D(r_ij)                                                      (j != i)
      Int(q) = sum_j (m / rho_j) F(|q - x_j|) f_j                                                         (every j)

    Returns a dict: "div" (len(probe)), "curl" (len(probe), 3), "lap_density", "lap_pressure" (len(probe)) and, with
    `queries`, "interp_density", "interp_pressure" (len(queries)).  Independent of the oracle and of the engine:
    numpy only."""
    h, m = float(p.h), float(p.mass)
    PI = 3.141592653589
    A, B, Ck = 315.0 / (64.0 * PI * h ** 3), -45.0 / (PI * h ** 4), 90.0 / (PI * h ** 5)
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(v_or_f, dtype=np.float64).reshape(-1, 3)
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    probe = np.asarray(probe, dtype=np.int64).reshape(-1)
    d0, w, g = float(p.eos_d0_grad), float(p.eos_w), float(p.eos_gamma)
    press = (w / g) * ((np.maximum(rho, d0) / d0) ** g - 1.0)
    vol = m / rho
    out = {"div": np.zeros(probe.size), "curl": np.zeros((probe.size, 3)), "lap_density": np.zeros(probe.size),
           "lap_pressure": np.zeros(probe.size)}
    for k, i in enumerate(probe):
        d = x - x[i]
        r = np.sqrt((d * d).sum(axis=1))
        msk = r < h
        msk[i] = False
        d, r, j = d[msk], r[msk], np.nonzero(msk)[0]
        dirn = np.where(r[:, None] > 0, d / np.where(r > 0, r, 1.0)[:, None], 0.0)
        grad = dirn * (-(B * (1.0 - r / h) ** 2))[:, None]
        s = t[j] * vol[j][:, None]
        out["div"][k] = (s * grad).sum()
        out["curl"][k] = np.cross(s, grad).sum(axis=0)
        o2 = Ck * (1.0 - r / h)
        out["lap_density"][k] = (m * (rho[j] - rho[i]) / rho[j] * o2).sum()
        out["lap_pressure"][k] = (m * (press[j] - press[i]) / rho[j] * o2).sum()
    if queries is not None:
        q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
        out["interp_density"], out["interp_pressure"] = np.zeros(q.shape[0]), np.zeros(q.shape[0])
        for k in range(q.shape[0]):
            d = x - q[k]
            r2 = (d * d).sum(axis=1)
            j = np.nonzero(r2 < h * h)[0]
            wgt = vol[j] * A * (1.0 - r2[j] / (h * h)) ** 2
            out["interp_density"][k] = (wgt * rho[j]).sum()
            out["interp_pressure"][k] = (wgt * press[j]).sum()
    return out


def fast_velocity_tolerance(p, steps, eps_rho=2.0e-6):
    """Absolute velocity tolerance (m/s) of DSL_MATH_FAST against the oracle after `steps` steps of a
    scene with the pressure force on.  Error model: FAST densities agree with the oracle to eps_rho ~ 2e-6
    (fma + expanded r^2 instead of separately rounded operations); the Tait EOS turns that into
    gamma * eps_rho * B of pressure, the pressure gradient into about gamma * eps_rho * c_s^2 / h of
    acceleration (c_s^2 = eos_w / mass in the build's scenes), one step into that times dt of velocity.
    Measured (tools/fast_errors.py, MI355X): 0.08-0.2 of this bound after 1 step, 0.03-0.07 after 10
    (errors of successive steps do not add coherently); after ~40 steps of a developed flow the two
    trajectories part for good (a neighbour crossing r = h one step apart), which is why parity is
    checked over at most 10 steps.  Half the bound is asserted.  `eps_rho`: the density agreement the model starts
    from -- 2e-6 on a jittered lattice; a developed flow (cells of 4 to 26 particles, tile-relative coordinates up to 3.5
    cells) measures up to 5e-6 (tools/pair_diag.py), and its tests pass 6e-6."""
    cs2 = float(p.eos_w) / float(p.mass)
    return 0.5 * float(p.eos_gamma) * eps_rho * cs2 / float(p.h) * float(p.dt) * steps


SLAB_SENTINEL = np.uint32(0x7FC0DEAD)  # what a message buffer holds before a pack; a quiet-NaN pattern no record carries
SLAB_RECORD_X = 4                      # position-only record: x, y, z, id bits


def slab_message_reference(pos, vel, ids, axis, lo, hi, width_full, width, cap_full, cap_x, rec=7, pci_pos=None,
                           pci_vel=None):
    """What dsl_slab_pack has to leave in its two message buffers, word for word, written from include/dslsph.h and
    the layout comments of kernels_grid.hpp (independent of oracle_slab_engine.py).

    `pos`, `vel` (n x 3 float32) and `ids` (n int32) are the engine's state in SLOT order (download(...,
    sorted_order=True), download_ids()); `pci_pos` / `pci_vel` the predictor state in the same order, needed for
    rec = 13.  The slab owns [lo, hi) along `axis`.

    Thresholds are sums of two floats, as the product computes them: full_lo = float32(lo) + float32(width_full),
    band_lo = float32(lo) + float32(width), full_hi = float32(hi) - float32(width_full), band_hi = float32(hi) -
    float32(width).  Lower message: p < full_lo is a full record, else p < band_lo a position-only record; upper
    message: p >= full_hi full, else p >= band_hi position-only.  A NaN axis coordinate fails every comparison and
    belongs to no band; an infinite plane (a domain end) leaves its message empty.  Records are in slot order.

    Layout (32-bit words): a header of `rec` words, [0] / [1] the numbers of full / position-only records as int32
    bits, clamped to the capacities; cap_full full records of `rec` words (x y z vx vy vz id [pci x y z, pci vx vy vz]);
    cap_x position-only records of 4 words (x y z id).  Records that do not fit are dropped, the first ones in slot
    order stay.

    Returns {"lo": side, "hi": side}; a side is a dict with
      counts   (nf, nx), UNclamped
      words    uint32[(cap_full + 1) * rec + 4 * cap_x]: the message; words nobody writes hold SLAB_SENTINEL
      written  bool mask of the same length: the words the pack writes -- every other word must keep what it held
      full, xonly  slot indices of the records that were kept, in message order"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 3)
    ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
    assert rec in (7, 13) and pos.shape[0] == vel.shape[0] == ids.shape[0]
    if rec == 13:
        pci_pos = np.ascontiguousarray(pci_pos, np.float32).reshape(-1, 3)
        pci_vel = np.ascontiguousarray(pci_vel, np.float32).reshape(-1, 3)
    cap_full, cap_x = int(cap_full), int(cap_x)
    f32 = np.float32
    p = pos[:, axis]
    with np.errstate(invalid="ignore", over="ignore"):
        full_lo, band_lo = f32(lo) + f32(width_full), f32(lo) + f32(width)
        full_hi, band_hi = f32(hi) - f32(width_full), f32(hi) - f32(width)
        lo_full = p < full_lo
        lo_x = ~lo_full & (p < band_lo)
        hi_full = p >= full_hi
        hi_x = ~hi_full & (p >= band_hi)
    out = {}
    for side, full, xonly in (("lo", lo_full, lo_x), ("hi", hi_full, hi_x)):
        fi, xi = np.nonzero(full)[0], np.nonzero(xonly)[0]
        nf, nx = int(fi.size), int(xi.size)
        fi, xi = fi[:cap_full], xi[:cap_x]
        words = np.full((cap_full + 1) * rec + cap_x * SLAB_RECORD_X, SLAB_SENTINEL, np.uint32)
        written = np.zeros(words.shape, bool)
        words[0:2] = np.array([min(nf, cap_full), min(nx, cap_x)], np.int32).view(np.uint32)
        written[0:2] = True
        r = words[rec:(cap_full + 1) * rec].reshape(cap_full, rec)
        rw = written[rec:(cap_full + 1) * rec].reshape(cap_full, rec)
        k = fi.size
        r[:k, 0:3] = pos[fi].view(np.uint32)
        r[:k, 3:6] = vel[fi].view(np.uint32)
        r[:k, 6] = ids[fi].view(np.uint32)
        if rec == 13:
            r[:k, 7:10] = pci_pos[fi].view(np.uint32)
            r[:k, 10:13] = pci_vel[fi].view(np.uint32)
        rw[:k, :] = True
        x = words[(cap_full + 1) * rec:].reshape(cap_x, SLAB_RECORD_X)
        xw = written[(cap_full + 1) * rec:].reshape(cap_x, SLAB_RECORD_X)
        k = xi.size
        x[:k, 0:3] = pos[xi].view(np.uint32)
        x[:k, 3] = ids[xi].view(np.uint32)
        xw[:k, :] = True
        out[side] = {"counts": (nf, nx), "words": words, "written": written, "full": fi, "xonly": xi}
    return out
