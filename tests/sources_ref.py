"""Sources and sinks, the rule (include/dslsph.h: dsl_particles_append .. dsl_particles_remove) in numpy, operation for
operation: what csrc/sources.hip has to compute, bit for bit.  The rule is build-defined (the reference has no sources)
and the same in both math modes.

  layer_points(nu, nv, shape)      the kept lattice points (a, b) of a face, b ascending and inside it a ascending.  shape 0:
                                   every point; shape 1, the ellipse inscribed in the rectangle: (a, b) is kept when
                                   (2a - (nu-1))^2 nv^2 + (2b - (nv-1))^2 nu^2 <= (nu nv)^2, in integers
  layer_positions(e)               per component c: (origin_c + float32(a) * u_c) + float32(b) * v_c, every product and sum
                                   rounded once to float32
  Schedule                         which emitters emit at step s, what is skipped, in ascending id; sinks first
  sink_goes(sinks, x)              inside = (x_a >= min_a && x_a < max_a) on all three axes, false for a NaN; a particle
                                   goes when, for some sink, inside != outside
  compact(goes, arrays)            survivors keep their relative host order; never empty: host index 0 stays when all go
  append_state(state, x, v, p)     the state of new particles: force = force_reset, pressure 0, density 0, predictor state
                                   = position and velocity
"""
import numpy as np

f32 = np.float32


def layer_points(nu, nv, shape=0):
    """(M, 2) int64: the kept (a, b), b ascending, inside it a ascending"""
    nu, nv = int(nu), int(nv)
    out = []
    for b in range(nv):
        for a in range(nu):
            if shape == 0:
                out.append((a, b))
            else:
                da, db = 2 * a - (nu - 1), 2 * b - (nv - 1)  # (python integers: exact)
                if da * da * nv * nv + db * db * nu * nu <= (nu * nv) ** 2:
                    out.append((a, b))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def layer_positions(origin, u, v, nu, nv, shape=0):
    """(M, 3) float32: one layer's positions in host-index order"""
    pts = layer_points(nu, nv, shape)
    o, u, v = (np.asarray(q, dtype=f32).reshape(3) for q in (origin, u, v))
    a, b = pts[:, 0].astype(f32), pts[:, 1].astype(f32)
    out = np.empty((pts.shape[0], 3), dtype=f32)
    for c in range(3):
        au = (a * u[c]).astype(f32)
        bv = (b * v[c]).astype(f32)
        out[:, c] = ((o[c] + au).astype(f32) + bv).astype(f32)
    return out


class Emitter:
    def __init__(self, origin, u, v, nu, nv, velocity, period=1, first_step=0, max_layers=0, shape=0):
        self.origin, self.u, self.v, self.nu, self.nv, self.shape = origin, u, v, int(nu), int(nv), int(shape)
        self.velocity = np.asarray(velocity, dtype=f32).reshape(3)
        self.period, self.first_step, self.max_layers = int(period), int(first_step), int(max_layers)
        self.layers = 0
        self.points = layer_positions(origin, u, v, nu, nv, shape)

    @property
    def m(self):
        return self.points.shape[0]

    def due(self, s):
        return (s >= self.first_step and (s - self.first_step) % self.period == 0
                and (self.max_layers == 0 or self.layers < self.max_layers))


class Schedule:
    """The step drivers' bookkeeping: at the start of step s the sinks act when every != 0 and s % every == 0 (the caller
    passes what they remove), then the emitters in ascending id; a layer that does not fit is skipped whole, counted, and
    is no layer."""

    def __init__(self, n, capacity, emitters=(), every=8):
        self.n, self.capacity, self.emitters, self.every = int(n), int(capacity), list(emitters), int(every)
        self.emitted = self.skipped = 0

    def looks(self, s):
        return self.every != 0 and s % self.every == 0

    def step(self, s, removed=0):
        """the emitters that emit at step s, in order, after `removed` particles went; updates n and the counters"""
        self.n -= int(removed)
        out = []
        for k, e in enumerate(self.emitters):
            if not e.due(s):
                continue
            if self.n + e.m > self.capacity:
                self.skipped += 1
                continue
            e.layers += 1
            self.n += e.m
            self.emitted += e.m
            out.append(k)
        return out


def sink_goes(sinks, x):
    """sinks: (box_min, box_max, outside) triples; x: (n, 3) float32.  bool (n,)"""
    x = np.asarray(x, dtype=f32).reshape(-1, 3)
    goes = np.zeros(x.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        for lo, hi, outside in sinks:
            lo, hi = np.asarray(lo, dtype=f32), np.asarray(hi, dtype=f32)
            inside = np.ones(x.shape[0], dtype=bool)
            for a in range(3):
                inside &= (x[:, a] >= lo[a]) & (x[:, a] < hi[a])  # (a NaN fails both)
            goes |= inside != bool(outside)
    return goes


def survivors(goes):
    """host indices that stay, ascending; never empty: index 0 stays when every particle would go"""
    goes = np.asarray(goes, dtype=bool)
    keep = np.nonzero(~goes)[0]
    if keep.size == 0:
        keep = np.array([0], dtype=np.int64)
    return keep


def new_index(goes):
    """per old host index: the new one (the number of survivors with a smaller old index), -1 for one that goes"""
    keep = survivors(goes)
    out = np.full(np.asarray(goes).shape[0], -1, dtype=np.int64)
    out[keep] = np.arange(keep.size)
    return out


def compact(goes, arrays):
    """every array (host order, first axis the particles) after the removal"""
    keep = survivors(goes)
    return {k: np.ascontiguousarray(a[keep]) for k, a in arrays.items()}


def append_state(arrays, x, v, force_reset):
    """arrays: a dict of host-order arrays among positions, velocities, forces, densities, pressures, pci_positions,
    pci_velocities; returns it with the new particles (x, v) behind"""
    x = np.asarray(x, dtype=f32).reshape(-1, 3)
    v = np.zeros_like(x) if v is None else np.broadcast_to(np.asarray(v, dtype=f32), x.shape)
    m = x.shape[0]
    new = {"positions": x, "velocities": v, "forces": np.tile(np.asarray(force_reset, dtype=f32).reshape(1, 3), (m, 1)),
           "densities": np.zeros(m, dtype=f32), "pressures": np.zeros(m, dtype=f32), "pci_positions": x, "pci_velocities": v}
    return {k: np.concatenate([a, new[k]]).astype(f32) for k, a in arrays.items()}
