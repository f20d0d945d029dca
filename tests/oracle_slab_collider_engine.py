"""OracleSlabEngine with a triangle-mesh collider (TEST INFRASTRUCTURE): the engine protocol of SlabDriver plus
set_collider / collide, as HipSlabEngine has them.  collide() applies collider_ref.respond to the rows whose position is
finite -- after force_pass those are the particles this rank owns; its ghosts are NaN -- and logs the global ids it moved,
one entry per call."""
import numpy as np

import collider_ref
from oracle_slab_engine import OracleSlabEngine


class OracleSlabColliderEngine(OracleSlabEngine):
    def __init__(self, params, device, cap_full, cap_x):
        super().__init__(params, device, cap_full, cap_x)
        self.mesh = None
        self.hit_log = []  # per collide(): the sorted global ids of the particles the response moved

    def set_option(self, name, value):  # (SlabDriver.dambreak switches the cell index on through this; no index here)
        pass

    def set_collider(self, vertices, normals, radius, restitution):
        self.mesh = (np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(normals, np.float32),
                     np.float32(radius), np.float32(restitution))

    def collide(self):
        verts, normals, radius, rest = self.mesh
        rows = np.isfinite(self.pos).all(axis=1)
        P, V, moved = collider_ref.respond(self.pos[rows], self.vel[rows], verts, normals, self.p.dt, radius, rest)
        self.pos[rows], self.vel[rows] = P, V
        self.hit_log.append(np.sort(self.ids[rows][moved]))
