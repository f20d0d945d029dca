"""SPHEngine: thin object wrapper over the C ABI (include/dslsph.h).

Method names follow model/sph.SPH (model/sph/fluid.go:111-215) and the solver drivers
(solver/wcsph/wcsph.go, solver/pcisph/pcisph_darwin.go) so the parity tests read like
the reference's call sequences.  Every method is one C-ABI call; no arithmetic happens
in Python.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import BodyProps, BodyState, DslError, Emitter, Params, Recorder, Sink, Stats, load_library

BUF = {
    "positions": 0, "velocities": 1, "forces": 2, "densities": 3, "pressures": 4,
    "pci_positions": 5, "pci_velocities": 6,
}
_COMPS = {0: 3, 1: 3, 2: 3, 3: 1, 4: 1, 5: 3, 6: 3}
KERNEL_IDS = {
    "cell_rank": 0, "scan": 1, "scatter": 2, "density": 3, "force_integrate": 4, "pressure": 5, "viscous": 6,
    "gradient": 7, "external": 8, "update": 9, "pci_predict": 10, "pci_density": 11, "tile_list": 12,
    "neigh_lists": 13, "collide": 14, "volume": 15, "surface": 16, "surface_mesh": 17, "sdf": 18,
    "sources": 19,
}
SDF_UNSIGNED = 1  # DSL_SDF_UNSIGNED


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def reference_params(n3: int) -> Params:
    """sph.Init's constants (dsl_params_reference)."""
    L = load_library()
    p = Params()
    rc = L.dsl_params_reference(C.byref(p), int(n3))
    if rc:
        raise DslError(L.dsl_last_error(None).decode())
    return p


class Comm:
    """dsl_comm: the RCCL communicator libdslsph.so owns (include/dslsph.h).  Rank 0 makes the unique id,
    the host hands its 128 bytes to every rank (here: any callable `bcast(bytes_or_None) -> bytes`)."""

    def __init__(self, nranks: int, rank: int, device: int, bcast=None):
        self._L = load_library()
        self.ptr = C.c_void_p()
        self.nranks, self.rank = int(nranks), int(rank)
        ident = (C.c_uint8 * 128)()
        if rank == 0:
            rc = self._L.dsl_comm_unique_id(ident)
            if rc:
                raise DslError(f"dsl_comm_unique_id failed ({rc}): {self._L.dsl_comm_last_error().decode()}")
        if nranks > 1:
            if bcast is None:
                raise DslError("Comm: nranks > 1 needs a broadcast function for the unique id")
            raw = bcast(bytes(ident) if rank == 0 else None)
            ident = (C.c_uint8 * 128).from_buffer_copy(raw)
        rc = self._L.dsl_comm_create(self.nranks, self.rank, ident, int(device), C.byref(self.ptr))
        if rc:
            raise DslError(f"dsl_comm_create failed ({rc}): {self._L.dsl_comm_last_error().decode()}")

    def count(self) -> int:
        """ranks the communicator really spans (ncclCommCount)"""
        n = C.c_int(0)
        rc = self._L.dsl_comm_count(self.ptr, C.byref(n))
        if rc:
            raise DslError(f"dsl_comm_count failed ({rc}): {self._L.dsl_comm_last_error().decode()}")
        return int(n.value)

    def close(self):
        if getattr(self, "ptr", None):
            self._L.dsl_comm_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostStagedComm(Comm):
    """dsl_comm over the host's OWN transport (dsl_comm_create_custom, include/dslsph.h): the library makes
    the same call sequence as it makes to RCCL (group_start / send, recv per neighbour / group_end;
    all_reduce_max for the re-plan words and the PCISPH iteration error), and this table moves the messages
    through host memory with torch.distributed (gloo).  It exists for the places RCCL cannot go -- several
    ranks on ONE device (the 2- and 3-rank GPU tests of the library's step drivers, gloo rehearsals of
    bench.py --gpus N) -- and doubles as the worked example of a host-supplied transport.  Blocking: every
    operation synchronises the stream it is ordered on."""

    def __init__(self, nranks: int, rank: int, device: int, group=None):
        import numpy as np
        import torch
        import torch.distributed as dist
        from ._lib import TR_GROUP, TR_REDUCE, TR_XFER, Transport
        self._L = load_library()
        self.ptr = C.c_void_p()
        self.nranks, self.rank = int(nranks), int(rank)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        hip.hipSetDevice.argtypes = [C.c_int]
        H2D, D2H = 1, 2
        state = {"ops": None, "calls": []}
        self.calls = state["calls"]  # (tests) the sequence of transport calls the library made

        def run(ops):
            hip.hipSetDevice(int(device))
            for st in {o[4] for o in ops}:
                if hip.hipStreamSynchronize(st):
                    return 1
            works, recvs, keep = [], [], []
            for kind, buf, nbytes, peer, _st in ops:
                t = torch.empty(nbytes, dtype=torch.uint8)
                keep.append(t)
                if kind == "send":
                    if hip.hipMemcpy(t.data_ptr(), buf, nbytes, D2H):
                        return 1
                    works.append(dist.P2POp(dist.isend, t, peer, group=group))
                else:
                    works.append(dist.P2POp(dist.irecv, t, peer, group=group))
                    recvs.append((t, buf, nbytes))
            for w in dist.batch_isend_irecv(works):
                w.wait()
            for t, buf, nbytes in recvs:
                if hip.hipMemcpy(buf, t.data_ptr(), nbytes, H2D):
                    return 1
            return 0

        def guarded(fn):
            def call(*a):
                try:
                    return int(fn(*a))
                except Exception as e:  # an exception must not unwind through the C frames
                    import traceback
                    traceback.print_exc()
                    self.error = e
                    return 1
            return call

        def group_start(_ctx):
            state["calls"].append("group_start")
            state["ops"] = []
            return 0

        def group_end(_ctx):
            state["calls"].append("group_end")
            ops, state["ops"] = state["ops"], None
            return run(ops) if ops else 0

        def xfer(kind):
            def f(_ctx, buf, nbytes, peer, stream):
                state["calls"].append((kind, int(peer), int(nbytes)))
                op = (kind, buf, int(nbytes), int(peer), stream)
                if state["ops"] is None:
                    return run([op])
                state["ops"].append(op)
                return 0
            return f

        def all_reduce(_ctx, buf, count, stream):
            state["calls"].append(("all_reduce_max", int(count)))
            hip.hipSetDevice(int(device))
            if hip.hipStreamSynchronize(stream):
                return 1
            a = np.zeros(int(count), dtype=np.uint32)
            if hip.hipMemcpy(a.ctypes.data, buf, a.nbytes, D2H):
                return 1
            t = torch.from_numpy(a.astype(np.int64))
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
            a = t.numpy().astype(np.uint32)
            return 1 if hip.hipMemcpy(buf, a.ctypes.data, a.nbytes, H2D) else 0

        # (the CFUNCTYPE objects must outlive the communicator: the library keeps the raw pointers)
        self._cb = (TR_GROUP(guarded(group_start)), TR_GROUP(guarded(group_end)), TR_XFER(guarded(xfer("send"))),
                    TR_XFER(guarded(xfer("recv"))), TR_REDUCE(guarded(all_reduce)))
        self._table = Transport(None, *self._cb)
        rc = self._L.dsl_comm_create_custom(self.nranks, self.rank, int(device), C.cast(C.byref(self._table), C.c_void_p),
                                            C.byref(self.ptr))
        if rc:
            raise DslError(f"dsl_comm_create_custom failed ({rc}): {self._L.dsl_comm_last_error().decode()}")


class SPHEngine:
    def __init__(self, params: Params, device: int = 0):
        self._L = load_library()
        self._h = C.c_void_p()
        rc = self._L.dsl_create(C.byref(params), int(device), C.byref(self._h))
        if rc:
            raise DslError(f"dsl_create failed ({rc}): {self._L.dsl_last_error(None).decode()}")
        self.device = device
        self.capacity = int(params.capacity) if params.capacity else int(params.n_particles)

    # -- plumbing -----------------------------------------------------------------
    def _ck(self, rc):
        if rc:
            raise DslError(f"libdslsph error {rc}: {self._L.dsl_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self._L.dsl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def n(self) -> int:
        """live particle count: changes in slab mode, and with append_particles, emitters and sinks"""
        n = C.c_int(0)
        self._ck(self._L.dsl_get_count(self._h, C.byref(n), None))
        return n.value

    def n_owned(self) -> int:
        n, o = C.c_int(0), C.c_int(0)
        self._ck(self._L.dsl_get_count(self._h, C.byref(n), C.byref(o)))
        return o.value

    @property
    def params(self) -> Params:
        p = Params()
        self._ck(self._L.dsl_get_params(self._h, C.byref(p)))
        return p

    def set_params(self, p: Params):
        self._ck(self._L.dsl_set_params(self._h, C.byref(p)))

    def set_stream(self, stream_ptr):
        """run on the given hipStream_t (0 / None = HIP's default stream)"""
        self._ck(self._L.dsl_set_stream(self._h, C.c_void_p(stream_ptr or None)))

    def use_own_stream(self):
        self._ck(self._L.dsl_use_own_stream(self._h))

    # -- buffers (ComputeGPU.PassFloatBuffer / ReadFloatBuffer) -------------------
    def upload(self, name: str, arr):
        b = BUF[name]
        a = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1)
        self._ck(self._L.dsl_upload(self._h, b, _fp(a), a.size))

    @property
    def n_fluid(self) -> int:
        """N(): particles that are not boundary particles (slab mode: the live count)"""
        nb = int(self.params.n_boundary)
        return self.n - nb if nb > 0 else self.n

    def add_boundary_particles(self, positions):
        """ParticleArray.AddBoundaryParticles (model/particle_array.go:123-128)"""
        a = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
        self._ck(self._L.dsl_add_boundary_particles(self._h, _fp(a), a.size))

    def download(self, name: str, sorted_order: bool = False) -> np.ndarray:
        b = BUF[name]
        n = self.n if name == "positions" else self.n_fluid
        out = np.empty(n * _COMPS[b], dtype=np.float32)
        fn = self._L.dsl_download_sorted if sorted_order else self._L.dsl_download
        self._ck(fn(self._h, b, _fp(out), out.size))
        return out.reshape(n, 3) if _COMPS[b] == 3 else out

    def download_decimated(self, name: str, stride: int) -> np.ndarray:
        """every stride-th particle of positions/velocities (render hand-off)"""
        n = self.n
        out = np.empty(3 * ((n + stride - 1) // stride), dtype=np.float32)
        self._ck(self._L.dsl_download_decimated(self._h, BUF[name], int(stride), _fp(out), out.size))
        return out.reshape(-1, 3)

    def device_pointers(self, name: str):
        """(x_ptr, y_ptr, z_ptr), ids_ptr, n of the live SoA device arrays (slot order)"""
        xyz = (C.c_void_p * 3)()
        ids = C.c_void_p()
        n = C.c_int(0)
        self._ck(self._L.dsl_device_pointers(self._h, BUF[name], xyz, C.byref(ids), C.byref(n)))
        return (xyz[0], xyz[1], xyz[2]), ids.value, n.value

    def set_ids(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        self._ck(self._L.dsl_set_ids(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size))

    def reset_forces(self):
        self._ck(self._L.dsl_reset_forces(self._h))

    # -- multi-GPU slabs (device record buffers are raw pointers, e.g. tensor.data_ptr()) --
    def slab_config(self, axis: int, lo: float, hi: float):
        self._ck(self._L.dsl_slab_config(self._h, int(axis), C.c_float(lo), C.c_float(hi)))

    def slab_message_floats(self, cap_full: int, cap_xonly: int) -> int:
        return int(self._L.dsl_slab_message_floats_for(self._h, int(cap_full), int(cap_xonly)))

    def slab_record_floats(self) -> int:
        return int(self._L.dsl_slab_record_floats(self._h))

    def pcisph_phase(self, phase: int):
        """0 begin step, 1 iterate, 2 check, 3 end step (include/dslsph.h)"""
        self._ck(self._L.dsl_pcisph_phase(self._h, int(phase)))

    def pcisph_set_binning(self, mode: int):
        """-1 never, 0 automatic, 1 always: sort DensityF's query points into grid cells of their own (include/dslsph.h)"""
        self._ck(self._L.dsl_pcisph_set_binning(self._h, int(mode)))

    def pcisph_binning(self):
        """(mode, active): active = the next correction iteration sorts its queries"""
        m, a = C.c_int(0), C.c_int(0)
        self._ck(self._L.dsl_pcisph_get_binning(self._h, C.byref(m), C.byref(a), None))
        return m.value, bool(a.value)

    def pcisph_query_escaped(self) -> bool:
        """slab mode: has a DensityF query point left what the ghost band covers (include/dslsph.h)?  Blocking."""
        e = C.c_int(0)
        self._ck(self._L.dsl_pcisph_get_binning(self._h, None, None, C.byref(e)))
        return bool(e.value)

    def pcisph_error_word(self, dev_word: int, store: bool):
        self._ck(self._L.dsl_pcisph_error_word(self._h, C.c_void_p(dev_word), 1 if store else 0))

    def slab_split(self, width: float, margin: float):
        self._ck(self._L.dsl_slab_split(self._h, C.c_float(width), C.c_float(margin)))

    def slab_pack(self, width_full: float, width: float, dev_lo: int, dev_hi: int, cap_full: int, cap_xonly: int):
        self._ck(self._L.dsl_slab_pack(self._h, C.c_float(width_full), C.c_float(width), C.c_void_p(dev_lo or None),
                                       C.c_void_p(dev_hi or None), int(cap_full), int(cap_xonly)))

    def slab_pack_band(self, width_full: float, dev_lo: int, dev_hi: int, cap_full: int, cap_xonly: int,
                       stream: int = 0):
        """between force_pass_split(BAND) and (INNER): packs the integrated band on `stream`"""
        self._ck(self._L.dsl_slab_pack_band(self._h, C.c_float(width_full), C.c_void_p(dev_lo or None),
                                            C.c_void_p(dev_hi or None), int(cap_full), int(cap_xonly),
                                            C.c_void_p(stream or None)))

    def force_pass_split(self, phase: int):
        self._ck(self._L.dsl_force_pass_split(self._h, int(phase)))

    def slab_append(self, dev_msg: int, cap_full: int, cap_xonly: int):
        self._ck(self._L.dsl_slab_append(self._h, C.c_void_p(dev_msg), int(cap_full), int(cap_xonly)))

    def slab_append2(self, dev_msg_a: int, dev_msg_b: int, cap_full: int, cap_xonly: int):
        self._ck(self._L.dsl_slab_append2(self._h, C.c_void_p(dev_msg_a or None), C.c_void_p(dev_msg_b or None),
                                          int(cap_full), int(cap_xonly)))

    def slab_status(self, reset_high_water: bool = False):
        """(overflow, band_missed, high-water full, high-water position-only); blocking"""
        st = (C.c_int32 * 4)()
        self._ck(self._L.dsl_slab_status(self._h, st, 1 if reset_high_water else 0))
        return tuple(int(v) for v in st)

    def slab_overflow(self) -> int:
        v = C.c_int(0)
        self._ck(self._L.dsl_slab_overflow(self._h, C.byref(v)))
        return v.value

    # -- the exchange behind the C ABI (RCCL inside libdslsph.so) ---------------------------------
    def slab_attach(self, comm, lo_rank: int, hi_rank: int, width_full: float, width: float, cap_full: int,
                    cap_xonly: int, overlap: bool):
        """comm: a Comm (or None for a lone slab); neighbour ranks, -1 at a domain end"""
        self._comm = comm  # keep it alive as long as the link
        self._ck(self._L.dsl_slab_attach(self._h, comm.ptr if comm is not None else None, int(lo_rank), int(hi_rank),
                                         C.c_float(width_full), C.c_float(width), int(cap_full), int(cap_xonly),
                                         1 if overlap else 0))

    def slab_detach(self):
        self._ck(self._L.dsl_slab_detach(self._h))

    def slab_image_shift(self, from_lo: float, from_hi: float):
        self._ck(self._L.dsl_slab_image_shift(self._h, C.c_float(from_lo), C.c_float(from_hi)))

    def slab_exchange(self):
        self._ck(self._L.dsl_slab_exchange(self._h))

    def slab_replan(self):
        self._ck(self._L.dsl_slab_replan(self._h))

    def slab_wcsph_step(self, nsteps: int = 1):
        self._ck(self._L.dsl_slab_wcsph_step(self._h, int(nsteps)))

    def slab_pcisph_step(self, nsteps: int = 1):
        self._ck(self._L.dsl_slab_pcisph_step(self._h, int(nsteps)))

    # -- re-balancing: the slab planes move during a run (include/dslsph.h) -----------------------
    def slab_layer_counts(self, origin: float, n_layers: int, dev_counts: int):
        """owned particles per cell layer from `origin` into n_layers int32 words of device memory; asynchronous"""
        self._ck(self._L.dsl_slab_layer_counts(self._h, C.c_float(origin), int(n_layers), C.c_void_p(dev_counts or None)))

    def slab_move_planes(self, lo: float, hi: float):
        """new [lo, hi) without touching the particles: only between an integrate and the next pack"""
        self._ck(self._L.dsl_slab_move_planes(self._h, C.c_float(lo), C.c_float(hi)))

    def slab_get_planes(self):
        lo, hi = C.c_float(0), C.c_float(0)
        self._ck(self._L.dsl_slab_get_planes(self._h, C.byref(lo), C.byref(hi)))
        return float(lo.value), float(hi.value)

    def slab_rebalance(self, every: int, origin: float = 0.0, n_layers: int = 0, planes=None, plane_min=None,
                       plane_max=None, min_layers: int = 2):
        """the native drivers look every `every` steps and move the planes (0: off); planes and bounds in layers"""
        arr = [None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in (planes, plane_min, plane_max)]
        ptr = [None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32)) for a in arr]
        self._ck(self._L.dsl_slab_rebalance(self._h, int(every), C.c_float(origin), int(n_layers), ptr[0], ptr[1], ptr[2],
                                            int(min_layers)))
        if every:
            self._balance_shape = (arr[0].size, int(n_layers))  # what slab_rebalance_state has to make room for

    def slab_rebalance_state(self):
        """(planes of the last plan, last global histogram, looks, moves planned); blocking"""
        n_planes, n_layers = getattr(self, "_balance_shape", (0, 0))
        planes, counts = np.zeros(n_planes, dtype=np.int32), np.zeros(n_layers, dtype=np.int32)
        looks, moves = C.c_int64(0), C.c_int64(0)
        self._ck(self._L.dsl_slab_rebalance_state(self._h, planes.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  counts.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(looks), C.byref(moves)))
        return planes, counts, int(looks.value), int(moves.value)

    def download_ids(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.int32)
        self._ck(self._L.dsl_download_ids(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size))
        return out

    def download_cell_start(self) -> np.ndarray:
        cells = self.stats().grid_cells
        out = np.empty(cells + 1, dtype=np.int32)
        self._ck(self._L.dsl_download_cell_start(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size))
        return out

    # -- lsh_ref parity mode (sampler/lsh/lsh.go) ---------------------------------------
    def set_hash_vectors(self, vectors):
        v = np.ascontiguousarray(vectors, dtype=np.float32).reshape(-1, 3)
        self._ck(self._L.dsl_set_hash_vectors(self._h, _fp(v), v.shape[0]))

    def lsh_table(self) -> np.ndarray:
        p = self.params
        out = np.empty(p.lsh_buckets * p.lsh_bucket_size, dtype=np.int32)
        self._ck(self._L.dsl_lsh_download_table(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size))
        return out

    # -- model/sph.SPH passes -----------------------------------------------------
    def nn(self):
        self._ck(self._L.dsl_build_neighbours(self._h))

    def density_all(self):
        self._ck(self._L.dsl_density_pass(self._h))

    def pressure_all(self):
        self._ck(self._L.dsl_pressure_pass(self._h))

    def viscous_all(self):
        self._ck(self._L.dsl_viscous_pass(self._h))

    def external_all(self, f):
        a = np.ascontiguousarray(f, dtype=np.float32)
        self._ck(self._L.dsl_external_pass(self._h, _fp(a)))

    def gradient_pressure_force(self):
        self._ck(self._L.dsl_gradient_pressure_pass(self._h))

    def update(self):
        self._ck(self._L.dsl_update_pass(self._h))

    def force_pass(self):
        self._ck(self._L.dsl_force_pass(self._h))

    # -- geom.Collider: Mesh.Collision (geom/mesh/mesh.go:41-57) -------------------
    def set_collider_mesh(self, vertices=None, normals=None, radius: float = 0.0, restitution: float = 0.0):
        """T triangles in list order: vertices (T, 3, 3), normals (T, 3), used as supplied.  Several meshes: concatenate
        them.  None or an empty array removes the mesh."""
        v = np.ascontiguousarray(vertices if vertices is not None else [], dtype=np.float32).reshape(-1)
        nrm = np.ascontiguousarray(normals if normals is not None else [], dtype=np.float32).reshape(-1)
        if v.size % 9 or nrm.size * 3 != v.size:
            raise DslError("set_collider_mesh: 9 vertex floats and 3 normal floats per triangle")
        self._ck(self._L.dsl_collider_set_mesh(self._h, _fp(v), _fp(nrm), v.size // 9, C.c_float(radius),
                                               C.c_float(restitution)))

    def collide(self):
        """query + response for every fluid particle (the step drivers run it themselves while a mesh is set)"""
        self._ck(self._L.dsl_collide_pass(self._h))

    def collider_query(self):
        """Mesh.Collision for every fluid particle, no response: (tri, normal, coord, point) in host order"""
        n = self.n_fluid
        tri = np.empty(n, dtype=np.int32)
        nrm, coord, point = (np.empty((n, 3), dtype=np.float32) for _ in range(3))
        self._ck(self._L.dsl_collider_query(self._h, tri.ctypes.data_as(C.POINTER(C.c_int32)), _fp(nrm), _fp(coord),
                                            _fp(point)))
        return tri, nrm, coord, point

    # -- implicit colliders (include/dslsph.h: dsl_mesh_distance_volume, dsl_collider_set_volume) --
    def mesh_distance_volume(self, vertices, origin, step, dims, band: float = float("inf"), unsigned: bool = False, dev_out=None):
        """The signed (or unsigned) distance of every lattice point origin + step * (i, j, k) to the triangles `vertices`
        (T, 3, 3), cut off at `band`: an ndarray of shape (nz, ny, nx), or None with `dev_out` -- a device pointer to
        nx * ny * nz floats, written on the engine's stream.  Negative inside (the +x ray crosses an odd number of triangles)."""
        v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1)
        if v.size % 9:
            raise DslError("mesh_distance_volume: 9 vertex floats per triangle")
        o, s, d = self._lattice(origin, step, dims)
        ip = d.ctypes.data_as(C.POINTER(C.c_int32))
        flags = SDF_UNSIGNED if unsigned else 0
        if dev_out is not None:
            self._ck(self._L.dsl_mesh_distance_volume(self._h, _fp(v), v.size // 9, _fp(o), _fp(s), ip, C.c_float(band), flags,
                                                      C.c_void_p(dev_out), None))
            return None
        n = int(d[0]) * int(d[1]) * int(d[2])
        out = np.empty(n if d.min() >= 1 and n <= 1 << 30 else 1, dtype=np.float32)  # (dims the library refuses: _ck raises)
        self._ck(self._L.dsl_mesh_distance_volume(self._h, _fp(v), v.size // 9, _fp(o), _fp(s), ip, C.c_float(band), flags, None,
                                                  _fp(out)))
        return out.reshape(int(d[2]), int(d[1]), int(d[0]))

    def set_collider_volume(self, volume=None, origin=None, step=None, dims=None, radius: float = 0.0, restitution: float = 0.0,
                            unsigned: bool = False, dev_volume=None):
        """A distance volume as the step's collider: `volume` an array of shape (nz, ny, nx), or `dev_volume` a device pointer
        with `dims` = (nx, ny, nz); the library keeps a copy.  Neither (or dims None without an array) removes the collider."""
        flags = SDF_UNSIGNED if unsigned else 0
        if volume is None and dev_volume is None:
            self._ck(self._L.dsl_collider_set_volume(self._h, None, None, None, None, None, C.c_float(0), C.c_float(0), 0))
            return
        if volume is not None:
            vol = np.ascontiguousarray(volume, dtype=np.float32)
            if vol.ndim != 3:
                raise DslError("set_collider_volume: volume has the shape (nz, ny, nx)")
            dims = vol.shape[::-1]
        o, s, d = self._lattice(origin, step, dims)
        ip = d.ctypes.data_as(C.POINTER(C.c_int32))
        self._ck(self._L.dsl_collider_set_volume(self._h, C.c_void_p(dev_volume) if volume is None else None,
                                                 _fp(vol) if volume is not None else None, _fp(o), _fp(s), ip,
                                                 C.c_float(radius), C.c_float(restitution), flags))

    def collider_volume_query(self):
        """the interpolated distance and the unit gradient of the volume collider at every fluid particle, host order, no response"""
        n = self.n_fluid
        dist = np.empty(n, dtype=np.float32)
        nrm = np.empty((n, 3), dtype=np.float32)
        self._ck(self._L.dsl_collider_volume_query(self._h, _fp(dist), _fp(nrm)))
        return dist, nrm

    def set_collider_volume_motion(self, rot=None, trans=None, lin_vel=None, ang_vel=None):
        """The volume collider as a rigid body in motion (dsl_collider_volume_motion): `rot` (3, 3) row-major, its columns the
        body's axes in world coordinates; `trans` the body frame's origin; `lin_vel` the body's velocity there and `ang_vel` its
        angular velocity, world.  None is the identity / zero; all four None turn motion off.  The voxels are not touched; the
        pose holds until the next call (the library does not integrate it)."""
        def arr(a, n, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
            if a.size != n:
                raise DslError(f"set_collider_volume_motion: {what} takes {n} values")
            return a
        r, t, lv, av = arr(rot, 9, "rot"), arr(trans, 3, "trans"), arr(lin_vel, 3, "lin_vel"), arr(ang_vel, 3, "ang_vel")
        ptr = lambda a: _fp(a) if a is not None else None
        self._ck(self._L.dsl_collider_volume_motion(self._h, ptr(r), ptr(t), ptr(lv), ptr(av)))

    def clear_collider_volume_motion(self):
        """motion off: the static pass runs again (the accumulated impulse stays until it is read and reset)"""
        self._ck(self._L.dsl_collider_volume_motion(self._h, None, None, None, None))

    def collider_volume_impulse(self, reset: bool = False):
        """(impulse (3,), torque impulse about `trans` (3,)): what the fluid handed to the moving body since the last reset"""
        imp = np.zeros(3, dtype=np.float32)
        trq = np.zeros(3, dtype=np.float32)
        self._ck(self._L.dsl_collider_volume_impulse(self._h, _fp(imp), _fp(trq), 1 if reset else 0))
        return imp, trq

    # -- rigid bodies (include/dslsph.h: dsl_body_add) ------------------------------
    @staticmethod
    def _body_props(inv_mass=0.0, inv_inertia=(0.0, 0.0, 0.0), accel=(0.0, 0.0, 0.0), radius=0.0, restitution=0.0):
        return BodyProps(inv_mass, (C.c_float * 3)(*inv_inertia), (C.c_float * 3)(*accel), radius, restitution)

    @staticmethod
    def _body_state(quat=(1.0, 0.0, 0.0, 0.0), trans=(0.0, 0.0, 0.0), lin_vel=(0.0, 0.0, 0.0), ang_vel=(0.0, 0.0, 0.0)):
        return BodyState((C.c_float * 4)(*quat), (C.c_float * 3)(*trans), (C.c_float * 3)(*lin_vel), (C.c_float * 3)(*ang_vel))

    def add_body(self, volume, origin, step, props: dict, state: dict | None = None, dims=None, dev_volume=None) -> int:
        """A rigid body from a distance volume (`volume` of shape (nz, ny, nx), or `dev_volume` a device pointer with `dims`);
        `props`: inv_mass, inv_inertia, accel, radius, restitution; `state`: quat (w, x, y, z), trans, lin_vel, ang_vel, None
        being the identity at rest.  Returns the body's id: 0, 1, ... in the order of the calls."""
        vol = None
        if volume is not None:
            vol = np.ascontiguousarray(volume, dtype=np.float32)
            if vol.ndim != 3:
                raise DslError("add_body: volume has the shape (nz, ny, nx)")
            dims = vol.shape[::-1]
        o, s, d = self._lattice(origin, step, dims)
        pr = self._body_props(**props)
        st = self._body_state(**state) if state is not None else None
        bid = C.c_int(-1)
        self._ck(self._L.dsl_body_add(self._h, C.c_void_p(dev_volume) if vol is None else None, _fp(vol) if vol is not None else None,
                                      _fp(o), _fp(s), d.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(pr),
                                      C.byref(st) if st is not None else None, C.byref(bid)))
        return int(bid.value)

    def clear_bodies(self):
        self._ck(self._L.dsl_bodies_clear(self._h))

    def set_body_state(self, body: int, **state):
        """quat, trans, lin_vel, ang_vel of one body (what is left out: the identity / zero); holds from the next pass on"""
        st = self._body_state(**state)
        self._ck(self._L.dsl_body_set_state(self._h, body, C.byref(st)))

    def set_body_props(self, body: int, **props):
        pr = self._body_props(**props)
        self._ck(self._L.dsl_body_set_props(self._h, body, C.byref(pr)))

    def body_state(self, body: int, reset: bool = False):
        """(state: dict of float32 arrays quat, trans, lin_vel, ang_vel; impulse (3,); torque impulse about trans (3,)) of one
        body; `reset` zeroes its accumulators after the read"""
        st = BodyState()
        imp = np.zeros(3, dtype=np.float32)
        trq = np.zeros(3, dtype=np.float32)
        self._ck(self._L.dsl_body_get_state(self._h, body, C.byref(st), _fp(imp), _fp(trq), 1 if reset else 0))
        state = {k: np.array(getattr(st, k)[:], dtype=np.float32) for k in ("quat", "trans", "lin_vel", "ang_vel")}
        return state, imp, trq

    def body_query(self, body: int):
        """the interpolated distance and the world-space unit gradient of one body at every fluid particle, host order, no response"""
        n = self.n_fluid
        dist = np.empty(n, dtype=np.float32)
        nrm = np.empty((n, 3), dtype=np.float32)
        self._ck(self._L.dsl_body_query(self._h, body, _fp(dist), _fp(nrm)))
        return dist, nrm

    # -- the bodies' contact stage (include/dslsph.h: dsl_contact_points) -----------
    def contact_points(self, body: int, cap: int | None = None):
        """(the first min(M, cap) voxel indices of a body's contact points, ascending; M).  cap None: all of them"""
        m = C.c_int64(0)
        if cap is None:
            self._ck(self._L.dsl_contact_points(self._h, body, None, 0, C.byref(m)))
            cap = int(m.value)
        out = np.zeros(max(cap, 1), dtype=np.int32)
        self._ck(self._L.dsl_contact_points(self._h, body, out.ctypes.data_as(C.POINTER(C.c_int32)) if cap > 0 else None, cap,
                                            C.byref(m)))
        return out[:min(cap, int(m.value))], int(m.value)

    def contact_pass(self, kinds: int = 3, solve: bool = False):
        """detection at the current poses (kinds: 1 walls | 2 bodies), and the solve behind it if asked; asynchronous"""
        self._ck(self._L.dsl_contact_pass(self._h, int(kinds), 1 if solve else 0))

    def contact_table(self) -> np.ndarray:
        """E of the last detection, (K, 6 + K, 9): S (3), N (3), W, C, D per body and target"""
        k = int(self.get_option("bodies"))
        out = np.zeros((k, 6 + k, 9), dtype=np.float32)
        self._ck(self._L.dsl_contact_table(self._h, _fp(out), out.size))
        return out

    # -- sources and sinks (include/dslsph.h: dsl_particles_append .. dsl_particles_remove) ---
    def append_particles(self, positions, velocities=None):
        """new fluid particles behind the current ones (host indices n .. n + len - 1); velocities None: zeros"""
        p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1)
        v = None if velocities is None else np.ascontiguousarray(velocities, dtype=np.float32).reshape(-1)
        if v is not None and v.size != p.size:
            raise ValueError("positions and velocities must have the same shape")
        self._ck(self._L.dsl_particles_append(self._h, _fp(p) if p.size else None, None if v is None else _fp(v), p.size // 3))

    def add_emitter(self, origin, u, v, nu: int, nv: int, velocity, period: int = 1, first_step: int = 0, max_layers: int = 0,
                    shape: int = 0) -> int:
        """a face of nu x nv lattice points origin + a u + b v (shape 1: the inscribed ellipse) that emits a layer every
        period-th step from first_step on, max_layers of them (0: no limit); returns the emitter's id"""
        e = Emitter((C.c_float * 3)(*origin), (C.c_float * 3)(*u), (C.c_float * 3)(*v), int(nu), int(nv), int(shape),
                    (C.c_float * 3)(*velocity), int(period), int(first_step), int(max_layers))
        k = C.c_int(-1)
        self._ck(self._L.dsl_emitter_add(self._h, C.byref(e), C.byref(k)))
        return k.value

    def clear_emitters(self):
        self._ck(self._L.dsl_emitters_clear(self._h))

    def emit(self, emitter: int):
        """one layer of the emitter now, between steps"""
        self._ck(self._L.dsl_emit(self._h, int(emitter)))

    def add_sink(self, box_min, box_max, outside: bool = False) -> int:
        """particles inside the box [box_min, box_max) go (outside: the ones outside it); entries may be +-inf"""
        s = Sink((C.c_float * 3)(*box_min), (C.c_float * 3)(*box_max), 1 if outside else 0)
        k = C.c_int(-1)
        self._ck(self._L.dsl_sink_add(self._h, C.byref(s), C.byref(k)))
        return k.value

    def clear_sinks(self):
        self._ck(self._L.dsl_sinks_clear(self._h))

    def remove_particles(self) -> int:
        """applies the sinks now; returns how many particles went"""
        r = C.c_int64(0)
        self._ck(self._L.dsl_particles_remove(self._h, C.byref(r)))
        return int(r.value)

    # -- the frame recorder (include/dslsph.h: dsl_recorder_set .. dsl_record_read; animation.py decodes and files the frames) ---
    REC_FIELDS = {"velocities": 1, "densities": 2}
    REC_ENCODINGS = {"f32": 0, "q16": 1}

    @staticmethod
    def recorder_spec(every: int = 1, stride: int = 1, fields=(), encoding="f32", slots: int = 4, box=None, first_step: int = 0,
                      max_frames: int = 0) -> Recorder:
        """a dsl_recorder: fields an iterable of "velocities" / "densities" (or the bit mask), encoding "f32" / "q16" (or the
        number), box None: each Q16 frame's own bounds (auto_box), else (box_min, box_max)"""
        bits = fields if isinstance(fields, int) else sum(SPHEngine.REC_FIELDS[f] for f in fields)
        enc = encoding if isinstance(encoding, int) else SPHEngine.REC_ENCODINGS[encoding]
        lo, hi = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) if box is None else box
        return Recorder(int(every), int(stride), int(bits), int(enc), int(slots), 1 if (box is None and enc == 1) else 0, (C.c_float * 3)(*lo),
                        (C.c_float * 3)(*hi), int(first_step), int(max_frames))

    def set_recorder(self, spec=None, **kw):
        """a frame every `every`-th step from first_step on (recorder_spec's arguments, or a Recorder); set_recorder(None)
        with no arguments turns it off and frees everything"""
        if spec is None and not kw:
            self._ck(self._L.dsl_recorder_set(self._h, None))
            return None
        spec = spec if spec is not None else self.recorder_spec(**kw)
        self._ck(self._L.dsl_recorder_set(self._h, C.byref(spec)))
        return spec

    def record_frame_bytes(self, spec: Recorder, n: int) -> int:
        return int(self._L.dsl_record_frame_bytes(C.byref(spec), int(n)))

    def record_now(self):
        """one frame of the current state, between steps"""
        self._ck(self._L.dsl_record_now(self._h))

    def record_poll(self):
        """(recorded, ready, dropped); never blocks"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ck(self._L.dsl_record_poll(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def peek_frame(self) -> np.ndarray:
        """the oldest unreleased frame as a uint8 view of its pinned slot: valid until release_frame"""
        ptr, size = C.c_void_p(), C.c_size_t(0)
        self._ck(self._L.dsl_record_peek(self._h, C.byref(ptr), C.byref(size)))
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(size.value,))

    def release_frame(self):
        self._ck(self._L.dsl_record_release(self._h))

    def read_frame(self) -> bytes:
        """the oldest unreleased frame, copied out and released (animation.decode_frame reads it)"""
        out = bytes(self.peek_frame())
        self.release_frame()
        return out

    # -- SPHField operators no solver calls (sph_field.go:124-135,203-294) ---------
    def field_div(self, tensor: str = "velocities") -> np.ndarray:
        out = np.empty(self.n_fluid, dtype=np.float32)
        self._ck(self._L.dsl_field_divergence(self._h, BUF[tensor], _fp(out), out.size))
        return out

    def field_curl(self, tensor: str = "velocities") -> np.ndarray:
        out = np.empty(self.n_fluid * 3, dtype=np.float32)
        self._ck(self._L.dsl_field_curl(self._h, BUF[tensor], _fp(out), out.size))
        return out.reshape(-1, 3)

    def field_laplacian(self, scalar: str = "densities") -> np.ndarray:
        out = np.empty(self.n_fluid, dtype=np.float32)
        self._ck(self._L.dsl_field_laplacian(self._h, BUF[scalar], _fp(out), out.size))
        return out

    def field_interpolate(self, positions, scalar: str = "densities") -> np.ndarray:
        q = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        out = np.empty(q.shape[0], dtype=np.float32)
        self._ck(self._L.dsl_field_interpolate(self._h, BUF[scalar], _fp(q), q.shape[0], _fp(out)))
        return out

    def field_volume(self, origin, step, dims, scalar: str = "densities", dev_out=None):
        """field_interpolate at every point of the lattice origin + step * (i, j, k) (scenes.volume_points), evaluated on the
        device: an ndarray of shape (nz, ny, nx), or None with `dev_out` -- a device pointer to nx * ny * nz floats, written
        asynchronously on the engine's stream.  `step` is one number or three."""
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, dtype=np.float32), (3,)))
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(step, dtype=np.float32), (3,)))
        d = np.ascontiguousarray(dims, dtype=np.int32).reshape(3)
        ip = d.ctypes.data_as(C.POINTER(C.c_int32))
        if dev_out is not None:
            self._ck(self._L.dsl_field_volume(self._h, BUF[scalar], _fp(o), _fp(s), ip, C.c_void_p(dev_out), None))
            return None
        n = int(d[0]) * int(d[1]) * int(d[2])
        out = np.empty(n if d.min() >= 1 and n <= 1 << 30 else 1, dtype=np.float32)  # (dims the library refuses: _ck raises)
        self._ck(self._L.dsl_field_volume(self._h, BUF[scalar], _fp(o), _fp(s), ip, None, _fp(out)))
        return out.reshape(int(d[2]), int(d[1]), int(d[0]))

    @staticmethod
    def _lattice(origin, step, dims):
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, dtype=np.float32), (3,)))
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(step, dtype=np.float32), (3,)))
        d = np.ascontiguousarray(dims, dtype=np.int32).reshape(3)
        return o, s, d

    def surface_extract(self, dev_volume, origin, step, dims, iso, dev_vertices=None, dev_normals=None, cap: int = 0,
                        dev_count=None, want_count: bool = True):
        """The iso-surface triangles of a device volume on field_volume's lattice (include/dslsph.h: dsl_surface_extract).
        Every dev_* argument is a device pointer (an int) or None: the first min(T, cap) triangles go to dev_vertices (9 floats
        each) and dev_normals (3 each), the full number T to the int64 at dev_count.  Returns T (a blocking 8-byte copy), or
        None with want_count = False: the call is then asynchronous on the engine's stream."""
        o, s, d = self._lattice(origin, step, dims)
        n = C.c_int64(-1)
        self._ck(self._L.dsl_surface_extract(self._h, C.c_void_p(dev_volume), _fp(o), _fp(s), d.ctypes.data_as(C.POINTER(C.c_int32)),
                                             C.c_float(iso), C.c_void_p(dev_vertices), C.c_void_p(dev_normals), int(cap),
                                             C.c_void_p(dev_count), C.byref(n) if want_count else None))
        return int(n.value) if want_count else None

    def field_surface(self, origin, step, dims, iso, scalar: str = "densities", guess: int = 0):
        """field_volume and the iso-surface of it in one call: (T, 3, 3) vertices and (T, 3) normals, in mesh.Mesh order.  The
        host buffer is sized from a guess -- `guess` triangles, or four per voxel of the lattice's three faces (a surface
        grows with the lattice's area, not its volume) -- and the library is called again only when the guess was short."""
        o, s, d = self._lattice(origin, step, dims)
        ip = d.ctypes.data_as(C.POINTER(C.c_int32))
        if guess <= 0:
            nx, ny, nz = (max(int(v), 1) for v in d)
            guess = max(1024, 4 * (nx * ny + ny * nz + nz * nx))
        n = C.c_int64(0)
        for _ in range(2):
            cap = int(guess)
            verts = np.empty((cap, 3, 3), dtype=np.float32)
            norms = np.empty((cap, 3), dtype=np.float32)
            self._ck(self._L.dsl_field_surface(self._h, BUF[scalar], _fp(o), _fp(s), ip, C.c_float(iso), _fp(verts), _fp(norms), cap,
                                               C.byref(n)))
            if n.value <= cap:
                break
            guess = n.value
        return verts[:n.value].copy(), norms[:n.value].copy()

    def surface_extract_indexed(self, dev_volume, origin, step, dims, iso, dev_positions=None, dev_normals=None, cap_vertices: int = 0,
                                dev_indices=None, cap_triangles: int = 0, dev_counts=None, want_counts: bool = True):
        """The same surface as an indexed mesh (include/dslsph.h: dsl_surface_extract_indexed): every vertex once, a normal per
        vertex, three int32 vertex ids per triangle.  Every dev_* argument is a device pointer (an int) or None: the first
        min(V, cap_vertices) vertices go to dev_positions and dev_normals (3 floats each), the first min(T, cap_triangles)
        triples to dev_indices, (V, T) to the two int64 at dev_counts.  Returns (V, T) (a blocking copy), or None with
        want_counts = False: the call is then asynchronous on the engine's stream.  The mesh is complete only when both
        capacities suffice."""
        o, s, d = self._lattice(origin, step, dims)
        n = (C.c_int64 * 2)(-1, -1)
        self._ck(self._L.dsl_surface_extract_indexed(self._h, C.c_void_p(dev_volume), _fp(o), _fp(s), d.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     C.c_float(iso), C.c_void_p(dev_positions), C.c_void_p(dev_normals),
                                                     int(cap_vertices), C.c_void_p(dev_indices), int(cap_triangles),
                                                     C.c_void_p(dev_counts), n if want_counts else None))
        return (int(n[0]), int(n[1])) if want_counts else None

    def field_surface_indexed(self, origin, step, dims, iso, scalar: str = "densities", guess=(0, 0)):
        """field_volume and the indexed mesh of it in one call: (V, 3) positions, (V, 3) normals and (T, 3) int32 indices.  The
        host buffers are sized from a guess -- `guess` = (vertices, triangles), or two vertices and four triangles per voxel
        of the lattice's three faces -- and the library is called again only when a guess was short."""
        o, s, d = self._lattice(origin, step, dims)
        ip = d.ctypes.data_as(C.POINTER(C.c_int32))
        nx, ny, nz = (max(int(v), 1) for v in d)
        area = nx * ny + ny * nz + nz * nx
        cap_v = int(guess[0]) if guess[0] > 0 else max(1024, 2 * area)
        cap_t = int(guess[1]) if guess[1] > 0 else max(1024, 4 * area)
        n = (C.c_int64 * 2)(0, 0)
        for _ in range(2):
            pos = np.empty((cap_v, 3), dtype=np.float32)
            nrm = np.empty((cap_v, 3), dtype=np.float32)
            idx = np.empty((cap_t, 3), dtype=np.int32)
            self._ck(self._L.dsl_field_surface_indexed(self._h, BUF[scalar], _fp(o), _fp(s), ip, C.c_float(iso), _fp(pos), _fp(nrm), cap_v,
                                                       idx.ctypes.data_as(C.POINTER(C.c_int32)), cap_t, n))
            if n[0] <= cap_v and n[1] <= cap_t:
                break
            cap_v, cap_t = max(cap_v, int(n[0])), max(cap_t, int(n[1]))
        return pos[:n[0]].copy(), nrm[:n[0]].copy(), idx[:n[1]].copy()

    # -- solver drivers -----------------------------------------------------------
    def wcsph_step(self, nsteps: int = 1):
        self._ck(self._L.dsl_wcsph_step(self._h, int(nsteps)))

    def pcisph_begin(self):
        self._ck(self._L.dsl_pcisph_begin(self._h))

    def pcisph_step(self, nsteps: int = 1):
        self._ck(self._L.dsl_pcisph_step(self._h, int(nsteps)))

    def sync(self):
        self._ck(self._L.dsl_sync(self._h))

    def stats(self) -> Stats:
        s = Stats()
        self._ck(self._L.dsl_get_stats(self._h, C.byref(s)))
        return s

    # -- timing ---------------------------------------------------------------------
    def timing_enable(self, on=True):
        """True / 1: every kernel; 2: only the step's dominant kernels; False / 0: off"""
        self._ck(self._L.dsl_timing_enable(self._h, int(on)))

    def timing_reset(self):
        self._ck(self._L.dsl_timing_reset(self._h))

    # library options (include/dslsph.h: DSL_OPT_*)
    OPTIONS = {"skin": 1, "skin_steps": 2, "skin_rebuilds": 3, "skin_list_overflow": 4, "skin_suspensions": 5, "device_bytes": 6, "skin_fields_own": 7, "skin_fields_padded": 8, "skin_predict": 9, "skin_tau_steps": 10,
               "density_pair": 16, "cell_keys": 17, "tile_box": 18, "persistent_blocks": 19, "pci_qtiled": 20,
               "pci_qpair": 21, "pci_qrows": 22, "pci_qincr": 23, "list_build": 24, "grid_oversub": 25, "tile_queue": 26,
               "collider_triangles": 32, "collide_hits": 33, "collide_cull": 34,
               "collide_index": 35, "collide_index_edge": 36, "collide_index_cells": 37, "collide_index_entries": 38,
               "collide_visits": 39, "collide_full_waves": 40, "collide_slab": 41,
               "volume_bricks": 48, "volume_lds_bricks": 49, "volume_fallback_bricks": 50,
               "volume_empty_bricks": 51, "volume_staged_records": 52,
               "surface_triangles": 56, "surface_active_bricks": 57, "surface_count_ms": 58, "surface_scan_ms": 59,
               "surface_emit_ms": 60, "surface_vertices": 61, "surface_mesh_vcount_ms": 62, "surface_mesh_vscan_ms": 63,
               "surface_mesh_vemit_ms": 64, "surface_mesh_iemit_ms": 65,
               "sdf_active_bricks": 72, "sdf_visits": 73, "sdf_distance_ms": 74, "sdf_sign_ms": 75, "collider_volume": 76,
               "collider_volume_moving": 77, "bodies": 78, "bodies_integrate": 79, "bodies_contact": 80,
               "bodies_contacts": 81,
               "emitters": 88, "sinks": 89, "emitted": 90, "emit_skipped": 91, "removed": 92, "sink_every": 93,
               "record_frames": 96, "record_dropped": 97, "record_ready": 98, "record_pack_ms": 99, "record_copy_ms": 100}

    def set_option(self, name: str, value: float):
        self._ck(self._L.dsl_set_option(self._h, self.OPTIONS[name], float(value)))

    def get_option(self, name: str) -> float:
        v = C.c_double(0.0)
        self._ck(self._L.dsl_get_option(self._h, self.OPTIONS[name], C.byref(v)))
        return float(v.value)

    def timing(self, kernel: str):
        ms, cnt = C.c_double(0), C.c_int64(0)
        self._ck(self._L.dsl_timing_get(self._h, KERNEL_IDS[kernel], C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value
