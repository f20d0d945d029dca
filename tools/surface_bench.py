#!/usr/bin/env python3
"""What the fluid's surface costs: dsl_surface_extract at iso = rho0 / 2 on the volume of tools/volume_bench.py -- the
densities over the wall box of bench.py's 16M DSL_MATH_FAST dam-break after 20 steps, at step = dx (1008 x 504 x 252 = 128M
voxels, 512 MB) -- with both in device memory.

After a warm-up pair, the dsl_field_volume call that makes the volume and the extraction ALTERNATE in this one process on one
handle; each is timed by its own device events (DSL_K_VOLUME, DSL_K_SURFACE; the extraction's three phases by
DSL_OPT_SURFACE_COUNT_MS / _SCAN_MS / _EMIT_MS).  One JSON line for the plain step, one for the surface: T, active and total
bricks, count / scan / emit / total ms (mean, min, max), the volume's ms next to them, the algorithmic bytes -- every voxel
read with the bricks' 405 / 256 halo by the count sweep and again by the emit sweep in the bricks that have triangles (the
others cost their two offsets), 8 per brick and scan pass (count written, read, offset written, read twice), 48 per triangle
written; "two_full_sweeps" is the figure if the emit sweep staged every brick again -- and their share of the HBM rate a copy
reaches (6.29 TB/s).

  python tools/surface_bench.py [--n3 252] [--calls 10] [--out profiles/surface_16m.jsonl]

--indexed: the same scene and volume, made once; then dsl_surface_extract (the soup) and dsl_surface_extract_indexed (the
indexed mesh with vertex normals) ALTERNATE on it in this one process.  One JSON line for the plain step, one for the soup,
one for the indexed mesh: V, T, the phases' ms (the triangle count and scan, shared with the soup, by DSL_OPT_SURFACE_COUNT_MS /
_SCAN_MS; vertex count, vertex scan, vertex emit and index emit by DSL_OPT_SURFACE_MESH_*_MS), the total from DSL_K_SURFACE plus
DSL_K_SURFACE_MESH, the output bytes of both (48 T against 24 V + 12 T), the algorithmic bytes, and the ratio to the soup.

  python tools/surface_bench.py --indexed [--n3 252] [--calls 10] [--out profiles/surface_indexed_16m.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_TB_S = 6.29  # what a float4 copy reaches on this part (8.0 by specification)


def _stat(v):
    return {"mean": round(statistics.fmean(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n3", type=int, default=252)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--indexed", action="store_true")
    args = ap.parse_args()
    import torch
    from dieselfluid_amd import SPHEngine, scenes

    p, pos = scenes.dambreak_scene(args.n3)  # DSL_MATH_FAST, h = 2 dx
    n = args.n3 ** 3
    dx = 1.0 / args.n3
    lines = []

    def emit(rec):
        rec = {"n_particles": n, **rec}
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    eng = SPHEngine(p, device=0)
    eng.upload("positions", pos)
    eng.reset_forces()
    eng.wcsph_step(10)
    eng.sync()
    t0 = time.perf_counter()
    eng.wcsph_step(10)
    eng.sync()
    step_ms = (time.perf_counter() - t0) * 1e3 / 10
    emit({"config": "plain step, default skin", "step_ms": round(step_ms, 4), "steps_before_the_volume": 20})

    box = [float(p.box_max[a]) for a in range(3)]
    dims = [int(round(box[a] / dx)) for a in range(3)]
    origin = [0.5 * dx] * 3  # voxel centres tile the wall box
    nvox = dims[0] * dims[1] * dims[2]
    iso = 0.5 * float(p.ref_density)
    vol = torch.empty(nvox, dtype=torch.float32, device="cuda")
    eng.timing_enable(1)

    def volume():
        eng.timing_reset()
        eng.field_volume(origin, dx, dims, "densities", dev_out=vol.data_ptr())
        t, launches = eng.timing("volume")
        assert launches == 1
        return t

    volume()
    if args.indexed:
        indexed(args, eng, emit, vol, origin, dx, dims, iso, step_ms)
        eng.close()
        write(args, lines)
        return
    T = eng.surface_extract(vol.data_ptr(), origin, dx, dims, iso)  # the counting call sizes the output
    verts = torch.empty(9 * T, dtype=torch.float32, device="cuda")
    norms = torch.empty(3 * T, dtype=torch.float32, device="cuda")
    ms = {"volume": [], "count": [], "scan": [], "emit": [], "total": []}
    for rep in range(args.calls + 1):  # (rep 0: the warm-up pair)
        tv = volume()
        eng.timing_reset()
        got = eng.surface_extract(vol.data_ptr(), origin, dx, dims, iso, dev_vertices=verts.data_ptr(), dev_normals=norms.data_ptr(),
                                  cap=T)
        assert got == T
        avg, launches = eng.timing("surface")
        assert launches == 3
        if rep > 0:
            ms["volume"].append(tv)
            ms["total"].append(avg * launches)
            for k in ("count", "scan", "emit"):
                ms[k].append(eng.get_option("surface_%s_ms" % k))
    active = int(eng.get_option("surface_active_bricks"))
    bricks = ((dims[0] - 1 + 7) // 8) * ((dims[1] - 1 + 7) // 8) * ((dims[2] - 1 + 3) // 4)
    count_bytes = 4 * 405 * bricks  # a sweep stages 405 voxels per brick of 256 cubes
    read_bytes = count_bytes + 4 * 405 * active
    scan_bytes = 5 * 8 * bricks
    tri_bytes = 48 * T
    nbytes = read_bytes + scan_bytes + tri_bytes
    total = statistics.fmean(ms["total"])
    emit({"config": "surface of the step = dx volume", "scalar": "densities", "iso": iso, "origin": origin, "step": dx, "dims": dims,
          "voxels": nvox, "triangles": T, "active_bricks": active, "bricks": bricks, "timed_calls": args.calls,
          "count_ms": _stat(ms["count"]), "scan_ms": _stat(ms["scan"]), "emit_ms": _stat(ms["emit"]), "surface_ms": _stat(ms["total"]),
          "volume_ms": _stat(ms["volume"]), "surface_over_volume": round(total / statistics.fmean(ms["volume"]), 3),
          "surface_over_plain_step": round(total / step_ms, 3),
          "algorithmic_bytes": {"voxels_read": read_bytes, "scan": scan_bytes, "triangles_written": tri_bytes, "all": nbytes,
                                "two_full_sweeps": 2 * count_bytes + scan_bytes + tri_bytes},
          "algorithmic_gb_per_s": round(nbytes / (total * 1e-3) / 1e9, 1),
          "hbm_share_of_copy_rate": round(nbytes / (total * 1e-3) / (HBM_COPY_TB_S * 1e12), 3),
          "count_gb_per_s": round(count_bytes / (statistics.fmean(ms["count"]) * 1e-3) / 1e9, 1)})
    eng.close()
    write(args, lines)


def write(args, lines):
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def indexed(args, eng, emit, vol, origin, dx, dims, iso, step_ms):
    """the soup and the indexed mesh, alternating on one volume"""
    import torch
    nvox = dims[0] * dims[1] * dims[2]
    V, T = eng.surface_extract_indexed(vol.data_ptr(), origin, dx, dims, iso)  # the counting call sizes the outputs
    assert T == eng.surface_extract(vol.data_ptr(), origin, dx, dims, iso)
    verts = torch.empty(9 * T, dtype=torch.float32, device="cuda")
    norms = torch.empty(3 * T, dtype=torch.float32, device="cuda")
    pos = torch.empty(3 * V, dtype=torch.float32, device="cuda")
    vnrm = torch.empty(3 * V, dtype=torch.float32, device="cuda")
    idx = torch.empty(3 * T, dtype=torch.int32, device="cuda")
    soup = {k: [] for k in ("count", "scan", "emit", "total")}
    mesh = {k: [] for k in ("count", "scan", "vcount", "vscan", "vemit", "iemit", "total")}
    for rep in range(args.calls + 1):  # (rep 0: the warm-up pair)
        eng.timing_reset()
        assert eng.surface_extract(vol.data_ptr(), origin, dx, dims, iso, dev_vertices=verts.data_ptr(), dev_normals=norms.data_ptr(),
                                   cap=T) == T
        avg, launches = eng.timing("surface")
        assert launches == 3
        if rep > 0:
            soup["total"].append(avg * launches)
            for k in ("count", "scan", "emit"):
                soup[k].append(eng.get_option("surface_%s_ms" % k))
        eng.timing_reset()
        assert eng.surface_extract_indexed(vol.data_ptr(), origin, dx, dims, iso, dev_positions=pos.data_ptr(), dev_normals=vnrm.data_ptr(),
                                           cap_vertices=V, dev_indices=idx.data_ptr(), cap_triangles=T) == (V, T)
        a0, l0 = eng.timing("surface")
        a1, l1 = eng.timing("surface_mesh")
        assert (l0, l1) == (2, 4)
        if rep > 0:
            mesh["total"].append(a0 * l0 + a1 * l1)
            for k in ("count", "scan"):
                mesh[k].append(eng.get_option("surface_%s_ms" % k))
            for k in ("vcount", "vscan", "vemit", "iemit"):
                mesh[k].append(eng.get_option("surface_mesh_%s_ms" % k))
    active = int(eng.get_option("surface_active_bricks"))
    # the mesh against the soup it indexes, on the device: positions[indices] are the soup's vertices, bit for bit
    same = bool(torch.equal(pos.view(torch.int32).view(-1, 3)[idx.long()].view(-1), verts.view(torch.int32)))
    referenced = int(torch.unique(idx).numel())
    # the bricks of 8 x 8 x 4 voxels that own a vertex: ESTIMATED from the positions (a vertex lies on an edge that starts at
    # its owner, so the floor of its lattice coordinates is the owner but for a vertex that rounds onto the edge's far end)
    o = torch.tensor(origin, dtype=torch.float64, device="cuda")
    cell = torch.floor((pos.view(-1, 3).double() - o) / dx + 1e-6).long().clamp_(min=0)
    nvx, nvy, nvz = -(-dims[0] // 8), -(-dims[1] // 8), -(-dims[2] // 4)
    vactive = int(torch.unique(((cell[:, 2] // 4) * nvy + cell[:, 1] // 8) * nvx + cell[:, 0] // 8).numel())
    bricks = ((dims[0] - 1 + 7) // 8) * ((dims[1] - 1 + 7) // 8) * ((dims[2] - 1 + 3) // 4)
    vbricks = nvx * nvy * nvz
    count_bytes = 4 * 405 * bricks
    scan_bytes = 5 * 8 * bricks
    soup_bytes = count_bytes + 4 * 405 * active + scan_bytes + 48 * T
    parts = {"triangle_count": count_bytes, "triangle_scan": scan_bytes,
             # the 10 x 10 x 6 image read by every brick of voxels, a word per voxel written by those that own a vertex
             "vertex_count": 4 * 600 * vbricks + 4 * 256 * vactive + 8 * vbricks,
             "vertex_scan": 5 * 8 * vbricks,
             "vertex_emit": 16 * vbricks + (4 * 847 + 4 * 256) * vactive + 24 * V,
             "index_emit": 16 * bricks + (2 * 4 * 405 + 64) * active + 12 * T}
    mesh_bytes = sum(parts.values())
    st, mt = statistics.fmean(soup["total"]), statistics.fmean(mesh["total"])
    emit({"config": "soup of the step = dx volume (alternating with the indexed mesh)", "iso": iso, "dims": dims, "voxels": nvox,
          "triangles": T, "active_bricks": active, "bricks": bricks, "timed_calls": args.calls,
          "count_ms": _stat(soup["count"]), "scan_ms": _stat(soup["scan"]), "emit_ms": _stat(soup["emit"]), "surface_ms": _stat(soup["total"]),
          "output_bytes": 48 * T, "algorithmic_bytes": soup_bytes, "algorithmic_gb_per_s": round(soup_bytes / (st * 1e-3) / 1e9, 1),
          "surface_over_plain_step": round(st / step_ms, 3)})
    emit({"config": "indexed mesh of the same volume", "iso": iso, "dims": dims, "voxels": nvox, "vertices": V, "triangles": T,
          "vertices_referenced": referenced, "positions_through_indices_equal_the_soup": same,
          "active_bricks": active, "bricks": bricks, "voxel_bricks": vbricks, "active_voxel_bricks_estimated": vactive,
          "timed_calls": args.calls,
          "count_ms": _stat(mesh["count"]), "scan_ms": _stat(mesh["scan"]), "vertex_count_ms": _stat(mesh["vcount"]),
          "vertex_scan_ms": _stat(mesh["vscan"]), "vertex_emit_ms": _stat(mesh["vemit"]), "index_emit_ms": _stat(mesh["iemit"]),
          "mesh_ms": _stat(mesh["total"]), "output_bytes": 24 * V + 12 * T, "output_bytes_over_soup": round((24 * V + 12 * T) / (48 * T), 3),
          "library_words_bytes": 4 * nvox, "algorithmic_bytes": {**parts, "all": mesh_bytes},
          "algorithmic_gb_per_s": round(mesh_bytes / (mt * 1e-3) / 1e9, 1),
          "hbm_share_of_copy_rate": round(mesh_bytes / (mt * 1e-3) / (HBM_COPY_TB_S * 1e12), 3),
          "mesh_over_soup": round(mt / st, 3), "mesh_over_plain_step": round(mt / step_ms, 3)})


if __name__ == "__main__":
    main()
