// collider_host.hip -- the HOST side of the triangle-mesh collider: the mesh and its cell index on the handle, the collide pass,
// dsl_collider_*.  Host code only: it launches through collide.hpp, and the kernels behind those launchers are compiled in
// collide.hip (list walk), collide_index.hip (cell index) and collide_slab.hip (slab forms).
#include "engine.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

using namespace dsl;

// ---- the cell index over the collider's triangles (kernels_collide_index.hpp; DSL_OPT_COLLIDE_INDEX) ----
namespace dsl {
void col_index_free(dsl_handle* h) {
  (void)hipFree(const_cast<int*>(h->col_ix.start));
  (void)hipFree(const_cast<int*>(h->col_ix.list));
  (void)hipFree(const_cast<int*>(h->col_ix.always));
  (void)hipFree(h->col_ix.counters);
  h->dev_bytes -= h->col_ix_bytes;
  h->col_ix = ColIndex{};
  h->col_ix_bytes = 0;
  h->col_ix_cells = 0;
  h->col_ix_entries = 0;
}
}  // namespace dsl

namespace {
// What an index over the mesh that is set would be: the grid (origin, top, edge, dims of `ix`), its cells and entries.
struct ColIndexPlan {
  ColIndex ix{};
  long long cells = 0, entries = 0;
  int n_reg = 0;
};

// The grid for cell edge `edge`: false if it has more than kColIndexMaxCells cells.  dims[k] = the cell of top[k] + 1, by
// col_cell's expression (the kernels clamp to dims, so the host's rounding of it decides nothing but the grid's size).
bool col_index_grid(ColIndexPlan* pl, float edge) {
  double cells = 1.0;
  for (int k = 0; k < 3; ++k) {
    const double d = std::floor((double)((pl->ix.top[k] - pl->ix.origin[k]) / edge)) + 1.0;
    if (!(d >= 1.0 && d <= (double)kColIndexMaxCells)) return false;
    pl->ix.dims[k] = (int)d;
    cells *= d;
  }
  if (cells > (double)kColIndexMaxCells) return false;
  pl->ix.edge = edge;
  pl->cells = (long long)cells;
  return true;
}

// Plans the index for cell edge `edge_req` (0: the library's choice) without touching the handle's state.  Blocking.
// The library's choice: the mean over the regular triangles of their padded box's mean extent, doubled until the grid
// has at most 2^22 cells and the lists at most max(2^20, 64 T) entries.  An edge the host sets is taken or refused.
int col_index_plan(dsl_handle* h, float edge_req, ColIndexPlan* pl) {
  const int T = h->col_tri;
  ColBounds* dpart = nullptr;
  unsigned long long* dtotal = nullptr;
  std::vector<ColBounds> part(kColBoundsWaves);
  hipError_t e = hipMalloc((void**)&dpart, kColBoundsWaves * sizeof(ColBounds));
  if (e == hipSuccess) e = hipMalloc((void**)&dtotal, sizeof(unsigned long long));
  auto done = [&](int rc) {
    (void)hipFree(dpart);
    (void)hipFree(dtotal);
    return rc;
  };
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return done(fail(h, DSL_ERR_NOMEM, "collider index: hipMalloc failed"));
  }
  launch_index_bounds(h->stream, T, h->col_box, dpart);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(part.data(), dpart, kColBoundsWaves * sizeof(ColBounds), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return done(fail(h, DSL_ERR_DEVICE, std::string("collider index: ") + hipGetErrorString(e)));
  double ext = 0.0;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (const ColBounds& b : part) {  // (in order: the same sum every time)
    pl->n_reg += b.n_reg;
    ext += b.ext;
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::fmin(lo[k], b.lo[k]);
      hi[k] = std::fmax(hi[k], b.hi[k]);
    }
  }
  const long long budget = col_index_max_entries(T);
  const std::string budget_text = "the index's budget is 2^22 cells and max(2^20, 64 T) = " + std::to_string(budget) + " list entries";
  if (pl->n_reg == 0) {  // every triangle is on the always-list: one empty cell
    for (int k = 0; k < 3; ++k) pl->ix.origin[k] = pl->ix.top[k] = 0.0f, pl->ix.dims[k] = 1;
    pl->ix.edge = edge_req > 0.0f ? edge_req : 1.0f;
    pl->cells = 1;
    pl->entries = T;
    return done(DSL_OK);
  }
  for (int k = 0; k < 3; ++k) pl->ix.origin[k] = lo[k], pl->ix.top[k] = hi[k];
  auto entries_of = [&](unsigned long long* out) {  // the regular triangles' entries in pl's grid
    hipError_t e2 = hipMemsetAsync(dtotal, 0, sizeof(unsigned long long), h->stream);
    if (e2 == hipSuccess) {
      launch_index_total(h->stream, T, h->col_box, pl->ix, dtotal);
      e2 = hipGetLastError();
    }
    if (e2 == hipSuccess) e2 = hipMemcpyAsync(out, dtotal, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
    if (e2 == hipSuccess) e2 = hipStreamSynchronize(h->stream);
    return e2;
  };
  unsigned long long reg_entries = 0;
  if (edge_req > 0.0f) {
    if (!col_index_grid(pl, edge_req))
      return done(fail(h, DSL_ERR_INVALID, "DSL_OPT_COLLIDE_INDEX_EDGE: too many cells over this mesh; " + budget_text));
    if ((e = entries_of(&reg_entries)) != hipSuccess)
      return done(fail(h, DSL_ERR_DEVICE, std::string("collider index: ") + hipGetErrorString(e)));
    if ((long long)reg_entries + (T - pl->n_reg) > budget)
      return done(fail(h, DSL_ERR_INVALID, "DSL_OPT_COLLIDE_INDEX_EDGE: too many list entries over this mesh; " + budget_text));
  } else {
    float edge = (float)(ext / pl->n_reg);
    if (!(edge > 0.0f)) edge = 1.0f;
    for (;; edge *= 2.0f) {
      if (!std::isfinite(edge)) return done(fail(h, DSL_ERR_INVALID, "collider index: no cell edge fits this mesh; " + budget_text));
      if (!col_index_grid(pl, edge)) continue;
      if ((e = entries_of(&reg_entries)) != hipSuccess)
        return done(fail(h, DSL_ERR_DEVICE, std::string("collider index: ") + hipGetErrorString(e)));
      if ((long long)reg_entries + (T - pl->n_reg) <= budget) break;
    }
  }
  pl->entries = (long long)reg_entries + (T - pl->n_reg);
  return done(DSL_OK);
}

// Builds the planned index on the device (any earlier one is freed first).  Blocking.  On failure the handle has no
// index and the list walk runs.
int col_index_build(dsl_handle* h, const ColIndexPlan& pl) {
  col_index_free(h);
  const int T = h->col_tri, cells = (int)pl.cells, n_always = T - pl.n_reg, n_pad = col_index_pad(cells);
  ColIndex ix = pl.ix;
  ix.n_always = n_always;
  int *start = nullptr, *list = nullptr, *always = nullptr, *cnt = nullptr, *tmp = nullptr;
  unsigned long long *counters = nullptr, *dtotal = nullptr;
  size_t bytes = 0;
  auto fin = [&](int rc) {  // scratch goes either way; the index's own arrays only on failure
    (void)hipFree(cnt);
    (void)hipFree(tmp);
    (void)hipFree(dtotal);
    if (rc) {
      (void)hipFree(start);
      (void)hipFree(list);
      (void)hipFree(always);
      (void)hipFree(counters);
    }
    return rc;
  };
  auto nomem = [&] {
    (void)hipGetLastError();
    return fin(fail(h, DSL_ERR_NOMEM, "collider index: hipMalloc failed; the list walk runs"));
  };
  auto dev = [&](hipError_t e) { return fin(fail(h, DSL_ERR_DEVICE, std::string("collider index: ") + hipGetErrorString(e))); };
  if (hipMalloc((void**)&start, (size_t)n_pad * sizeof(int)) != hipSuccess) return nomem();
  if (hipMalloc((void**)&cnt, (size_t)n_pad * sizeof(int)) != hipSuccess) return nomem();
  if (hipMalloc((void**)&counters, 2 * sizeof(unsigned long long)) != hipSuccess) return nomem();
  if (hipMalloc((void**)&dtotal, sizeof(unsigned long long)) != hipSuccess) return nomem();
  if (n_always > 0 && hipMalloc((void**)&always, (size_t)n_always * sizeof(int)) != hipSuccess) return nomem();
  bytes += (size_t)n_pad * sizeof(int) + 2 * sizeof(unsigned long long) + (size_t)n_always * sizeof(int);
  ix.start = start;
  ix.always = always;
  ix.counters = counters;
  hipError_t e = hipMemsetAsync(cnt, 0, (size_t)n_pad * sizeof(int), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(counters, 0, 2 * sizeof(unsigned long long), h->stream);
  unsigned long long padded = 0;
  if (e == hipSuccess) {
    launch_index_count(h->stream, T, h->col_box, ix, n_pad, cnt, start, dtotal);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&padded, dtotal, sizeof(padded), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return dev(e);
  if (padded > 0x7fffffffull) return fin(fail(h, DSL_ERR_NOMEM, "collider index: the cell lists pass 2^31 entries; the list walk runs"));
  const size_t n_list = (size_t)std::max<unsigned long long>(padded, 4);
  if (hipMalloc((void**)&list, n_list * sizeof(int)) != hipSuccess) return nomem();
  if (hipMalloc((void**)&tmp, n_list * sizeof(int)) != hipSuccess) return nomem();
  bytes += n_list * sizeof(int);
  ix.list = list;
  e = hipMemsetAsync(list, kColNone & 0xff, n_list * sizeof(int), h->stream);
  if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, (size_t)n_pad * sizeof(int), h->stream);
  if (e == hipSuccess) {
    launch_index_fill(h->stream, T, h->col_box, ix, cells, cnt, list, tmp, always);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return dev(e);
  h->col_ix = ix;
  h->col_ix_cells = cells;
  h->col_ix_entries = pl.entries;
  h->col_ix_bytes = bytes;
  h->dev_bytes += bytes;
  return fin(DSL_OK);
}
}  // namespace

namespace dsl {
// The index follows the mesh, the option and the edge: called when any of them has changed.  A refused edge
// (DSL_ERR_INVALID) leaves the index that was built.
int col_index_update(dsl_handle* h, bool on, float edge_req) {
  if (!on || h->col_tri == 0) {
    col_index_free(h);
    return DSL_OK;
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (a pass in flight may still read the index that is replaced)
  ColIndexPlan pl;
  if (int rc = col_index_plan(h, edge_req, &pl)) return rc;
  return col_index_build(h, pl);
}
}  // namespace dsl

namespace {
// The collider pass (kernels_collide.hpp): Mesh.Collision for every fluid particle, then the build-defined response, in
// place on the current state.  Without a mesh nothing is launched.  dsl_stats.max_vel / max_f stay what Update saw.
ColMesh col_mesh(const dsl_handle* h) {
  return ColMesh{h->col_rec, h->col_box, h->col_chunk, h->col_tri, h->col_s_thr, h->col_rest, h->col_cull ? 1 : 0};
}
// The launch of either collide kernel: the walk over the cell index if one is built and the broad phase is on (cull 0
// keeps meaning "every pair is tested"), the list walk otherwise.
int collide_launch(dsl_handle* h, bool respond, ColQuery q, int* hits) {
  h->col_last_indexed = h->col_ix_cells > 0 && h->col_cull;
  if (h->col_last_indexed) {
    HIP_TRY(h, hipMemsetAsync(h->col_ix.counters, 0, 2 * sizeof(unsigned long long), h->stream));
    launch_collide_indexed(h->stream, respond, h->n, h->c.dt, bnd_of(h), col_mesh(h), h->col_ix, mpos(h, h->cur_pv),
                           mvel(h, h->cur_pv), q, hits);
  } else {
    launch_collide(h->stream, respond, h->n, h->c.dt, bnd_of(h), col_mesh(h), mpos(h, h->cur_pv), mvel(h, h->cur_pv), q, hits);
  }
  return DSL_OK;
}
// The pass on a slab rank (csrc/collide_slab.hip; the rules are at dsl_collide_pass in include/dslsph.h): exactly the
// slots the last integrate wrote.  After the band launch of the split step these lie in the OUTPUT half of the state
// and the state has not flipped; the pre-step coordinates that select band or inner slots are in the other half.
int collide_pass_slab(dsl_handle* h) {
  const int stage = h->col_stage;
  if (stage == 0)
    return fail(h, DSL_ERR_INVALID,
                "dsl_collide_pass: on a slab handle the order is integrate -> collide -> pack / append / neighbour build, one "
                "collide per integrate: nothing has been integrated since the last collide, dsl_slab_pack, dsl_slab_pack_band, "
                "dsl_slab_append, dsl_slab_exchange or dsl_build_neighbours");
  const int out = stage == 2 ? h->cur_pv ^ 1 : h->cur_pv;
  const int sel = stage - 1;
  const float* old_axis = sel != 0 ? h->pv[out ^ 1][h->c.slab_axis] : nullptr;
  const bool indexed = h->col_ix_cells > 0 && h->col_cull;
  if (!h->col_step_zeroed) {  // the counters sum over the launches of one step: band + inner
    HIP_TRY(h, hipMemsetAsync(h->col_hits, 0, sizeof(int), h->stream));
    if (indexed) HIP_TRY(h, hipMemsetAsync(h->col_ix.counters, 0, 2 * sizeof(unsigned long long), h->stream));
    h->col_step_zeroed = true;
  }
  h->col_last_indexed = indexed;
  const int rc = timed(h, DSL_K_COLLIDE, [&] {
    launch_collide_slab(h->stream, h->cap, h->c, sel, old_axis, col_mesh(h), indexed ? &h->col_ix : nullptr, mpos(h, out),
                        mvel(h, out), h->col_hits);
  });
  if (rc) return rc;
  // (a host that packs the band on a stream of its own waits for this event: it has to cover the band's collide too)
  if (stage == 2 && h->ev_band) HIP_TRY(h, hipEventRecord(h->ev_band, h->stream));
  h->col_stage = 0;
  if (stage != 2) {  // (the band launch's state is still the pre-step one: its grid and masks serve the inner launch)
    h->grid_valid = false;
    h->masks_valid = false;
  }
  return DSL_OK;
}
}  // namespace

namespace dsl {
int collide_pass(dsl_handle* h, bool step) {
  if (h->n_bodies > 0) return bodies_pass(h, step && h->bodies_integrate);  // (rigid bodies exclude a volume and a mesh: bodies.hip)
  if (h->colv_on) return collide_volume_pass(h);  // (a volume collider excludes a mesh: sdf.hip)
  if (h->col_tri == 0) return DSL_OK;
  if (h->c.n_ptr) return collide_pass_slab(h);
  HIP_TRY(h, hipMemsetAsync(h->col_hits, 0, sizeof(int), h->stream));
  int lrc = DSL_OK;
  int rc = timed(h, DSL_K_COLLIDE, [&] { lrc = collide_launch(h, true, ColQuery{}, h->col_hits); });
  if (lrc) return lrc;
  if (rc) return rc;
  h->grid_valid = false;  // positions moved
  h->masks_valid = false;
  return DSL_OK;
}
}  // namespace dsl

// ---------------------------------------------------------------------------------------
// triangle-mesh collider (kernels_collide.hpp)
// ---------------------------------------------------------------------------------------
int dsl_collider_set_mesh(dsl_handle* h, const float* vertices, const float* normals, size_t n_triangles, float radius,
                          float restitution) {
  CHECK_HANDLE(h);
  if ((h->c.slab_axis >= 0 || h->c.n_ptr) && !h->col_slab)  // (DSL_OPT_COLLIDE_SLAB: every rank sets the same mesh)
    return fail(h, DSL_ERR_UNSUPPORTED, "dsl_collider_set_mesh: a collider mesh is not supported in slab mode");
  if (n_triangles == 0) {  // removes the mesh (the arrays stay for the next one; the cell index goes)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->col_tri = 0;
    h->col_last_indexed = false;
    col_index_free(h);
    return DSL_OK;
  }
  if (h->n_bodies > 0)
    return fail(h, DSL_ERR_INVALID, "dsl_collider_set_mesh: rigid bodies exist, and a mesh collider, a volume collider and rigid bodies "
                                    "exclude each other; remove the bodies first (dsl_bodies_clear)");
  if (h->colv_on)
    return fail(h, DSL_ERR_INVALID, "dsl_collider_set_mesh: a volume collider is set, and a mesh collider and a volume collider exclude "
                                    "each other; remove the volume first (dsl_collider_set_volume with dims = NULL)");
  if (!vertices || !normals) return fail(h, DSL_ERR_INVALID, "dsl_collider_set_mesh: null vertex or normal pointer");
  if (n_triangles > ((size_t)1 << 24)) return fail(h, DSL_ERR_INVALID, "dsl_collider_set_mesh: more than 2^24 triangles");
  const int T = (int)n_triangles, nchunk = (T + kColChunk - 1) / kColChunk;
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (a pass in flight may still read the mesh that is replaced)
  h->col_tri = 0;  // no mesh until the new one is whole: a failure below leaves the handle without a collider
  h->col_last_indexed = false;
  col_index_free(h);
  if (T > h->col_alloc) {
    (void)hipFree(h->col_rec);
    (void)hipFree(h->col_box);
    (void)hipFree(h->col_chunk);
    h->col_rec = nullptr;
    h->col_box = h->col_chunk = nullptr;
    h->col_alloc = 0;
    int rc = DSL_OK;
    if ((rc = dev_alloc(h, &h->col_rec, (size_t)T))) return rc;
    if ((rc = dev_alloc(h, &h->col_box, (size_t)T))) return rc;
    if ((rc = dev_alloc(h, &h->col_chunk, (size_t)nchunk))) return rc;
    h->col_alloc = T;
  }
  if (!h->col_hits)
    if (int rc = dev_alloc(h, &h->col_hits, 1)) return rc;
  float* in = nullptr;  // the caller's arrays: 9 T vertices, then 3 T normals
  if (hipMalloc((void**)&in, (size_t)12 * T * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(h, DSL_ERR_NOMEM, "dsl_collider_set_mesh: hipMalloc failed");
  }
  hipError_t e = hipMemcpyAsync(in, vertices, (size_t)9 * T * sizeof(float), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(in + (size_t)9 * T, normals, (size_t)3 * T * sizeof(float), hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess) {
    launch_collide_prep(h->stream, T, in, in + (size_t)9 * T, radius, h->col_rec, h->col_box, h->col_chunk);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (host pointers are never retained after a call returns)
  (void)hipFree(in);
  if (e != hipSuccess) return fail(h, DSL_ERR_DEVICE, std::string("dsl_collider_set_mesh: ") + hipGetErrorString(e));
  // `Mag(q) <= r` on the float32 sum of squares: Mag is float32(sqrt(float64(s))) (vector.go:301-308), monotone in s, so
  // the test is s <= the largest float whose Mag is <= r.  None for a negative or NaN radius (s >= 0 or NaN: -1 fails all).
  float thr = -1.0f;
  if (radius >= 0.0f) {
    auto mag = [](float s) { return (float)std::sqrt((double)s); };
    thr = radius * radius;
    if (!(thr <= 3.4028235e38f)) thr = 3.4028235e38f;
    while (thr > 0.0f && mag(thr) > radius) thr = std::nextafter(thr, 0.0f);
    while (thr < INFINITY && mag(std::nextafter(thr, INFINITY)) <= radius) thr = std::nextafter(thr, INFINITY);
  }
  h->col_s_thr = thr;
  h->col_radius = radius;
  h->col_rest = restitution;
  h->col_tri = T;
  // the cell index, if it is switched on: a failure here leaves the mesh set, without an index (the list walk runs)
  return col_index_update(h, h->col_ix_on, h->col_ix_edge_req);
}

int dsl_collide_pass(dsl_handle* h) {
  CHECK_HANDLE(h);
  return collide_pass(h);
}

int dsl_collider_query(dsl_handle* h, int32_t* tri, float* normal, float* coord, float* point) {
  CHECK_HANDLE(h);
  if (h->c.n_ptr) return fail(h, DSL_ERR_UNSUPPORTED, "dsl_collider_query: not available in slab mode");
  if (h->ids_global) return fail(h, DSL_ERR_INVALID, "dsl_collider_query: host order is gone after dsl_set_ids");
  const size_t nf = (size_t)n_fluid_of(h);
  if (h->col_tri == 0) {  // Mesh.Collision of an empty mesh: no collision, empty vectors (mesh.go:56)
    if (tri) std::fill(tri, tri + nf, -1);
    for (float* a : {normal, coord, point})
      if (a) std::fill(a, a + 3 * nf, 0.0f);
    return DSL_OK;
  }
  if (!h->col_query)
    if (int rc = dev_alloc(h, &h->col_query, (size_t)10 * h->cap)) return rc;
  float* qb = h->col_query;
  const ColQuery q{tri ? reinterpret_cast<int*>(qb) : nullptr, normal ? qb + nf : nullptr, coord ? qb + 4 * nf : nullptr,
                   point ? qb + 7 * nf : nullptr, h->ids[h->cur_ids]};
  if (int rc = collide_launch(h, false, q, nullptr)) return rc;
  HIP_TRY(h, hipGetLastError());
  if (tri) HIP_TRY(h, hipMemcpyAsync(tri, q.tri, nf * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (normal) HIP_TRY(h, hipMemcpyAsync(normal, q.normal, 3 * nf * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (coord) HIP_TRY(h, hipMemcpyAsync(coord, q.coord, 3 * nf * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (point) HIP_TRY(h, hipMemcpyAsync(point, q.point, 3 * nf * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DSL_OK;
}
