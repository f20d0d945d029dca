// collide.hpp -- the triangle-mesh collider's device records and the launchers of its kernels.  The kernels are compiled
// in translation units of their own -- kernels_collide.hpp in collide.hip, kernels_collide_index.hpp in
// collide_index.hip, the slab forms of both walks in collide_slab.hip; the host units (engine.hpp) include this header only.
#pragma once

#include "sph_device.hpp"

namespace dsl {

constexpr int kColBlock = 256;  // lanes per workgroup of k_collide
constexpr int kColChunk = 256;  // triangles per broad-phase chunk

// a, e0 = b - a, e1 = c - a, n, d00 = e0.e0, d01 = e0.e1, d11 = e1.e1, denom = d00 d11 - d01 d01 (tri.go:81-89): the
// per-triangle half of Barycentric, the same whether computed once or per particle
struct alignas(64) TriRec {
  float a[3], e0[3], e1[3], n[3];
  float d00, d01, d11, denom;
};
// Broad phase: the box a colliding particle of a REGULAR triangle must lie in (triangle's bounding box, inflated), and
// whether the triangle is regular; for a chunk: the union over its triangles / all of them regular.
struct alignas(32) TriBox {
  float lo[3], hi[3];
  int regular;
  int pad_;
};

struct ColMesh {
  const TriRec* rec;
  const TriBox* box;    // per triangle
  const TriBox* chunk;  // per kColChunk triangles
  int n_tri;
  float s_thr;  // `dist <= r` on the float32 sum of squares
  float rest;   // restitution e
  int cull;
};

// The cell index over the triangles (kernels_collide_index.hpp; DSL_OPT_COLLIDE_INDEX): cubic cells of edge `edge` over
// [origin, top], the union of the REGULAR triangles' padded boxes.  Cell c lists the regular triangles whose box
// overlaps it, ascending, in list[start[c] .. start[c + 1]): every segment begins on a multiple of four entries and is
// filled up with kColNone, so a lane reads its list in aligned 16-byte windows.  `always`: the irregular triangles,
// ascending -- every wave merges them in.  counters: [0] triangle records loaded, [1] waves that walked the whole list.
constexpr int kColNone = 0x7f7f7f7f;  // (a byte pattern: the list is filled with hipMemset) past every triangle index
struct ColIndex {
  const int* start;  // cells + 1
  const int* list;
  const int* always;
  int n_always;
  int dims[3];
  float origin[3], top[3];
  float edge;
  unsigned long long* counters;
};
// the index's budget: cells, and list entries for T triangles
constexpr long long kColIndexMaxCells = 1ll << 22;
constexpr long long col_index_max_entries(long long T) { return 64 * T > (1ll << 20) ? 64 * T : (1ll << 20); }
// one wave's share of k_index_bounds: over its regular triangles' padded boxes
struct ColBounds {
  float lo[3], hi[3];
  double ext;  // sum over the triangles of the box's mean extent
  int n_reg;
  int pad_;
};
constexpr int kColBoundsWaves = 256;

// the four returns of Mesh.Collision in HOST order (index = particle id), xyz interleaved; any pointer may be null
struct ColQuery {
  int* tri;
  float *normal, *coord, *point;
  const int* ids;  // slot -> particle
};

// The launches, on `stream`; errors are left for the caller's hipGetLastError.
// collide_prep: k_collide_prep + k_collide_chunks over n_tri triangles (verts 9 floats, normals 3 floats each, device arrays).
void launch_collide_prep(hipStream_t stream, int n_tri, const float* verts, const float* normals, float r, TriRec* rec,
                         TriBox* box, TriBox* chunk);
// collide: k_collide<respond> over n particle slots.
void launch_collide(hipStream_t stream, bool respond, int n, float dt, Bnd bnd, ColMesh m, Soa3 p, Soa3 v, ColQuery q, int* hits);


// collide_index.hip.  index_bounds: out[kColBoundsWaves], the host combines them in order.  index_total: *total += the
// cells every regular triangle's box overlaps in the grid of `ix` (dims, origin, top, edge).  index_build: counts into
// cnt (zeroed, col_index_pad(cells) entries), start (as many) from their scan, segments rounded up to four entries, and
// *total = start[cells]; the caller allocates list (filled with kColNone) and tmp of that many entries, zeroes cnt again,
// and index_fill writes the ascending lists (tmp: scratch of the sort) and the always-list (null: none).
void launch_index_bounds(hipStream_t stream, int n_tri, const TriBox* box, ColBounds* out);
void launch_index_total(hipStream_t stream, int n_tri, const TriBox* box, ColIndex ix, unsigned long long* total);
void launch_index_count(hipStream_t stream, int n_tri, const TriBox* box, ColIndex ix, int n_pad, int* cnt, int* start,
                        unsigned long long* total);
void launch_index_fill(hipStream_t stream, int n_tri, const TriBox* box, ColIndex ix, int cells, int* cnt, int* list, int* tmp,
                       int* always);
int col_index_pad(int cells);  // entries of the count and start arrays for that many cells
// collide over the index: k_collide_indexed<respond>; m.cull is taken as 1
void launch_collide_indexed(hipStream_t stream, bool respond, int n, float dt, Bnd bnd, ColMesh m, ColIndex ix, Soa3 p, Soa3 v,
                            ColQuery q, int* hits);

// collide_slab.hip: the response pass of a slab rank (DSL_OPT_COLLIDE_SLAB).  The live count is read from c.n_ptr, so
// the launch covers `cap` slots.  sel = 0: every live slot the last integrate wrote (a ghost's position is NaN: never
// queried); 1: only the slots whose cell BEFORE the step, along the slab axis, is a band layer of the split step
// (slab_band_cell on old_axis, as k_slab_count / k_slab_write decide it); 2: only the others.  A slot that is not
// selected is not read beyond old_axis.  The walk over the cell index if `ix` is given, the list walk otherwise.
void launch_collide_slab(hipStream_t stream, int cap, const DevConsts& c, int sel, const float* old_axis, ColMesh m,
                         const ColIndex* ix, Soa3 p, Soa3 v, int* hits);

}  // namespace dsl
