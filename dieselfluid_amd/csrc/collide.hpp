// collide.hpp -- the triangle-mesh collider's device records and the launchers of its kernels.  The kernels
// (kernels_collide.hpp) are compiled in a translation unit of their own, collide.hip; dslsph.hip includes this header only.
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

}  // namespace dsl
