// collide.hip -- the triangle-mesh collider's kernels (kernels_collide.hpp) and their launchers (collide.hpp): a
// translation unit of its own, linked into libdslsph.so next to dslsph.hip.  Same flags: -ffp-contract=off is what makes
// the kernels' arithmetic the reference's.
#include "kernels_collide.hpp"

namespace dsl {

void launch_collide_prep(hipStream_t stream, int n_tri, const float* verts, const float* normals, float r, TriRec* rec,
                         TriBox* box, TriBox* chunk) {
  const int nchunk = (n_tri + kColChunk - 1) / kColChunk;
  hipLaunchKernelGGL(k_collide_prep, dim3(nchunk), dim3(kColChunk), 0, stream, n_tri, verts, normals, r, rec, box);
  hipLaunchKernelGGL(k_collide_chunks, dim3((nchunk + 63) / 64), dim3(64), 0, stream, n_tri, box, chunk);
}

void launch_collide(hipStream_t stream, bool respond, int n, float dt, Bnd bnd, ColMesh m, Soa3 p, Soa3 v, ColQuery q, int* hits) {
  const dim3 g((n + kColBlock - 1) / kColBlock), b(kColBlock);
  if (respond) hipLaunchKernelGGL(k_collide<true>, g, b, 0, stream, n, dt, bnd, m, p, v, q, hits);
  else hipLaunchKernelGGL(k_collide<false>, g, b, 0, stream, n, dt, bnd, m, p, v, q, hits);
}

}  // namespace dsl
