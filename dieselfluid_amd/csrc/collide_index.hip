// collide_index.hip -- the cell index over the collider's triangles and the collide kernel that walks it
// (kernels_collide_index.hpp), with their launchers (collide.hpp): the third translation unit of libdslsph.so.  Same
// flags as collide.hip: -ffp-contract=off is what makes the narrow phase's arithmetic the reference's.
#include "kernels_collide_index.hpp"

namespace dsl {

int col_index_pad(int cells) { return (cells + 1 + kColScanTrip - 1) / kColScanTrip * kColScanTrip; }

void launch_index_bounds(hipStream_t stream, int n_tri, const TriBox* box, ColBounds* out) {
  hipLaunchKernelGGL(k_index_bounds, dim3(kColBoundsWaves), dim3(kWave), 0, stream, n_tri, box, out);
}

void launch_index_total(hipStream_t stream, int n_tri, const TriBox* box, ColIndex ix, unsigned long long* total) {
  hipLaunchKernelGGL(k_index_total, dim3((n_tri + kColChunk - 1) / kColChunk), dim3(kColChunk), 0, stream, n_tri, box, ix, total);
}

void launch_index_count(hipStream_t stream, int n_tri, const TriBox* box, ColIndex ix, int n_pad, int* cnt, int* start,
                        unsigned long long* total) {
  hipLaunchKernelGGL(k_index_scatter<false>, dim3((n_tri + kColChunk - 1) / kColChunk), dim3(kColChunk), 0, stream, n_tri, box, ix,
                     cnt, nullptr);
  hipLaunchKernelGGL(k_index_scan, dim3(1), dim3(kWave), 0, stream, n_pad, cnt, start, total);
}

void launch_index_fill(hipStream_t stream, int n_tri, const TriBox* box, ColIndex ix, int cells, int* cnt, int* list, int* tmp,
                       int* always) {
  int bits = 1;
  while (bits < 31 && (1 << bits) < n_tri) ++bits;
  hipLaunchKernelGGL(k_index_scatter<true>, dim3((n_tri + kColChunk - 1) / kColChunk), dim3(kColChunk), 0, stream, n_tri, box, ix,
                     cnt, list);
  const int per = kColBlock / kWave;  // one wave per cell
  hipLaunchKernelGGL(k_index_sort, dim3((cells + per - 1) / per), dim3(kColBlock), 0, stream, cells, bits, cnt, ix.start, list, tmp);
  if (always) hipLaunchKernelGGL(k_index_always, dim3(1), dim3(kWave), 0, stream, n_tri, box, always);
}

void launch_collide_indexed(hipStream_t stream, bool respond, int n, float dt, Bnd bnd, ColMesh m, ColIndex ix, Soa3 p, Soa3 v,
                            ColQuery q, int* hits) {
  const dim3 g((n + kColBlock - 1) / kColBlock), b(kColBlock);
  if (respond) hipLaunchKernelGGL(k_collide_indexed<true>, g, b, 0, stream, n, dt, bnd, m, ix, p, v, q, hits);
  else hipLaunchKernelGGL(k_collide_indexed<false>, g, b, 0, stream, n, dt, bnd, m, ix, p, v, q, hits);
}

}  // namespace dsl
