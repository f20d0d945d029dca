// slab_balance.hip -- the count behind the slab re-balancing (slab_balance.hpp): how many particles this rank owns in
// every cell layer along the slab axis.  A translation unit of its own, linked into libdslsph.so next to dslsph.hip; its
// kernel list is tests/golden/device_kernels_slab_balance.txt.  Launched once per look (every M steps), never by a step
// that takes no look.
#include "slab_balance.hpp"

namespace dsl {

// One lane per live slot, grid-stride.  The slots are cell-sorted (the appended ghosts and migrants behind them are in
// band order), so the lanes of a wave mostly share a layer: equal-layer runs are found with one ballot, as k_cell_rank
// finds its equal-cell runs, and only a run's first lane adds -- the run's length -- to the workgroup's histogram in
// LDS.  At its end a workgroup adds its non-zero bins to the global counts, one atomic each.  Integer sums: the result
// does not depend on the order.
__global__ __launch_bounds__(kBalBlock) void k_slab_layer_count(DevConsts c, const float* __restrict__ pa, float origin,
                                                                int n_layers, int* __restrict__ counts) {
  __shared__ int hist[kBalMaxLayers];
  for (int k = threadIdx.x; k < n_layers; k += kBalBlock) hist[k] = 0;
  lds_barrier();
  const int lane = threadIdx.x & (kWave - 1);
  const int n = live_n(c);
  // (the trip count is the same for every lane of a workgroup: ballot and shuffle see whole waves)
  for (int first = blockIdx.x * kBalBlock; first < n; first += gridDim.x * kBalBlock) {
    const int i = first + (int)threadIdx.x;
    int layer = -1;  // not counted: past the end, a ghost, or NaN
    if (i < n) {
      const float v = pa[i];
      // the layer rule is the cell rule (cell_coord), on the caller's origin: floor((p - origin) * inv_cell), clamped
      if (slab_owned(c, v, v, v)) layer = cell_coord(v, origin, c.inv_cell, n_layers);
    }
    const int prev = __shfl_up(layer, 1, kWave);
    const bool head = lane == 0 || layer != prev;
    const unsigned long long heads = __ballot(head);
    if (head && layer >= 0) {
      const unsigned long long above = lane == kWave - 1 ? 0ull : (heads & ~((2ull << lane) - 1ull));
      const int next = above ? __builtin_ctzll(above) : kWave;
      atomicAdd(&hist[layer], next - lane);
    }
  }
  lds_barrier();
  for (int k = threadIdx.x; k < n_layers; k += kBalBlock) {
    const int v = hist[k];
    if (v != 0) atomicAdd(&counts[k], v);
  }
}

void launch_slab_layer_count(hipStream_t stream, DevConsts c, int slots, CSoa3 p, float origin, int n_layers, int* counts) {
  const float* pa = c.slab_axis == 0 ? p.x : (c.slab_axis == 1 ? p.y : p.z);
  int blocks = (slots + kBalBlock - 1) / kBalBlock;
  blocks = blocks < 1 ? 1 : (blocks > kBalMaxBlocks ? kBalMaxBlocks : blocks);
  hipLaunchKernelGGL(k_slab_layer_count, dim3(blocks), dim3(kBalBlock), 0, stream, c, pa, origin, n_layers, counts);
}

}  // namespace dsl
