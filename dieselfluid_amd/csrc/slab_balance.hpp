// slab_balance.hpp -- the launcher of the slab re-balancing count (dsl_slab_layer_counts, the look of
// dsl_slab_rebalance): owned particles per cell layer along the slab axis.  The kernel is compiled in a translation
// unit of its own, slab_balance.hip; slab_link.hip includes this header only.
#pragma once

#include "sph_device.hpp"

namespace dsl {

constexpr int kBalBlock = 256;       // lanes per workgroup of k_slab_layer_count
constexpr int kBalMaxLayers = 4096;  // bins of its LDS histogram (16 KB)
constexpr int kBalMaxBlocks = 1024;  // its grid is capped: every workgroup flushes a histogram of its own

// counts[layer] += the owned (slab_owned: inside [slab_lo, slab_hi), not NaN) particles among the live slots whose
// coordinate along c.slab_axis falls into layer floor((p - origin) * c.inv_cell), clamped to [0, n_layers).  `slots`:
// an upper bound of the live count (the capacity, in slab mode); 1 <= n_layers <= kBalMaxLayers and c.slab_axis >= 0 are
// the caller's to check, and counts[0 .. n_layers) the caller's to zero.  On `stream`; errors are left for the
// caller's hipGetLastError.
void launch_slab_layer_count(hipStream_t stream, DevConsts c, int slots, CSoa3 p, float origin, int n_layers, int* counts);

}  // namespace dsl
