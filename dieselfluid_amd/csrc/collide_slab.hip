// collide_slab.hip -- the collider's response pass on a slab rank (DSL_OPT_COLLIDE_SLAB): the slab forms of the list walk
// and of the walk over the cell index, with their launcher (collide.hpp).  A translation unit of its own, same flags as
// collide.hip: -ffp-contract=off is what makes the narrow phase's arithmetic the reference's.
//
// The walks (collide_walk.hpp), the narrow phase and the epilogue (collide_narrow.hpp) are the single-domain kernels';
// what differs is which lanes take part.  A rank keeps its live count on the device, holds ghosts next to the particles
// it owns, and in the split step integrates the band cell layers before the others:
//   - live count: *c.n_ptr; workgroups past it return at once;
//   - ghosts: the integrate that has just run wrote NaN into their positions.  A lane whose position is NaN is not live:
//     it loads no velocity, holds zeros, and so is never queried, never counted, never widens its wave's broad-phase box
//     and never makes the wave slow;
//   - sel 1 / 2: only the slots of the band layers / of the other layers, decided by the cell of the coordinate BEFORE
//     the step (old_axis) -- the rule of k_slab_count / k_slab_write (kernels_grid.hpp), so the pass touches exactly what
//     the launch before it integrated.  A lane that is not selected reads old_axis[i] and nothing else: its place in the
//     output arrays is either not written yet or already in a band message.
#include "collide_walk.hpp"

namespace dsl {

// The wave-wide float minimum / maximum in registers, the steps of wave_min_i32 (collide_walk.hpp): no LDS crossbar.
// Every lane of the wave must be active.  Minimum and maximum are exact, so the box is wave_min's / wave_max's.
template <bool MAX>
__device__ __forceinline__ float wave_reduce_dpp(float x) {
  int v = __float_as_int(x);
  auto op = [](int a, int b) {
    const float fa = __int_as_float(a), fb = __int_as_float(b);
    return __float_as_int(MAX ? fmaxf(fa, fb) : fminf(fa, fb));
  };
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));   // quad_perm:[1,0,3,2]
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));   // quad_perm:[2,3,0,1]
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));  // row_mirror
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xA, 0xF, false));  // row_bcast:15 into rows 1 and 3
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xC, 0xF, false));  // row_bcast:31 into rows 2 and 3
  return __int_as_float(__builtin_amdgcn_readlane(v, kWave - 1));
}
__device__ __forceinline__ float wave_min_dpp(float x) { return wave_reduce_dpp<false>(x); }
__device__ __forceinline__ float wave_max_dpp(float x) { return wave_reduce_dpp<true>(x); }

// is slot i one of this pass's particles?  If so its position and velocity are loaded.
__device__ __forceinline__ bool col_slab_load(const DevConsts& c, int n, int sel, const float* __restrict__ old_axis, int i,
                                              Soa3 p, Soa3 v, float& px, float& py, float& pz, float& vx, float& vy, float& vz) {
  bool pick = i < n;
  if (pick && sel != 0) {
    const int a = c.slab_axis;
    pick = slab_band_cell(c, cell_coord(old_axis[i], c.gmin[a], c.inv_cell, c.dims[a])) == (sel == 1);
  }
  if (!pick) return false;
  const float x = p.x[i], y = p.y[i], z = p.z[i];
  if (!(x == x && y == y && z == z)) return false;  // a ghost of the step just integrated
  px = x;
  py = y;
  pz = z;
  vx = v.x[i];
  vy = v.y[i];
  vz = v.z[i];
  return true;
}

__global__ __launch_bounds__(kColBlock) void k_collide_slab(DevConsts c, float dt, int sel, const float* __restrict__ old_axis,
                                                         ColMesh m, Soa3 p, Soa3 v, int* __restrict__ hits) {
  const int n = live_n(c);
  if ((int)(blockIdx.x * kColBlock) >= n) return;  // (the whole workgroup: the capacity is launched, not the count)
  const int i = blockIdx.x * kColBlock + threadIdx.x;
  float px = 0.f, py = 0.f, pz = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
  const bool live = col_slab_load(c, n, sel, old_axis, i, p, v, px, py, pz, vx, vy, vz);
  DSL_COL_WALK_LIST(wave_min_dpp, wave_max_dpp);
  col_finish<true>(i, live, dt, m.rest, hit, px, py, pz, vx, vy, vz, p, v, ColQuery{}, hits);
}

__global__ __launch_bounds__(kColBlock) void k_collide_slab_indexed(DevConsts c, float dt, int sel,
                                                                 const float* __restrict__ old_axis, ColMesh m, ColIndex ix,
                                                                 Soa3 p, Soa3 v, int* __restrict__ hits) {
  const int n = live_n(c);
  if ((int)(blockIdx.x * kColBlock) >= n) return;
  const int i = blockIdx.x * kColBlock + threadIdx.x;
  float px = 0.f, py = 0.f, pz = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
  const bool live = col_slab_load(c, n, sel, old_axis, i, p, v, px, py, pz, vx, vy, vz);
  DSL_COL_WALK_INDEXED();
  col_finish<true>(i, live, dt, m.rest, hit, px, py, pz, vx, vy, vz, p, v, ColQuery{}, hits);
}

void launch_collide_slab(hipStream_t stream, int cap, const DevConsts& c, int sel, const float* old_axis, ColMesh m,
                         const ColIndex* ix, Soa3 p, Soa3 v, int* hits) {
  const dim3 g((cap + kColBlock - 1) / kColBlock), b(kColBlock);
  if (ix) hipLaunchKernelGGL(k_collide_slab_indexed, g, b, 0, stream, c, c.dt, sel, old_axis, m, *ix, p, v, hits);
  else hipLaunchKernelGGL(k_collide_slab, g, b, 0, stream, c, c.dt, sel, old_axis, m, p, v, hits);
}

}  // namespace dsl
