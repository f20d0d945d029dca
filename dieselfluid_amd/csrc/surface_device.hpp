// surface_device.hpp -- what the two fluid-surface units share on the device: surface.hip (the triangle soup) and
// surface_mesh.hip (the indexed mesh).  The lattice with its brick counts, the brick of 8 x 8 x 4 cubes with its 9 x 9 x 5 staged
// voxels, the inside mask of a cube, and the prefix over a workgroup.  Everything is __forceinline__ in an unnamed
// namespace: each unit gets its own copy, and no __global__ function lives here.
#pragma once

#include "lattice.hpp"
#include "surface_table.hpp"

namespace dsl {

constexpr int kSurfBlock = 256;
// a brick of cubes: lanes x fastest, a wave is one z layer of 8 x 8 cubes
constexpr int kSurfBX = 8, kSurfBY = 8, kSurfBZ = 4;
constexpr int kSurfVX = kSurfBX + 1, kSurfVY = kSurfBY + 1, kSurfVZ = kSurfBZ + 1;
constexpr int kSurfVoxels = kSurfVX * kSurfVY * kSurfVZ;  // 405 floats of LDS
constexpr int kSurfScanTile = kSurfBlock;                 // values per workgroup of a scan level
static_assert(kSurfBX * kSurfBY * kSurfBZ == kSurfBlock && kSurfBX * kSurfBY == kWave, "one lane per cube, one wave per layer");

typedef unsigned long long surf_u64;

struct SurfLattice : Lattice {
  int nbx, nby;  // bricks of 8 x 8 x 4 cubes along x and y
};

namespace {
struct SurfBrick {
  int bi, bj, bk;
};
__device__ __forceinline__ SurfBrick surf_brick(const SurfLattice& g, int b) {
  SurfBrick k;
  k.bi = b % g.nbx;
  const int bjk = b / g.nbx;
  k.bj = bjk % g.nby;
  k.bk = bjk / g.nby;
  return k;
}

// The brick's 9 x 9 x 5 voxel values into LDS, rows of 9 consecutive floats.  A voxel outside the lattice is staged as NaN,
// so a cube that overhangs the lattice falls under the non-finite rule and emits nothing.
__device__ __forceinline__ void surf_stage(const float* __restrict__ vol, const SurfLattice& g, const SurfBrick& k, float* s_v) {
  for (int e = threadIdx.x; e < kSurfVoxels; e += kSurfBlock) {
    const int row = e / kSurfVX, xo = e - row * kSurfVX;
    const int ry = row % kSurfVY, rz = row / kSurfVY;
    const int vi = k.bi * kSurfBX + xo, vj = k.bj * kSurfBY + ry, vk = k.bk * kSurfBZ + rz;
    float v = __builtin_nanf("");
    if (vi < g.n[0] && vj < g.n[1] && vk < g.n[2]) v = vol[((size_t)vk * g.n[1] + vj) * g.n[0] + vi];
    s_v[e] = v;
  }
  lds_barrier();
}

__device__ __forceinline__ int surf_corner_at(int base, int c) {
  return base + (c & 1) + kSurfVX * ((c >> 1) & 1) + kSurfVX * kSurfVY * (c >> 2);
}

// the lane's cube: its first voxel in the LDS image and its 8-bit inside mask -- 0 (nothing to emit) if a corner is not finite
__device__ __forceinline__ unsigned surf_mask(const float* s_v, float iso, int base) {
  unsigned mask = 0;
  bool finite = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float v = s_v[surf_corner_at(base, c)];
    finite = finite && (fabsf(v) <= 3.402823466e+38f);
    mask |= (v >= iso ? 1u : 0u) << c;
  }
  return finite ? mask : 0u;
}

__device__ __forceinline__ int surf_lane_base(int tid) {
  const int cx = tid & (kSurfBX - 1), cy = (tid / kSurfBX) & (kSurfBY - 1), cz = tid / (kSurfBX * kSurfBY);
  return (cz * kSurfVY + cy) * kSurfVX + cx;
}

// inclusive prefix over the workgroup's 256 lanes: shuffles inside a wave, one LDS step over the four waves.  total: the
// workgroup's sum
template <class T>
__device__ __forceinline__ T surf_block_scan(T v, T* s_wave, T& total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  T incl = v;
  for (int off = 1; off < kWave; off <<= 1) {
    const T o = __shfl_up(incl, off, kWave);
    if (lane >= off) incl += o;
  }
  if (lane == kWave - 1) s_wave[wave] = incl;
  lds_barrier();
  T before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kSurfBlock / kWave; ++w) {
    const T s = s_wave[w];
    if (w < wave) before += s;
    total += s;
  }
  return incl + before;
}
}  // namespace

}  // namespace dsl
