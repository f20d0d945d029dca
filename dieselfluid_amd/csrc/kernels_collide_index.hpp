// kernels_collide_index.hpp -- a uniform-grid index over the collider's triangles (DSL_OPT_COLLIDE_INDEX) and the collide
// kernel that walks it.  Results are the list walk's (kernels_collide.hpp), bit for bit: the narrow phase and the epilogue
// are the same functions (collide_narrow.hpp), and a lane meets the triangles that can hit it in list order.
//
// Soundness.  k_collide_prep marks a triangle REGULAR and pads its box so that a particle with Mag(V)^2 >= 1.0001e-8 can
// hit it only from inside that box (the argument is in kernels_collide.hpp).  The index is a grid of cubic cells over
// [origin, top], the union of the regular triangles' boxes; a regular triangle is listed in every cell its box overlaps.
// The cell range of a box and the cell of a particle come from ONE monotone float32 expression (col_cell): a position
// inside the box cannot land outside the box's cell range, whatever the rounding.  So a lane's candidates are its own
// cell's list plus the irregular triangles (the "always" list: a zero or oblique normal, a needle, a degenerate triangle, a
// non-finite value); a lane outside [origin, top] -- a NaN position compares false and is outside -- has none of the
// former.  Both lists ascend, the wave visits the union of its lanes' candidates in ascending order, and every lane still
// looking tests every visited triangle: a superset of its candidates, in list order, so the first hit is the list walk's.
// A lane with a non-finite position tests what the others visit and, as in the list walk, hits nothing (k or the
// distance is NaN).  A wave with a slow lane (0 < Mag(V)^2 < 1.0001e-8, or NaN) walks the whole list, as k_collide does.
//
// Every visit is wave-uniform: the triangle index is a scalar (readlane of the wave-wide minimum), so the record still
// arrives through one 16-dword scalar load.
//
// The build is deterministic (two builds give the same bytes): count per cell, scan, fill with atomics, then every cell's
// segment is sorted by one wave.
#pragma once

#include "collide_walk.hpp"  // col_cell, col_cell_id, DSL_COL_WALK_INDEXED

namespace dsl {

constexpr int kColScanPer = 8;                     // cells per lane and trip of k_index_scan
constexpr int kColScanTrip = kWave * kColScanPer;  // the count and start arrays are padded to a multiple of this

struct ColRange {
  int lo[3], hi[3];
};
__device__ __forceinline__ ColRange col_range(const TriBox& B, const ColIndex& ix) {
  ColRange r;
  for (int k = 0; k < 3; ++k) {
    r.lo[k] = col_cell(B.lo[k], ix.origin[k], ix.edge, ix.dims[k]);
    r.hi[k] = col_cell(B.hi[k], ix.origin[k], ix.edge, ix.dims[k]);
  }
  return r;
}
// kColBoundsWaves waves of one workgroup each: wave w takes triangles w * 64 + lane, + 64 * kColBoundsWaves, ...
__global__ __launch_bounds__(kWave) void k_index_bounds(int n_tri, const TriBox* __restrict__ box, ColBounds* __restrict__ out) {
  const float inf = __builtin_inff();
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  double ext = 0.0;
  int n_reg = 0;
  for (int t = blockIdx.x * kWave + threadIdx.x; t < n_tri; t += kWave * kColBoundsWaves) {
    const TriBox B = box[t];
    if (!B.regular) continue;
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(lo[k], B.lo[k]);
      hi[k] = fmaxf(hi[k], B.hi[k]);
    }
    ext += (double)(((B.hi[0] - B.lo[0]) + (B.hi[1] - B.lo[1])) + (B.hi[2] - B.lo[2])) / 3.0;
    ++n_reg;
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {  // (the same tree every time: the sum is deterministic)
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(lo[k], __shfl_xor(lo[k], off, kWave));
      hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off, kWave));
    }
    ext += __shfl_xor(ext, off, kWave);
    n_reg += __shfl_xor(n_reg, off, kWave);
  }
  if (threadIdx.x == 0) {
    ColBounds b;
    for (int k = 0; k < 3; ++k) {
      b.lo[k] = lo[k];
      b.hi[k] = hi[k];
    }
    b.ext = ext;
    b.n_reg = n_reg;
    b.pad_ = 0;
    out[blockIdx.x] = b;
  }
}

// the list entries an edge would cost: the sum over the regular triangles of the cells their boxes overlap
__global__ __launch_bounds__(kColChunk) void k_index_total(int n_tri, const TriBox* __restrict__ box, ColIndex ix,
                                                           unsigned long long* __restrict__ total) {
  const int t = blockIdx.x * kColChunk + threadIdx.x;
  if (t >= n_tri) return;
  const TriBox B = box[t];
  if (!B.regular) return;
  const ColRange r = col_range(B, ix);
  atomicAdd(total, (unsigned long long)(r.hi[0] - r.lo[0] + 1) * (unsigned long long)(r.hi[1] - r.lo[1] + 1) *
                       (unsigned long long)(r.hi[2] - r.lo[2] + 1));
}

// FILL = false: cnt[c] += 1 per overlapped cell.  FILL = true (cnt zeroed again, start scanned): the triangle takes the
// next free place of each cell's segment -- in whatever order the atomics fall; k_index_sort puts the segment in order.
template <bool FILL>
__global__ __launch_bounds__(kColChunk) void k_index_scatter(int n_tri, const TriBox* __restrict__ box, ColIndex ix,
                                                             int* __restrict__ cnt, int* __restrict__ list) {
  const int t = blockIdx.x * kColChunk + threadIdx.x;
  if (t >= n_tri) return;
  const TriBox B = box[t];
  if (!B.regular) return;
  const ColRange r = col_range(B, ix);
  for (int cz = r.lo[2]; cz <= r.hi[2]; ++cz)
    for (int cy = r.lo[1]; cy <= r.hi[1]; ++cy)
      for (int cx = r.lo[0]; cx <= r.hi[0]; ++cx) {
        const int c = col_cell_id(cx, cy, cz, ix);
        const int slot = atomicAdd(&cnt[c], 1);
        if constexpr (FILL) list[ix.start[c] + slot] = t;
      }
}

// One wave: start[c] = the sum of cnt[0 .. c) with every count rounded up to four entries; n_pad (a multiple of
// kColScanTrip, > cells; cnt is zero past the cells) entries of each array.  *total: the whole sum, which is start[cells].
__global__ __launch_bounds__(kWave) void k_index_scan(int n_pad, const int* __restrict__ cnt, int* __restrict__ start,
                                                      unsigned long long* __restrict__ total) {
  const int lane = threadIdx.x;
  unsigned long long carry = 0ull;
  for (int base = 0; base < n_pad; base += kColScanTrip) {
    const int c0 = base + lane * kColScanPer;
    int v[kColScanPer];
    unsigned int mine = 0u;
    for (int k = 0; k < kColScanPer; ++k) {
      v[k] = (cnt[c0 + k] + 3) & ~3;
      mine += (unsigned int)v[k];
    }
    unsigned int incl = mine;
    for (int off = 1; off < kWave; off <<= 1) {
      const unsigned int o = __shfl_up(incl, off, kWave);
      if (lane >= off) incl += o;
    }
    unsigned long long at = carry + (incl - mine);
    for (int k = 0; k < kColScanPer; ++k) {
      start[c0 + k] = (int)at;  // (the host refuses a total past 2^31 before anyone reads this)
      at += (unsigned int)v[k];
    }
    carry += __shfl(incl, kWave - 1, kWave);
  }
  if (lane == 0) *total = carry;
}

// One wave per cell: its segment's `cnt[c]` entries -- distinct triangle indices below 2^bits -- in ascending order.  A
// stable binary radix sort, least significant bit first, between the segment and the same place of `tmp`: per bit the
// wave counts the zeros, then deals the entries out by ballot and prefix count.  Linear in the segment's length.
__global__ __launch_bounds__(kColBlock) void k_index_sort(int cells, int bits, const int* __restrict__ cnt,
                                                          const int* __restrict__ start, int* list, int* tmp) {
  const int c = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kColBlock + threadIdx.x) / kWave));
  if (c >= cells) return;
  const int len = cnt[c];
  if (len < 2) return;
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned long long below = (1ull << lane) - 1ull;
  int* src = list + start[c];
  int* dst = tmp + start[c];
  const int trips = (len + kWave - 1) / kWave;
  for (int bit = 0; bit < bits; ++bit) {
    int zeros = 0;
    for (int k = 0; k < trips; ++k) {
      const int j = k * kWave + lane;
      const bool zero = j < len && ((src[j] >> bit) & 1) == 0;
      zeros += (int)__popcll(__ballot(zero));
    }
    int at0 = 0, at1 = zeros;
    for (int k = 0; k < trips; ++k) {
      const int j = k * kWave + lane;
      const bool valid = j < len;
      const int x = valid ? src[j] : 0;
      const bool one = valid && ((x >> bit) & 1) != 0, zero = valid && !one;
      const unsigned long long b0 = __ballot(zero), b1 = __ballot(one);
      if (zero) dst[at0 + (int)__popcll(b0 & below)] = x;
      if (one) dst[at1 + (int)__popcll(b1 & below)] = x;
      at0 += (int)__popcll(b0);
      at1 += (int)__popcll(b1);
    }
    __threadfence();  // the next pass reads what other lanes of this wave wrote
    int* s = src;
    src = dst;
    dst = s;
  }
  if (bits & 1)  // the sorted segment lies in tmp
    for (int j = lane; j < len; j += kWave) dst[j] = src[j];
}

// One wave: the irregular triangles, ascending.
__global__ __launch_bounds__(kWave) void k_index_always(int n_tri, const TriBox* __restrict__ box, int* __restrict__ always) {
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  int at = 0;
  for (int base = 0; base < n_tri; base += kWave) {
    const int t = base + lane;
    const bool irr = t < n_tri && box[t].regular == 0;
    const unsigned long long b = __ballot(irr);
    if (irr) always[at + (int)__popcll(b & below)] = t;
    at += (int)__popcll(b);
  }
}

// k_collide over the index.  One lane per particle slot; a lane that moves and lies inside the grid holds a cursor into
// its cell's list and a window of up to eight entries of it (two aligned 16-byte loads, the second in flight while the
// first is used), the wave a cursor into the always-list.  The next triangle is the minimum of the heads; lanes whose
// head it is advance; a lane that has hit drops out of the minimum; the wave ends when no head is left.
// ix.counters: [0] += the triangle records this wave loaded, [1] += 1 if it walked the whole list (a slow lane).
template <bool RESPOND>
__global__ __launch_bounds__(kColBlock) void k_collide_indexed(int n, float dt, Bnd bnd, ColMesh m, ColIndex ix, Soa3 p,
                                                            Soa3 v, ColQuery q, int* __restrict__ hits) {
  const int i = blockIdx.x * kColBlock + threadIdx.x;
  const bool live = i < n && !bnd.is(i);  // boundary particles are not queried
  float px = 0.f, py = 0.f, pz = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
  if (live) {
    px = p.x[i];
    py = p.y[i];
    pz = p.z[i];
    vx = v.x[i];
    vy = v.y[i];
    vz = v.z[i];
  }
  DSL_COL_WALK_INDEXED();
  col_finish<RESPOND>(i, live, dt, m.rest, hit, px, py, pz, vx, vy, vz, p, v, q, hits);
}

}  // namespace dsl
