// collide_walk.hpp -- the two walks of the triangle-mesh collider, written once: what one wave of 64 particle lanes does
// between loading its particles and the epilogue (collide_narrow.hpp, col_finish).  DSL_COL_WALK_LIST is the walk over
// the triangle list behind the broad phase's boxes (the soundness argument is at k_collide_prep, kernels_collide.hpp),
// DSL_COL_WALK_INDEXED the walk over the cell index (kernels_collide_index.hpp).  The single-domain kernels (k_collide,
// k_collide_indexed) and the slab kernels (collide_slab.hip) differ only in which lanes are `live` and where their
// particles come from; the walk, and with it every rounding and every choice of the first triangle, is this one.
//
// Why macros and not functions: the walks were lifted out of k_collide / k_collide_indexed, whose device code must stay
// what it was (tools/compare_device_asm.py).  As __forceinline__ functions -- arguments by value or by reference -- the
// same statements came out with another register allocation and another strength reduction of the record pointer; as
// text expanded in the kernel they compile to the very same body.  Each expands to statements that use the names of the
// enclosing kernel: `m` (ColMesh), `live`, `px .. vz` (zeros in a lane that is not live: its |V|^2 is 0, it never looks,
// never widens the wave's box, never makes the wave slow), for the indexed walk `ix` (ColIndex); each declares
// `ColHit hit`, the lane's result.
#pragma once

#include "collide_narrow.hpp"

namespace dsl {

__device__ __forceinline__ float wave_min(float v) {
  for (int off = kWave / 2; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, kWave));
  return wave_uniform(v);
}
__device__ __forceinline__ float wave_max(float v) {
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return wave_uniform(v);
}

// The list walk: chunks of kColChunk triangles, then the triangles of a chunk, each skipped if the wave's box misses
// its padded box; the record arrives through the scalar data cache (wave-uniform).  WMIN / WMAX: the wave-wide float
// minimum / maximum as a wave-uniform value -- wave_min / wave_max above in the single-domain kernel; any exact
// reduction gives the same box.
#define DSL_COL_WALK_LIST(WMIN, WMAX)                                                                          \
  /* Mag(V) == 0: no collision with any triangle (tri.go:39); the root of a float is zero only for zero */     \
  const float mv2 = col_dot(vx, vy, vz, vx, vy, vz);                                                           \
  bool todo = live && mv2 != 0.0f;                                                                             \
  /* the broad phase: this wave's particles' box; off in a wave with a slow lane (0 < |V| < 1e-4, or NaN) */   \
  const bool slow = todo && !(mv2 >= 1.0001e-8f);                                                              \
  const bool cull = m.cull != 0 && __ballot(slow) == 0ull;                                                     \
  float wlo[3] = {0.f, 0.f, 0.f}, whi[3] = {0.f, 0.f, 0.f};                                                    \
  if (cull) {                                                                                                  \
    const float inf = __builtin_inff();                                                                        \
    wlo[0] = WMIN(todo ? px : inf);                                                                            \
    wlo[1] = WMIN(todo ? py : inf);                                                                            \
    wlo[2] = WMIN(todo ? pz : inf);                                                                            \
    whi[0] = WMAX(todo ? px : -inf);                                                                           \
    whi[1] = WMAX(todo ? py : -inf);                                                                           \
    whi[2] = WMAX(todo ? pz : -inf);                                                                           \
  }                                                                                                            \
  auto skippable = [&](const TriBox& B) {                                                                      \
    return B.regular != 0 && (whi[0] < B.lo[0] || wlo[0] > B.hi[0] || whi[1] < B.lo[1] || wlo[1] > B.hi[1] ||  \
                              whi[2] < B.lo[2] || wlo[2] > B.hi[2]);                                           \
  };                                                                                                           \
  ColHit hit;                                                                                                  \
  for (int cb = 0; cb < m.n_tri; cb += kColChunk) {                                                            \
    if (__ballot(todo) == 0ull) break;  /* every lane has hit or stands still */                               \
    if (cull && skippable(m.chunk[cb / kColChunk])) continue;                                                  \
    const int ce = min(cb + kColChunk, m.n_tri);                                                               \
    for (int t = cb; t < ce; ++t) {                                                                            \
      if (__ballot(todo) == 0ull) break;                                                                       \
      if (cull && skippable(m.box[t])) continue;                                                               \
      const TriRec R = m.rec[t];  /* wave-uniform */                                                           \
      if (todo && col_narrow(R, t, m.s_thr, px, py, pz, vx, vy, vz, hit)) todo = false;                        \
    }                                                                                                          \
  }

// THE cell coordinate of the index, of a box corner and of a particle alike; monotone in x.  For origin <= x <= top.
__device__ __forceinline__ int col_cell(float x, float origin, float edge, int dim) {
  const float f = floorf((x - origin) / edge);
  return (int)fminf(fmaxf(f, 0.0f), (float)(dim - 1));
}
__device__ __forceinline__ int col_cell_id(int cx, int cy, int cz, const ColIndex& ix) {
  return (cz * ix.dims[1] + cy) * ix.dims[0] + cx;
}

// The wave-wide minimum as a scalar.  Every lane of the wave must be active (the callers' control flow is wave-uniform
// and a kernel's only early return takes whole workgroups).  Four steps inside each row of 16 lanes, the rows combined
// by the two row broadcasts, lane 63 holds the result.
__device__ __forceinline__ int wave_min_i32(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));   // quad_perm:[1,0,3,2]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));   // quad_perm:[2,3,0,1]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));  // row_mirror
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xA, 0xF, false));  // row_bcast:15 into rows 1 and 3
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xC, 0xF, false));  // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, kWave - 1);
}

// The walk over the cell index.  A lane that moves and lies inside the grid holds a cursor into its cell's list and a
// window of up to eight entries of it (two aligned 16-byte loads, the second in flight while the first is used), the
// wave a cursor into the always-list.  The next triangle is the minimum of the heads; lanes whose head it is advance; a
// lane that has hit drops out of the minimum; the wave ends when no head is left.  A wave with a slow lane walks the
// whole list.  ix.counters: [0] += the triangle records this wave loaded, [1] += 1 if it walked the whole list.
#define DSL_COL_WALK_INDEXED()                                                                                                     \
  const float mv2 = col_dot(vx, vy, vz, vx, vy, vz);                                                                               \
  bool todo = live && mv2 != 0.0f;  /* Mag(V) == 0: no collision with any triangle (tri.go:39) */                                  \
  const bool slow = todo && !(mv2 >= 1.0001e-8f);                                                                                  \
  const bool full = __ballot(slow) != 0ull;                                                                                        \
                                                                                                                                   \
  ColHit hit;                                                                                                                      \
  int visits = 0;                                                                                                                  \
  if (full) {                                                                                                                      \
    for (int t = 0; t < m.n_tri; ++t) {                                                                                            \
      if (__ballot(todo) == 0ull) break;                                                                                           \
      const TriRec R = m.rec[t];  /* wave-uniform */                                                                               \
      ++visits;                                                                                                                    \
      if (todo && col_narrow(R, t, m.s_thr, px, py, pz, vx, vy, vz, hit)) todo = false;                                            \
    }                                                                                                                              \
  } else {                                                                                                                         \
    int cur = 0, end = 0;                                                                                                          \
    if (todo && px >= ix.origin[0] && px <= ix.top[0] && py >= ix.origin[1] && py <= ix.top[1] && pz >= ix.origin[2] &&            \
        pz <= ix.top[2]) {                                                                                                         \
      const int c = col_cell_id(col_cell(px, ix.origin[0], ix.edge, ix.dims[0]), col_cell(py, ix.origin[1], ix.edge, ix.dims[1]),  \
                                col_cell(pz, ix.origin[2], ix.edge, ix.dims[2]), ix);                                              \
      cur = ix.start[c];                                                                                                           \
      end = ix.start[c + 1];                                                                                                       \
    }                                                                                                                              \
    const int4* __restrict__ list4 = reinterpret_cast<const int4*>(ix.list);                                                       \
    const int4 none4 = make_int4(kColNone, kColNone, kColNone, kColNone);                                                          \
    int4 w = none4, nw = none4;                                                                                                    \
    if (cur < end) {                                                                                                               \
      w = list4[cur >> 2];                                                                                                         \
      cur += 4;                                                                                                                    \
    }                                                                                                                              \
    if (cur < end) {                                                                                                               \
      nw = list4[cur >> 2];                                                                                                        \
      cur += 4;                                                                                                                    \
    }                                                                                                                              \
    int ai = 0;                                                                                                                    \
    int a = ix.n_always > 0 ? ix.always[0] : kColNone;  /* wave-uniform, like everything about the always-list */                  \
    for (;;) {                                                                                                                     \
      if (__ballot(todo) == 0ull) break;  /* every lane has hit or stands still: the always-list is nobody's business either */    \
      const int t = min(wave_min_i32(todo ? w.x : kColNone), a);  /* a scalar */                                                   \
      if (t == kColNone) break;                                                                                                    \
      if (t == a) {                                                                                                                \
        ++ai;                                                                                                                      \
        a = ai < ix.n_always ? ix.always[ai] : kColNone;                                                                           \
      }                                                                                                                            \
      const TriRec R = m.rec[t];  /* wave-uniform: one 16-dword scalar load */                                                     \
      ++visits;                                                                                                                    \
      if (todo && col_narrow(R, t, m.s_thr, px, py, pz, vx, vy, vz, hit)) todo = false;                                            \
      if (w.x == t) {                                                                                                              \
        w.x = w.y;                                                                                                                 \
        w.y = w.z;                                                                                                                 \
        w.z = w.w;                                                                                                                 \
        w.w = kColNone;                                                                                                            \
        if (w.x == kColNone) {  /* (the fill of a segment's last window: the list is at its end as well) */                        \
          w = nw;                                                                                                                  \
          nw = none4;                                                                                                              \
          if (cur < end) {                                                                                                         \
            nw = list4[cur >> 2];                                                                                                  \
            cur += 4;                                                                                                              \
          }                                                                                                                        \
        }                                                                                                                          \
      }                                                                                                                            \
    }                                                                                                                              \
  }                                                                                                                                \
  if ((threadIdx.x & (kWave - 1)) == 0) {                                                                                          \
    if (visits) atomicAdd(&ix.counters[0], (unsigned long long)visits);                                                            \
    if (full) atomicAdd(&ix.counters[1], 1ull);                                                                                    \
  }

}  // namespace dsl
