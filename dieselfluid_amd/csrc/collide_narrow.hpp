// collide_narrow.hpp -- the collider's narrow phase and its epilogue, written once: Triangle.BarycentricCollision /
// Barycentric (geom/triangle/tri.go:37-101) for one particle against one triangle record, and what a lane does with
// its hit (the response, or the four query returns).  Included, through collide_walk.hpp, by every collide kernel's
// translation unit (kernels_collide.hpp: the list walk; kernels_collide_index.hpp: the walk over the cell index;
// collide_slab.hip: both on a slab rank), so that they cannot drift apart by a rounding.  The arithmetic's rules are stated at the head of kernels_collide.hpp.
#pragma once

#include "collide.hpp"

namespace dsl {

__device__ __forceinline__ float col_dot(float x0, float x1, float x2, float y0, float y1, float y2) {
  const float t0 = x0 * y0, t1 = x1 * y1, t2 = x2 * y2;
  return (t0 + t1) + t2;
}

__device__ __forceinline__ float wave_uniform(float v) {
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

// a lane's hit: the triangle (-1: none), k, the barycentric coordinates and the normal as supplied
struct ColHit {
  int tri = -1;
  float k = 0.f, u = 0.f, v = 0.f, w = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
};

// Does the particle (P, V) collide with triangle `t`, record R?  If so the hit is recorded and true returned.
__device__ __forceinline__ bool col_narrow(const TriRec& R, int t, float s_thr, float px, float py, float pz, float vx,
                                           float vy, float vz, ColHit& h) {
  float ndr = col_dot(R.n[0], R.n[1], R.n[2], vx, vy, vz);
  if (ndr == 0.0f) ndr = 0.0001f;
  const float d = col_dot(R.a[0] - px, R.a[1] - py, R.a[2] - pz, R.n[0], R.n[1], R.n[2]);
  const float k = d / ndr;
  const float sx = vx * k, sy = vy * k, sz = vz * k;
  const float p0x = px + sx, p0y = py + sy, p0z = pz + sz;
  const float qx = px - p0x, qy = py - p0y, qz = pz - p0z;
  const float s = col_dot(qx, qy, qz, qx, qy, qz);
  if (s <= s_thr) {  // dist <= r (false for NaN)
    const float wx = px - R.a[0], wy = py - R.a[1], wz = pz - R.a[2];
    const float d20 = col_dot(wx, wy, wz, R.e0[0], R.e0[1], R.e0[2]);
    const float d21 = col_dot(wx, wy, wz, R.e1[0], R.e1[1], R.e1[2]);
    const float a0 = R.d11 * d20, a1 = R.d01 * d21, b0 = R.d00 * d21, b1 = R.d01 * d20;
    const float bu = (a0 - a1) / R.denom;
    const float bv = (b0 - b1) / R.denom;
    const float bw = (1.0f - bv) - bu;
    const float bs = (bu + bv) + bw;
    if (bu <= 1.0f && bv <= 1.0f && bw <= 1.0f && bs <= 1.0f && bu >= 0.0f && bv >= 0.0f && bw >= 0.0f) {
      h.tri = t;  // the first triangle in list order wins (mesh.go:48-53)
      h.k = k;
      h.u = bu;
      h.v = bv;
      h.w = bw;
      h.nx = R.n[0];
      h.ny = R.n[1];
      h.nz = R.n[2];
      return true;
    }
  }
  return false;
}

// RESPOND = false: the query (writes `q`, leaves the particles alone).  RESPOND = true: the build-defined response -- a
// colliding particle with k >= 0 (the plane lies ahead along V) goes back to `point` and its velocity is reflected,
// v <- v - n ((1 + e) (v.n)); a receding one (k < 0) is left alone -- and `hits` counts the particles moved.
template <bool RESPOND>
__device__ __forceinline__ void col_finish(int i, bool live, float dt, float rest, const ColHit& h, float px, float py,
                                           float pz, float vx, float vy, float vz, Soa3 p, Soa3 v, ColQuery q,
                                           int* __restrict__ hits) {
  // point = P + V (-dt): the position rewound (tri.go:70)
  const float mdt = -dt;
  const float bx = px + vx * mdt, by = py + vy * mdt, bz = pz + vz * mdt;
  if constexpr (RESPOND) {
    const bool moved = h.tri >= 0 && h.k >= 0.0f;
    if (moved) {
      const float f = (1.0f + rest) * col_dot(vx, vy, vz, h.nx, h.ny, h.nz);
      p.x[i] = bx;
      p.y[i] = by;
      p.z[i] = bz;
      v.x[i] = vx - h.nx * f;
      v.y[i] = vy - h.ny * f;
      v.z[i] = vz - h.nz * f;
    }
    const unsigned long long mm = __ballot(moved);
    if (mm != 0ull && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(hits, (int)__popcll(mm));
  } else {
    if (live) {
      const size_t o = (size_t)q.ids[i];
      const bool hh = h.tri >= 0;
      if (q.tri) q.tri[o] = h.tri;
      if (q.normal) {
        q.normal[3 * o] = hh ? h.nx : 0.f;
        q.normal[3 * o + 1] = hh ? h.ny : 0.f;
        q.normal[3 * o + 2] = hh ? h.nz : 0.f;
      }
      if (q.coord) {
        q.coord[3 * o] = hh ? h.u : 0.f;
        q.coord[3 * o + 1] = hh ? h.v : 0.f;
        q.coord[3 * o + 2] = hh ? h.w : 0.f;
      }
      if (q.point) {
        q.point[3 * o] = hh ? bx : 0.f;
        q.point[3 * o + 1] = hh ? by : 0.f;
        q.point[3 * o + 2] = hh ? bz : 0.f;
      }
    }
  }
}

}  // namespace dsl
