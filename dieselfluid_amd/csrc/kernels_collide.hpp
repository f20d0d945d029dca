// kernels_collide.hpp -- triangle-mesh colliders: geom.Collider as Mesh.Collision implements it (geom/mesh/mesh.go:41-57)
// through Triangle.BarycentricCollision / Barycentric (geom/triangle/tri.go:37-101), for every fluid particle at once.
//
// ONE arithmetic in both math modes: a collision is a classification, a last-bit difference flips it.  Every operation
// below is the reference's, IEEE float32, rounded once (the translation unit is compiled with -ffp-contract=off and `/` is
// the correctly rounded division); dot products are (x0 y0 + x1 y1) + x2 y2 (vector.go:268-276); Mag's float64 square
// root (vector.go:301-308) is replaced by its monotone inverse: `Mag(q) <= r` is `|q|^2 <= s_thr`, s_thr the largest
// float whose root, rounded to float32, is <= r (found once on the host).
//
// Layout: one lane per particle slot, a wave walks the triangle list in order.  The triangle record is the same for all
// 64 lanes at the same time, so it is wave-uniform data: the loop counter is uniform, the records are read through the
// scalar data cache into scalar registers (16 dwords per triangle) and cost no vector memory instruction, no LDS and no
// barrier ("colliders").  These kernels are compiled in a translation unit of their own (collide.hip);
// the host layer reaches them through the launchers of collide.hpp.
#pragma once

#include "collide_walk.hpp"  // DSL_COL_WALK_LIST, and through it collide_narrow.hpp: col_dot, col_narrow, col_finish

namespace dsl {

// Which triangles may the broad phase skip?  For a particle with |V| >= 1e-4 a hit needs |V k| <= r (up to rounding), and
// |V k| = |V| |d| / |n.V| >= |d| / |n| -- or, with n.V == 0 and the 0.0001 substitute, |V| |d| / 1e-4 >= |d|: the particle
// lies within r / |n| <= 2 r of the plane { (x - a).n = 0 }.  It also passes the barycentric test: its projection ALONG
// THE TRIANGLE'S OWN NORMAL lies in the triangle.  The two together confine it to the triangle's bounding box, inflated,
// only if n is (nearly) that normal -- the host supplies n unchecked -- and the barycentric solve is well conditioned.
// `regular` therefore asks for all of: 0.5 <= |n| <= 1.001; n within 1e-3 of perpendicular to both edges; the edges
// at more than 5.7 degrees to each other (denom >= 0.01 d00 d11).  Then the offset from the triangle is at most
// (2 r + 1e-3 (|e0| + |e1|)) / 0.999 along the normal, and the rounding of u, v (condition number <= 100: 1e-5 relative)
// moves the accepted region by less than 1e-4 of the triangle's extent; the pad below is 2.1 r + 1 % of the box's
// extents + 1e-5 of its largest coordinate.  Everything else -- a zero or oblique normal, a needle, a degenerate triangle, a
// non-finite value -- is never skipped.  A pad that is NaN (r NaN) fails every comparison: never skipped either.
__global__ __launch_bounds__(kColChunk) void k_collide_prep(int n_tri, const float* __restrict__ verts,
                                                            const float* __restrict__ normals, float r,
                                                            TriRec* __restrict__ rec, TriBox* __restrict__ box) {
  const int t = blockIdx.x * kColChunk + threadIdx.x;
  if (t >= n_tri) return;
  const float* q = verts + (size_t)9 * t;
  TriRec R;
  float b[3], c[3];
  for (int k = 0; k < 3; ++k) {
    R.a[k] = q[k];
    b[k] = q[3 + k];
    c[k] = q[6 + k];
    R.e0[k] = b[k] - R.a[k];
    R.e1[k] = c[k] - R.a[k];
    R.n[k] = normals[(size_t)3 * t + k];
  }
  R.d00 = col_dot(R.e0[0], R.e0[1], R.e0[2], R.e0[0], R.e0[1], R.e0[2]);
  R.d01 = col_dot(R.e0[0], R.e0[1], R.e0[2], R.e1[0], R.e1[1], R.e1[2]);
  R.d11 = col_dot(R.e1[0], R.e1[1], R.e1[2], R.e1[0], R.e1[1], R.e1[2]);
  const float p0 = R.d00 * R.d11, p1 = R.d01 * R.d01;
  R.denom = p0 - p1;
  rec[t] = R;

  TriBox B;
  float ext = 0.0f, big = 0.0f;
  for (int k = 0; k < 3; ++k) {
    B.lo[k] = fminf(R.a[k], fminf(b[k], c[k]));
    B.hi[k] = fmaxf(R.a[k], fmaxf(b[k], c[k]));
    ext += B.hi[k] - B.lo[k];
    big = fmaxf(big, fmaxf(fabsf(B.lo[k]), fabsf(B.hi[k])));
  }
  const float pad = 2.1f * r + 0.01f * ext + 1.0e-5f * big;
  for (int k = 0; k < 3; ++k) {
    B.lo[k] -= pad;
    B.hi[k] += pad;
  }
  const float n2 = col_dot(R.n[0], R.n[1], R.n[2], R.n[0], R.n[1], R.n[2]);
  const float ne0 = col_dot(R.n[0], R.n[1], R.n[2], R.e0[0], R.e0[1], R.e0[2]);
  const float ne1 = col_dot(R.n[0], R.n[1], R.n[2], R.e1[0], R.e1[1], R.e1[2]);
  bool reg = n2 >= 0.25f && n2 <= 1.002001f;
  reg = reg && R.d00 > 0.0f && R.d11 > 0.0f && R.denom >= 0.01f * p0 && p0 < 1.0e30f;
  reg = reg && ne0 * ne0 <= 1.0e-6f * (n2 * R.d00) && ne1 * ne1 <= 1.0e-6f * (n2 * R.d11);
  reg = reg && pad >= 0.0f && pad < 1.0e30f && big < 1.0e30f;  // (false for NaN)
  B.regular = reg ? 1 : 0;
  B.pad_ = 0;
  box[t] = B;
}

// one thread per chunk: the union of its triangles' boxes; regular only if every triangle is
__global__ __launch_bounds__(64) void k_collide_chunks(int n_tri, const TriBox* __restrict__ box, TriBox* __restrict__ chunk) {
  const int ch = blockIdx.x * 64 + threadIdx.x;
  const int t0 = ch * kColChunk;
  if (t0 >= n_tri) return;
  const int t1 = min(t0 + kColChunk, n_tri);
  TriBox U = box[t0];
  for (int t = t0 + 1; t < t1; ++t) {
    const TriBox B = box[t];
    for (int k = 0; k < 3; ++k) {
      U.lo[k] = fminf(U.lo[k], B.lo[k]);
      U.hi[k] = fmaxf(U.hi[k], B.hi[k]);
    }
    U.regular &= B.regular;
  }
  chunk[ch] = U;
}

// RESPOND: collide_narrow.hpp, col_finish.
template <bool RESPOND>
__global__ __launch_bounds__(kColBlock) void k_collide(int n, float dt, Bnd bnd, ColMesh m, Soa3 p, Soa3 v, ColQuery q,
                                                    int* __restrict__ hits) {
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
  DSL_COL_WALK_LIST(wave_min, wave_max);

  col_finish<RESPOND>(i, live, dt, m.rest, hit, px, py, pz, vx, vy, vz, p, v, q, hits);
}

}  // namespace dsl
