// sdf.hip -- implicit colliders: the signed distance volume of a triangle mesh on a voxel lattice (dsl_mesh_distance_volume)
// and the collision of the fluid particles with such a volume inside the step (dsl_collider_set_volume, the volume branch of
// dsl_collide_pass, dsl_collider_volume_query).  A translation unit of its own with its kernels and their host side; its
// kernel list is tests/golden/device_kernels_sdf.txt (the collider in rigid motion is sdf_rigid.hip, reached from the
// dispatches below).  Same flags as dslsph.hip: -ffp-contract=off keeps every operation at
// one rounding, `/` and sqrtf are the correctly rounded ones.  Both rules are build-defined (include/dslsph.h)
// and restated operation for operation in tests/sdf_ref.py; they are the same in DSL_MATH_EXACT and DSL_MATH_FAST.
//
//   k_sdf_prep          one lane per triangle: the record (a, ab, ac, b, c) and the box a voxel within `band` must lie in
//   k_sdf_brick_count   one lane per brick of 8 x 8 x 4 voxels: the triangles whose box reaches the brick's voxels
//   k_sdf_brick_fill    ... and, behind surface.hip's scan, their indices, ascending (no atomics: the lists are the same every time)
//   k_sdf_distance      one workgroup per brick, one lane per voxel: the brick's records through LDS in chunks of 256, a
//                       running min d^2; a brick with an empty list stores `band`
//   k_sdf_sweep         one lane per triangle: for every lattice row (j, k) of its projected box whose +x ray it claims, an
//                       integer mark at the last voxel in front of the crossing
//   k_sdf_sign          one wave per row: the suffix parity of the marks along x flips the sign of the voxels inside
//   k_collide_volume    one lane per particle slot: eight loads, the trilinear value and its analytic gradient, the response
#include "engine.hpp"
#include "sph_device.hpp"

#include <algorithm>
#include <cmath>

namespace dsl {

constexpr int kSdfBlock = 256;
constexpr int kSdfBX = 8, kSdfBY = 8, kSdfBZ = 4;
constexpr int kSdfChunk = 256;   // records per LDS chunk: 16 KiB
constexpr int kSdfCounters = 4;  // [0] bricks with a non-empty list, [1] triangle visits (pairs tested), [2] list entries

struct SdfLattice : Lattice {
  int nbx, nby, nbz;  // bricks of 8 x 8 x 4 voxels per axis
};
// a, ab = b - a, ac = c - a, b, c: what the seven regions and the sweep need, the same whether computed once or per voxel
struct alignas(16) SdfRec {
  float a[3], ab[3], ac[3], b[3], c[3], pad_;
};
static_assert(sizeof(SdfRec) == 64, "four float4 per record");
struct SdfBox {
  float lo[3], hi[3];
};
struct ColVol {
  const float* vol;
  Lattice g;
  float radius, rest;
};

namespace {
// how many of the axis' n coordinates are < v (STRICT) or <= v: the coordinate is monotone in the index, so a bisection on
// the real coordinates decides it exactly, whatever the rounding of origin + step * idx.  0 for a NaN.
template <bool STRICT>
__device__ __forceinline__ int sdf_count_below(float o, float s, int n, float v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    const float x = lattice_coord(o, s, mid);
    if (STRICT ? x < v : x <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Squared distance to the closest point of the triangle: the seven regions on d1..d6, vertex regions first, then the edges,
// then the face (tests/sdf_ref.py: tri_dist2, operation for operation).  NaN where the branch taken divides zero by zero.
__device__ __forceinline__ float sdf_dist2(float px, float py, float pz, const float4 r0, const float4 r1, const float4 r2,
                                           const float4 r3) {
  const float ax = r0.x, ay = r0.y, az = r0.z, abx = r0.w, aby = r1.x, abz = r1.y, acx = r1.z, acy = r1.w, acz = r2.x;
  const float bx = r2.y, by = r2.z, bz = r2.w, cx = r3.x, cy = r3.y, cz = r3.z;
  float qx = ax, qy = ay, qz = az;
  const float d1 = dot3(abx, aby, abz, px - ax, py - ay, pz - az);
  const float d2 = dot3(acx, acy, acz, px - ax, py - ay, pz - az);
  if (!(d1 <= 0.f && d2 <= 0.f)) {
    const float d3 = dot3(abx, aby, abz, px - bx, py - by, pz - bz);
    const float d4 = dot3(acx, acy, acz, px - bx, py - by, pz - bz);
    if (d3 >= 0.f && d4 <= d3) {
      qx = bx, qy = by, qz = bz;
    } else {
      const float d5 = dot3(abx, aby, abz, px - cx, py - cy, pz - cz);
      const float d6 = dot3(acx, acy, acz, px - cx, py - cy, pz - cz);
      const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
      const float e1 = d4 - d3, e2 = d5 - d6;
      if (d6 >= 0.f && d5 <= d6) {
        qx = cx, qy = cy, qz = cz;
      } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        const float t = d1 / (d1 - d3);
        qx = ax + abx * t, qy = ay + aby * t, qz = az + abz * t;
      } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
        const float t = d2 / (d2 - d6);
        qx = ax + acx * t, qy = ay + acy * t, qz = az + acz * t;
      } else if (va <= 0.f && e1 >= 0.f && e2 >= 0.f) {
        const float t = e1 / (e1 + e2);
        qx = bx + (cx - bx) * t, qy = by + (cy - by) * t, qz = bz + (cz - bz) * t;
      } else {
        const float s = (va + vb) + vc;
        const float v = vb / s, w = vc / s;
        qx = (ax + abx * v) + acx * w, qy = (ay + aby * v) + acy * w, qz = (az + abz * v) + acz * w;
      }
    }
  }
  const float ex = px - qx, ey = py - qy, ez = pz - qz;
  return dot3(ex, ey, ez, ex, ey, ez);
}
}  // namespace

// Which triangles may a brick skip?  One whose distance to every voxel of the brick, AS COMPUTED, exceeds `band`: such a
// triangle cannot change min(sqrt(min d2), band).  The vertex and edge branches return the distance to a point of the
// triangle itself (t in [0, 1] by the branch conditions, the division being monotone) up to the rounding of p - q, a few
// ulp of the largest coordinate.  The face branch returns the distance to a point of the triangle's PLANE; it is taken
// when the projection of p lies in the triangle up to the error eta of the barycentric coordinates, so the true distance
// is at most sqrt(d^2 + (eta L)^2).  For a REGULAR triangle -- |ab x ac|^2 >= 1e-4 |ab|^2 |ac|^2, everything finite -- eta L
// is below 1e-3 of the distance.  So a voxel whose computed distance is <= band lies within 1.001 band + rounding of the
// triangle, hence of its bounding box; the pad is 1.01 band + 1 % of the box's extents + 1e-5 of its largest coordinate.
// Everything else -- a needle, a degenerate triangle, a non-finite value -- is never skipped (an infinite box).  With
// band = +inf the pad is infinite: every brick lists every triangle.
__global__ __launch_bounds__(kSdfBlock) void k_sdf_prep(int n_tri, const float* __restrict__ verts, float band,
                                                        SdfRec* __restrict__ rec, SdfBox* __restrict__ box) {
  const int t = blockIdx.x * kSdfBlock + threadIdx.x;
  if (t >= n_tri) return;
  const float* q = verts + (size_t)9 * t;
  SdfRec R;
  SdfBox B;
  float ext = 0.f, big = 0.f;
  for (int k = 0; k < 3; ++k) {
    R.a[k] = q[k];
    R.b[k] = q[3 + k];
    R.c[k] = q[6 + k];
    R.ab[k] = R.b[k] - R.a[k];
    R.ac[k] = R.c[k] - R.a[k];
    B.lo[k] = fminf(R.a[k], fminf(R.b[k], R.c[k]));
    B.hi[k] = fmaxf(R.a[k], fmaxf(R.b[k], R.c[k]));
    ext += B.hi[k] - B.lo[k];
    big = fmaxf(big, fmaxf(fabsf(B.lo[k]), fabsf(B.hi[k])));
  }
  R.pad_ = 0.f;
  rec[t] = R;
  const float d00 = dot3(R.ab[0], R.ab[1], R.ab[2], R.ab[0], R.ab[1], R.ab[2]);
  const float d01 = dot3(R.ab[0], R.ab[1], R.ab[2], R.ac[0], R.ac[1], R.ac[2]);
  const float d11 = dot3(R.ac[0], R.ac[1], R.ac[2], R.ac[0], R.ac[1], R.ac[2]);
  const float p0 = d00 * d11, denom = p0 - d01 * d01;
  const float pad = 1.01f * band + 0.01f * ext + 1.0e-5f * big;
  bool reg = d00 > 0.f && d11 > 0.f && p0 < 1.0e30f && denom >= 1.0e-4f * p0;
  reg = reg && pad >= 0.f && pad < 1.0e30f && big < 1.0e30f;  // (false for NaN and for band = +inf)
  for (int k = 0; k < 3; ++k) {
    B.lo[k] = reg ? B.lo[k] - pad : -INFINITY;
    B.hi[k] = reg ? B.hi[k] + pad : INFINITY;
  }
  box[t] = B;
}

namespace {
// the brick's voxels span [lo, hi] per axis: coordinates are monotone in the index, so the first and the last voxel bound them
struct SdfBrick {
  float lo[3], hi[3];
  int nvox;
};
__device__ __forceinline__ SdfBrick sdf_brick(const SdfLattice& g, int b) {
  const int bi = b % g.nbx, bjk = b / g.nbx;
  const int first[3] = {bi * kSdfBX, (bjk % g.nby) * kSdfBY, (bjk / g.nby) * kSdfBZ};
  const int edge[3] = {kSdfBX, kSdfBY, kSdfBZ};
  SdfBrick K;
  K.nvox = 1;
  for (int a = 0; a < 3; ++a) {
    const int last = min(first[a] + edge[a], g.n[a]) - 1;
    K.lo[a] = lattice_coord(g.o[a], g.s[a], first[a]);
    K.hi[a] = lattice_coord(g.o[a], g.s[a], last);
    K.nvox *= last - first[a] + 1;
  }
  return K;
}
__device__ __forceinline__ bool sdf_reaches(const SdfBox& B, const SdfBrick& K) {
  return B.lo[0] <= K.hi[0] && B.hi[0] >= K.lo[0] && B.lo[1] <= K.hi[1] && B.hi[1] >= K.lo[1] && B.lo[2] <= K.hi[2] &&
         B.hi[2] >= K.lo[2];
}
}  // namespace

// (all lanes of a wave read the same box at the same time: one broadcast load per triangle and wave)
__global__ __launch_bounds__(kSdfBlock) void k_sdf_brick_count(int n_tri, const SdfBox* __restrict__ box, SdfLattice g, int nb,
                                                               unsigned long long* __restrict__ counts,
                                                               unsigned long long* __restrict__ ctr) {
  const int b = blockIdx.x * kSdfBlock + threadIdx.x;
  if (b >= nb) return;
  const SdfBrick K = sdf_brick(g, b);
  unsigned long long cnt = 0;
  for (int t = 0; t < n_tri; ++t) cnt += sdf_reaches(box[t], K) ? 1ull : 0ull;
  counts[b] = cnt;
  if (cnt != 0ull) {
    atomicAdd(&ctr[0], 1ull);
    atomicAdd(&ctr[1], cnt * (unsigned long long)K.nvox);
  }
}

__global__ __launch_bounds__(kSdfBlock) void k_sdf_brick_fill(int n_tri, const SdfBox* __restrict__ box, SdfLattice g, int nb,
                                                              const unsigned long long* __restrict__ offsets,
                                                              int* __restrict__ list) {
  const int b = blockIdx.x * kSdfBlock + threadIdx.x;
  if (b >= nb) return;
  const SdfBrick K = sdf_brick(g, b);
  size_t at = (size_t)offsets[b];
  for (int t = 0; t < n_tri; ++t)
    if (sdf_reaches(box[t], K)) list[at++] = t;
}

__global__ __launch_bounds__(kSdfBlock) void k_sdf_distance(const float4* __restrict__ rec, SdfLattice g, int nb,
                                                            const unsigned long long* __restrict__ offsets,
                                                            const unsigned long long* __restrict__ ctr,
                                                            const int* __restrict__ list, float band, float* __restrict__ out) {
  __shared__ float4 s_rec[kSdfChunk * 4];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int bi = b % g.nbx, bjk = b / g.nbx;
  const int vi = bi * kSdfBX + (tid & 7), vj = (bjk % g.nby) * kSdfBY + ((tid >> 3) & 7), vk = (bjk / g.nby) * kSdfBZ + (tid >> 6);
  const bool mine = vi < g.n[0] && vj < g.n[1] && vk < g.n[2];  // (the bricks of the upper faces overhang)
  const size_t at = ((size_t)vk * g.n[1] + vj) * g.n[0] + vi;
  const unsigned long long first = offsets[b], end = b + 1 < nb ? offsets[b + 1] : ctr[2];  // (uniform)
  if (first == end) {
    if (mine) out[at] = band;
    return;
  }
  const float px = lattice_coord(g.o[0], g.s[0], vi), py = lattice_coord(g.o[1], g.s[1], vj), pz = lattice_coord(g.o[2], g.s[2], vk);
  float best = INFINITY;
  for (unsigned long long base = first; base < end; base += kSdfChunk) {
    const int m = (int)min((unsigned long long)kSdfChunk, end - base);
    if (tid < m) {
      const float4* src = rec + (size_t)4 * list[base + tid];
      s_rec[4 * tid] = src[0];
      s_rec[4 * tid + 1] = src[1];
      s_rec[4 * tid + 2] = src[2];
      s_rec[4 * tid + 3] = src[3];
    }
    lds_barrier();
    for (int r = 0; r < m; ++r) {
      const float d2 = sdf_dist2(px, py, pz, s_rec[4 * r], s_rec[4 * r + 1], s_rec[4 * r + 2], s_rec[4 * r + 3]);
      if (d2 < best) best = d2;  // (NaN and +inf never win)
    }
    lds_barrier();  // (the next chunk overwrites the image)
  }
  if (mine) out[at] = fminf(sqrtf(best), band);
}

// The sign rule (include/dslsph.h): projected onto (y, z), a row's ray belongs to the triangle when the row lies on the
// inner side of all three edges, a row exactly on an edge being shifted by one infinitesimal amount for the whole mesh.
__global__ __launch_bounds__(kSdfBlock) void k_sdf_sweep(int n_tri, const SdfRec* __restrict__ rec, SdfLattice g,
                                                         unsigned int* __restrict__ marks) {
  const int t = blockIdx.x * kSdfBlock + threadIdx.x;
  if (t >= n_tri) return;
  const SdfRec R = rec[t];
  // per edge: lo (y, z), delta (y, z), whether the opposite vertex is on the positive side
  float ly0, lz0, dy0, dz0, ly1, lz1, dy1, dz1, ly2, lz2, dy2, dz2;
  bool pos0, pos1, pos2, ok = true;
  auto edge = [&](float p0y, float p0z, float p1y, float p1z, float ry, float rz, float& ly, float& lz, float& dy, float& dz,
                  bool& pos) {
    const bool swap = p1y < p0y || (p1y == p0y && p1z < p0z);
    ly = swap ? p1y : p0y;
    lz = swap ? p1z : p0z;
    const float hy = swap ? p0y : p1y, hz = swap ? p0z : p1z;
    dy = hy - ly;
    dz = hz - lz;
    if (dy == 0.f && dz == 0.f) ok = false;
    const float er = dy * (rz - lz) - dz * (ry - ly);
    if (!(er > 0.f || er < 0.f)) ok = false;
    pos = er > 0.f;
  };
  edge(R.a[1], R.a[2], R.b[1], R.b[2], R.c[1], R.c[2], ly0, lz0, dy0, dz0, pos0);
  edge(R.b[1], R.b[2], R.c[1], R.c[2], R.a[1], R.a[2], ly1, lz1, dy1, dz1, pos1);
  edge(R.c[1], R.c[2], R.a[1], R.a[2], R.b[1], R.b[2], ly2, lz2, dy2, dz2, pos2);
  if (!ok) return;
  const float ymin = fminf(R.a[1], fminf(R.b[1], R.c[1])), ymax = fmaxf(R.a[1], fmaxf(R.b[1], R.c[1]));
  const float zmin = fminf(R.a[2], fminf(R.b[2], R.c[2])), zmax = fmaxf(R.a[2], fmaxf(R.b[2], R.c[2]));
  // the rows with ymin <= y_j <= ymax and zmin <= z_k <= zmax, exactly
  const int j0 = sdf_count_below<true>(g.o[1], g.s[1], g.n[1], ymin), j1 = sdf_count_below<false>(g.o[1], g.s[1], g.n[1], ymax);
  const int k0 = sdf_count_below<true>(g.o[2], g.s[2], g.n[2], zmin), k1 = sdf_count_below<false>(g.o[2], g.s[2], g.n[2], zmax);
  const float nx = R.ab[1] * R.ac[2] - R.ab[2] * R.ac[1];
  const float ny = R.ab[2] * R.ac[0] - R.ab[0] * R.ac[2];
  const float nz = R.ab[0] * R.ac[1] - R.ab[1] * R.ac[0];
  auto claims = [](float ev, float dz, bool pos) {
    return pos ? (ev > 0.f || (ev == 0.f && dz <= 0.f)) : (ev < 0.f || (ev == 0.f && dz > 0.f));
  };
  for (int k = k0; k < k1; ++k) {
    const float z = lattice_coord(g.o[2], g.s[2], k);
    for (int j = j0; j < j1; ++j) {
      const float y = lattice_coord(g.o[1], g.s[1], j);
      if (!claims(dy0 * (z - lz0) - dz0 * (y - ly0), dz0, pos0)) continue;
      if (!claims(dy1 * (z - lz1) - dz1 * (y - ly1), dz1, pos1)) continue;
      if (!claims(dy2 * (z - lz2) - dz2 * (y - ly2), dz2, pos2)) continue;
      const float x_hit = R.a[0] - (ny * (y - R.a[1]) + nz * (z - R.a[2])) / nx;
      const int i_hit = sdf_count_below<true>(g.o[0], g.s[0], g.n[0], x_hit);  // voxels of the row with x_i < x_hit
      if (i_hit > 0) atomicAdd(&marks[((size_t)k * g.n[1] + j) * g.n[0] + (i_hit - 1)], 1u);
    }
  }
}

// voxel i is inside when an odd number of marks lies at or behind it in its row
__global__ __launch_bounds__(kSdfBlock) void k_sdf_sign(SdfLattice g, int nrows, const unsigned int* __restrict__ marks,
                                                        float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int row = blockIdx.x * (kSdfBlock / kWave) + threadIdx.x / kWave;
  if (row >= nrows) return;  // (wave-uniform)
  const size_t base = (size_t)row * g.n[0];
  int carry = 0;
  for (int top = ((g.n[0] - 1) / kWave) * kWave; top >= 0; top -= kWave) {
    const int i = top + lane;
    const bool in = i < g.n[0];
    const unsigned long long mask = __ballot(in && (marks[in ? base + i : base] & 1u) != 0u);
    const int par = (__popcll(mask >> lane) + carry) & 1;
    if (in && par) out[base + i] = -out[base + i];
    carry = (carry + __popcll(mask)) & 1;
  }
}

// The collide pass against a volume (include/dslsph.h; tests/sdf_ref.py: collider_eval).  RESPOND = false: the query, d and
// n = g / |g| in host order.
template <bool RESPOND>
__global__ __launch_bounds__(kSdfBlock) void k_collide_volume(int n, Bnd bnd, ColVol m, Soa3 p, Soa3 v, float* __restrict__ qdist,
                                                              float* __restrict__ qnormal, const int* __restrict__ ids,
                                                              int* __restrict__ hits) {
  const int s = blockIdx.x * kSdfBlock + threadIdx.x;
  const bool live = s < n && !bnd.is(s);  // boundary particles are not touched
  bool moved = false;
  if (live) {
    const float px = p.x[s], py = p.y[s], pz = p.z[s];
    const CellEval e = volume_cell_eval(m.g, m.vol, px, py, pz);
    const bool cell = e.cell, has_n = cell && e.mag > 0.f;
    const float d = e.d, nx_ = e.gx / e.mag, ny_ = e.gy / e.mag, nz_ = e.gz / e.mag;
    if constexpr (RESPOND) {
      moved = has_n && d < m.radius;
      if (moved) {
        const float pen = m.radius - d;
        p.x[s] = px + pen * nx_;
        p.y[s] = py + pen * ny_;
        p.z[s] = pz + pen * nz_;
        const float vx = v.x[s], vy = v.y[s], vz = v.z[s];
        const float vn = dot3(vx, vy, vz, nx_, ny_, nz_);
        if (vn < 0.f) {
          const float f = (1.0f + m.rest) * vn;
          v.x[s] = vx - f * nx_;
          v.y[s] = vy - f * ny_;
          v.z[s] = vz - f * nz_;
        }
      }
    } else {
      const size_t o = (size_t)ids[s];
      if (qdist) qdist[o] = cell ? d : 0.f;
      if (qnormal) {
        qnormal[3 * o] = has_n ? nx_ : 0.f;
        qnormal[3 * o + 1] = has_n ? ny_ : 0.f;
        qnormal[3 * o + 2] = has_n ? nz_ : 0.f;
      }
    }
  }
  if constexpr (RESPOND) {
    const unsigned long long mm = __ballot(moved);
    if (mm != 0ull && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(hits, (int)__popcll(mm));
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
namespace {
ColVol col_vol(const dsl_handle* h) { return ColVol{h->colv_vol.p, h->colv_g, h->colv_radius, h->colv_rest}; }
}  // namespace

int sdf_option(dsl_handle* h, int option, double* value) {
  *value = 0.0;
  if (option == DSL_OPT_COLLIDER_VOLUME) {
    *value = h->colv_on ? (double)h->colv_g.n[0] * h->colv_g.n[1] * h->colv_g.n[2] : 0.0;
    return DSL_OK;
  }
  if (option == DSL_OPT_COLLIDER_VOLUME_MOVING) {
    *value = h->colv_moving ? 1.0 : 0.0;
    return DSL_OK;
  }
  if (option == DSL_OPT_SDF_ACTIVE_BRICKS || option == DSL_OPT_SDF_VISITS) {
    unsigned long long ctr[kSdfCounters] = {};
    if (h->sdf_ctr) {
      HIP_TRY(h, hipMemcpyAsync(ctr, h->sdf_ctr, sizeof(ctr), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    *value = (double)ctr[option == DSL_OPT_SDF_ACTIVE_BRICKS ? 0 : 1];
    return DSL_OK;
  }
  // the last call's phases, from device events of their own (recorded while dsl_timing_enable(1) holds)
  return h->sdf_clock.ms(h, option == DSL_OPT_SDF_DISTANCE_MS ? 0 : 1, value);
}

void sdf_free(dsl_handle* h) {
  release(h->sdf_stage);
  release(h->sdf_verts);
  release(h->sdf_rec);
  release(h->sdf_box);
  release(h->sdf_scan);
  (void)hipFree(h->sdf_ctr);
  release(h->sdf_list);
  release(h->sdf_marks);
  release(h->colv_vol);
  (void)hipFree(h->colv_query);
  sdf_rigid_free(h);
  bodies_free(h);
  h->sdf_clock.destroy();
}

// The volume branch of the collide pass: in place on the current state.  dsl_stats.max_vel / max_f stay what Update saw.
int collide_volume_pass(dsl_handle* h) {
  if (h->colv_moving) return collide_volume_rigid_pass(h);  // (sdf_rigid.hip)
  HIP_TRY(h, hipMemsetAsync(h->col_hits, 0, sizeof(int), h->stream));
  const int rc = timed(h, DSL_K_COLLIDE, [&] {
    hipLaunchKernelGGL(k_collide_volume<true>, dim3((unsigned)((h->n + kSdfBlock - 1) / kSdfBlock)), dim3(kSdfBlock), 0, h->stream,
                       h->n, bnd_of(h), col_vol(h), mpos(h, h->cur_pv), mvel(h, h->cur_pv), (float*)nullptr, (float*)nullptr,
                       (const int*)nullptr, h->col_hits);
  });
  if (rc) return rc;
  h->grid_valid = false;  // positions moved
  h->masks_valid = false;
  return DSL_OK;
}

}  // namespace dsl

using namespace dsl;

int dsl_mesh_distance_volume(dsl_handle* h, const float* vertices, size_t n_triangles, const float origin[3], const float step[3],
                             const int32_t dims[3], float band, int flags, float* dev_out, float* host_out) {
  CHECK_HANDLE_ONLY(h);  // (no particle state is read: a live skin episode stays live, a slab handle is as good as any)
  const std::string w = "dsl_mesh_distance_volume";
  // every refusal comes before anything is touched
  if (!vertices || n_triangles == 0) return fail(h, DSL_ERR_INVALID, w + ": vertices must not be NULL and n_triangles must be > 0");
  if (n_triangles > ((size_t)1 << 24)) return fail(h, DSL_ERR_INVALID, w + ": more than 2^24 triangles");
  SdfLattice g;
  long long nvox = 0;
  if (int rc = lattice_check(h, w, origin, step, dims, 1, &g, &nvox)) return rc;
  if (!(band > 0.0f)) return fail(h, DSL_ERR_INVALID, w + ": band must be > 0 (+inf is allowed)");
  if (flags & ~DSL_SDF_UNSIGNED) return fail(h, DSL_ERR_INVALID, w + ": unknown bits in flags");
  if (!dev_out && !host_out) return fail(h, DSL_ERR_INVALID, w + ": dev_out and host_out are both NULL");
  g.nbx = (g.n[0] + kSdfBX - 1) / kSdfBX;
  g.nby = (g.n[1] + kSdfBY - 1) / kSdfBY;
  g.nbz = (g.n[2] + kSdfBZ - 1) / kSdfBZ;
  // (at most 2^30 voxels, and a brick holds at least 4 of them whatever the shape: at most 2^28 bricks)
  const int nb = (int)((long long)g.nbx * g.nby * g.nbz);
  const int T = (int)n_triangles;

  float* out = dev_out;
  if (!out) {
    if (int rc = reserve(h, h->sdf_stage, (size_t)nvox, "dsl_mesh_distance_volume: the staging array")) return rc;
    out = h->sdf_stage.p;
  }
  std::vector<long long> len;
  std::vector<size_t> first;
  const size_t scan_all = surf_scan_layout(nb, &len, &first);
  if (int rc = reserve(h, h->sdf_verts, (size_t)9 * T, "dsl_mesh_distance_volume: the vertex array")) return rc;
  if (int rc = reserve(h, h->sdf_rec, (size_t)4 * T, "dsl_mesh_distance_volume: the triangle records")) return rc;
  if (int rc = reserve(h, h->sdf_box, (size_t)6 * T, "dsl_mesh_distance_volume: the triangle boxes")) return rc;
  if (int rc = reserve(h, h->sdf_scan, scan_all, "dsl_mesh_distance_volume: the scan array")) return rc;
  if (!h->sdf_ctr)
    if (int rc = dev_alloc(h, &h->sdf_ctr, kSdfCounters)) return rc;
  SdfRec* rec = reinterpret_cast<SdfRec*>(h->sdf_rec.p);
  SdfBox* box = reinterpret_cast<SdfBox*>(h->sdf_box.p);
  const dim3 block(kSdfBlock);
  const dim3 tri_grid((unsigned)((T + kSdfBlock - 1) / kSdfBlock)), brick_grid((unsigned)((nb + kSdfBlock - 1) / kSdfBlock));

  h->sdf_clock.reset();
  HIP_TRY(h, hipMemcpyAsync(h->sdf_verts.p, vertices, (size_t)9 * T * sizeof(float), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemsetAsync(h->sdf_ctr, 0, kSdfCounters * sizeof(unsigned long long), h->stream));
  int rc = timed(h, DSL_K_SDF, [&] { hipLaunchKernelGGL(k_sdf_prep, tri_grid, block, 0, h->stream, T, h->sdf_verts.p, band, rec, box); });
  if (rc) return rc;
  rc = timed(h, DSL_K_SDF, [&] {
    hipLaunchKernelGGL(k_sdf_brick_count, brick_grid, block, 0, h->stream, T, box, g, nb, h->sdf_scan.p, h->sdf_ctr);
  });
  if (rc) return rc;
  if ((rc = surf_scan_run(h, DSL_K_SDF, h->sdf_scan.p, len, first, h->sdf_ctr + 2, nullptr))) return rc;
  // the lists' length decides their allocation: one blocking read (it also ends the use of `vertices`)
  unsigned long long ctr[kSdfCounters] = {};
  HIP_TRY(h, hipMemcpyAsync(ctr, h->sdf_ctr, sizeof(ctr), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (int rc2 = reserve(h, h->sdf_list, (size_t)std::max<unsigned long long>(ctr[2], 1), "dsl_mesh_distance_volume: the brick lists"))
    return rc2;
  rc = timed(h, DSL_K_SDF, [&] {
    hipLaunchKernelGGL(k_sdf_brick_fill, brick_grid, block, 0, h->stream, T, box, g, nb, h->sdf_scan.p, h->sdf_list.p);
  });
  if (rc) return rc;
  h->sdf_clock.begin(h, 0);
  rc = timed(h, DSL_K_SDF, [&] {
    hipLaunchKernelGGL(k_sdf_distance, dim3((unsigned)nb), block, 0, h->stream, reinterpret_cast<const float4*>(h->sdf_rec.p), g, nb,
                       h->sdf_scan.p, h->sdf_ctr, h->sdf_list.p, band, out);
  });
  if (rc) return rc;
  h->sdf_clock.end(h, 0);
  if (!(flags & DSL_SDF_UNSIGNED)) {
    if (int rc2 = reserve(h, h->sdf_marks, (size_t)nvox, "dsl_mesh_distance_volume: the marks")) return rc2;
    HIP_TRY(h, hipMemsetAsync(h->sdf_marks.p, 0, (size_t)nvox * sizeof(unsigned int), h->stream));
    h->sdf_clock.begin(h, 1);
    rc = timed(h, DSL_K_SDF, [&] { hipLaunchKernelGGL(k_sdf_sweep, tri_grid, block, 0, h->stream, T, rec, g, h->sdf_marks.p); });
    if (rc) return rc;
    const int nrows = (int)(nvox / g.n[0]), per = kSdfBlock / kWave;
    rc = timed(h, DSL_K_SDF, [&] {
      hipLaunchKernelGGL(k_sdf_sign, dim3((unsigned)((nrows + per - 1) / per)), block, 0, h->stream, g, nrows, h->sdf_marks.p, out);
    });
    if (rc) return rc;
    h->sdf_clock.end(h, 1);
  }
  if (host_out) {
    HIP_TRY(h, hipMemcpyAsync(host_out, out, (size_t)nvox * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  return DSL_OK;
}

int dsl_collider_set_volume(dsl_handle* h, const float* dev_volume, const float* host_volume, const float origin[3],
                            const float step[3], const int32_t dims[3], float radius, float restitution, int flags) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_collider_set_volume";
  if (h->c.slab_axis >= 0 || h->c.n_ptr) return fail(h, DSL_ERR_UNSUPPORTED, w + ": a volume collider is not supported in slab mode");
  if (!dims) {  // removes the collider (the copy stays for the next one)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->colv_on = false;
    return collide_volume_rigid_reset(h);
  }
  if (h->n_bodies > 0)
    return fail(h, DSL_ERR_INVALID, w + ": rigid bodies exist, and a mesh collider, a volume collider and rigid bodies exclude each "
                                        "other; remove the bodies first (dsl_bodies_clear)");
  if (h->col_tri > 0)
    return fail(h, DSL_ERR_INVALID, w + ": a mesh collider is set, and a mesh collider and a volume collider exclude each other; "
                                        "remove the mesh first (dsl_collider_set_mesh with n_triangles = 0)");
  if ((dev_volume != nullptr) == (host_volume != nullptr)) return fail(h, DSL_ERR_INVALID, w + ": exactly one of dev_volume and host_volume must be given");
  if (!origin || !step) return fail(h, DSL_ERR_INVALID, w + ": origin and step must not be NULL");
  Lattice g;  // (the handle keeps the old lattice until the new collider is whole)
  long long nvox = 0;
  if (int rc = lattice_check(h, w, origin, step, dims, 2, &g, &nvox)) return rc;
  if (flags & ~DSL_SDF_UNSIGNED) return fail(h, DSL_ERR_INVALID, w + ": unknown bits in flags");
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (a pass in flight may still read the volume that is replaced)
  h->colv_on = false;  // no collider until the new one is whole
  if (int rc = collide_volume_rigid_reset(h)) return rc;  // ... and a new volume starts at rest, with nothing handed over
  if (int rc = reserve(h, h->colv_vol, (size_t)nvox, "dsl_collider_set_volume: the volume")) return rc;
  if (!h->col_hits)
    if (int rc = dev_alloc(h, &h->col_hits, 1)) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->colv_vol.p, dev_volume ? dev_volume : host_volume, (size_t)nvox * sizeof(float),
                            dev_volume ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the caller's array is never retained after the call returns)
  h->colv_g = g;
  h->colv_radius = radius;
  h->colv_rest = restitution;
  h->colv_flags = flags;
  h->colv_on = true;
  return DSL_OK;
}

int dsl_collider_volume_query(dsl_handle* h, float* dist, float* normal) {
  CHECK_HANDLE(h);
  if (h->c.n_ptr) return fail(h, DSL_ERR_UNSUPPORTED, "dsl_collider_volume_query: not available in slab mode");
  if (h->ids_global) return fail(h, DSL_ERR_INVALID, "dsl_collider_volume_query: host order is gone after dsl_set_ids");
  const size_t nf = (size_t)n_fluid_of(h);
  if (!h->colv_on) {  // no volume: no cell anywhere
    if (dist) std::fill(dist, dist + nf, 0.0f);
    if (normal) std::fill(normal, normal + 3 * nf, 0.0f);
    return DSL_OK;
  }
  if (!h->colv_query)
    if (int rc = dev_alloc(h, &h->colv_query, (size_t)4 * h->cap)) return rc;
  float* qd = h->colv_query;
  float* qn = h->colv_query + nf;
  if (h->colv_moving) {
    if (int rc = collide_volume_rigid_query(h, dist ? qd : nullptr, normal ? qn : nullptr)) return rc;
  } else {
    hipLaunchKernelGGL(k_collide_volume<false>, dim3((unsigned)((h->n + kSdfBlock - 1) / kSdfBlock)), dim3(kSdfBlock), 0, h->stream, h->n,
                       bnd_of(h), col_vol(h), mpos(h, h->cur_pv), mvel(h, h->cur_pv), dist ? qd : nullptr, normal ? qn : nullptr,
                       (const int*)h->ids[h->cur_ids], (int*)nullptr);
    HIP_TRY(h, hipGetLastError());
  }
  if (dist) HIP_TRY(h, hipMemcpyAsync(dist, qd, nf * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (normal) HIP_TRY(h, hipMemcpyAsync(normal, qn, 3 * nf * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DSL_OK;
}
