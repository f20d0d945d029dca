// surface_mesh.hip -- fluid surfaces as an indexed mesh: dsl_surface_extract's triangles with every vertex stored once, a
// normal per vertex (the volume's negated gradient) and three int32 vertex ids per triangle.  A translation unit of its own;
// its kernel list is tests/golden/device_kernels_surface_mesh.txt.  The triangle count and its scan are surface.hip's
// (surf_count), the device helpers surface_device.hpp's.  Same flags and the same arithmetic discipline as surface.hip: every
// sum, difference and product written with its rounding (__f*_rn), quotients and the square root the correctly rounded
// a / b and __builtin_sqrtf -- both math modes give the same bits.  include/dslsph.h and DESIGN.md 4.5 have the rule.
//
// A vertex lies on a lattice edge (u, d): from voxel u to w = u + (d & 1, (d >> 1) & 1, d >> 2), d in 1..7 -- the seven edge
// types of the Kuhn triangulation.  Vertices are owned by u, and voxels are dealt in bricks of 8 x 8 x 4 VOXELS.
//
//   k_mesh_vertex_count  a 256-lane workgroup owns a brick of voxels, one lane per voxel: it stages the 10 x 10 x 6 voxel values
//                        from -1 to +8 (+4 in z) into LDS (NaN outside the lattice), derives which of the 9 x 9 x 5 cubes
//                        around the brick are live (8 finite corners), every lane forms the 7-bit mask of its voxel's edges
//                        that carry a vertex; a prefix inside the brick gives the per-voxel word (prefix << 7 | mask) and the
//                        brick's count
//   (the scan)           surface.hip's multi-level 64-bit scan over the brick counts (surf_scan_run)
//   k_mesh_vertex_emit   bricks with vertices below the capacity only (two offsets tell): the staging again, one voxel further
//                        (11 x 11 x 7: the gradient at an edge's far end needs that end's neighbour), the lane's
//                        word, and for every set bit the position -- the soup's edge point, the same operations -- and the
//                        normal at id = brick offset + prefix + bits below
//   k_mesh_index_emit    per brick of CUBES with triangles below the capacity, the soup's staging, masks and in-brick prefix
//                        again, next to the 9 x 9 x 5 per-voxel words and the offsets of the up to 8 voxel bricks they belong
//                        to, in LDS; every triangle corner looks its id up: offset[brick(u)] + (word[u] >> 7) +
//                        popcount(word[u] & ((1 << (d - 1)) - 1))
// Every position in the output comes from counts and prefix sums, none from an atomic; no workgroup waits for another.
#include "engine.hpp"
#include "surface_device.hpp"

#include <algorithm>
#include <cmath>

namespace dsl {

// the staged image of a brick of voxels starts at -1 along every axis.  The emit reaches +9 (+5 in z): the far end w of an
// edge and w's neighbour for the gradient; the count stops at +8 (+4), the far corners of the cubes that hold the brick's voxels
constexpr int kMeshSX = kSurfBX + 3, kMeshSY = kSurfBY + 3, kMeshSZ = kSurfBZ + 3;
constexpr int kMeshStaged = kMeshSX * kMeshSY * kMeshSZ;  // 847 floats of LDS
constexpr int kMeshCX = kSurfBX + 2, kMeshCY = kSurfBY + 2, kMeshCZ = kSurfBZ + 2;
constexpr int kMeshCounted = kMeshCX * kMeshCY * kMeshCZ;  // 600
// the cubes that hold a voxel of the brick: corner 0 from -1 to +7 (+3 in z), which is surface.hip's brick image in size
constexpr int kMeshCubes = kSurfVoxels;
constexpr long long kMeshMaxVoxels = 1ll << 28;  // 7 ids per voxel stay below 2^31

struct MeshLattice {
  SurfLattice g;
  int nvx, nvy;  // bricks of 8 x 8 x 4 voxels along x and y
};

namespace {
// the cubes that hold both ends of an edge of type d have corner 0 at u - s for the offsets s with (s & d) == 0: bit s of
// kMeshHolders(d)
__device__ __forceinline__ constexpr unsigned mesh_holders(int d) {
  unsigned m = 0;
  for (int s = 0; s < 8; ++s) m |= ((s & d) == 0 ? 1u : 0u) << s;
  return m;
}

template <int SX = kMeshSX, int SY = kMeshSY>
__device__ __forceinline__ int mesh_offset(int d) {
  return (d & 1) + SX * ((d >> 1) & 1) + SX * SY * (d >> 2);
}

__device__ __forceinline__ bool mesh_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// the brick's SX x SY x SZ voxel values from -1 on into LDS; a voxel outside the lattice is staged as NaN
template <int SX = kMeshSX, int SY = kMeshSY, int SZ = kMeshSZ>
__device__ __forceinline__ void mesh_stage(const float* __restrict__ vol, const SurfLattice& g, int bi, int bj, int bk, float* s_v) {
  for (int e = threadIdx.x; e < SX * SY * SZ; e += kSurfBlock) {
    const int row = e / SX, xo = e - row * SX;
    const int ry = row % SY, rz = row / SY;
    const int vi = bi * kSurfBX + xo - 1, vj = bj * kSurfBY + ry - 1, vk = bk * kSurfBZ + rz - 1;
    float v = __builtin_nanf("");
    if (vi >= 0 && vj >= 0 && vk >= 0 && vi < g.n[0] && vj < g.n[1] && vk < g.n[2]) v = vol[((size_t)vk * g.n[1] + vj) * g.n[0] + vi];
    s_v[e] = v;
  }
  lds_barrier();
}

// one component of the volume's gradient at the voxel at e of the image, whose value is vp and whose index along the axis
// is idx: central where both neighbours are usable (inside the lattice -- staged as NaN otherwise -- and finite), one-sided
// where one is, 0 where none is
__device__ __forceinline__ float mesh_grad(const float* s_v, int e, int stride, float vp, float o, float s, int idx) {
  const float vm = s_v[e - stride], vq = s_v[e + stride];
  const bool um = mesh_finite(vm), uq = mesh_finite(vq);
  const float xm = lattice_coord(o, s, idx - 1), xp = lattice_coord(o, s, idx), xq = lattice_coord(o, s, idx + 1);
  const float hi = uq ? vq : vp, lo = um ? vm : vp;
  const float xhi = uq ? xq : xp, xlo = um ? xm : xp;
  return (um || uq) ? __fsub_rn(hi, lo) / __fsub_rn(xhi, xlo) : 0.0f;
}
}  // namespace

__global__ __launch_bounds__(kSurfBlock) void k_mesh_vertex_count(const float* __restrict__ vol, MeshLattice m, float iso,
                                                                  unsigned* __restrict__ words, surf_u64* __restrict__ counts) {
  __shared__ float s_v[kMeshCounted];
  __shared__ int s_live[kMeshCubes];
  __shared__ int s_wave[kSurfBlock / kWave];
  const SurfLattice& g = m.g;
  const int b = blockIdx.x;
  const int bi = b % m.nvx, bjk = b / m.nvx, bj = bjk % m.nvy, bk = bjk / m.nvy;
  mesh_stage<kMeshCX, kMeshCY, kMeshCZ>(vol, g, bi, bj, bk, s_v);
  // cube (X, Y, Z) of the 9 x 9 x 5 has its corner 0 at (X, Y, Z) of the image
  for (int e = threadIdx.x; e < kMeshCubes; e += kSurfBlock) {
    const int row = e / kSurfVX, X = e - row * kSurfVX, Y = row % kSurfVY, Z = row / kSurfVY;
    const int at = (Z * kMeshCY + Y) * kMeshCX + X;
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) finite = finite && mesh_finite(s_v[at + mesh_offset<kMeshCX, kMeshCY>(c)]);
    s_live[e] = finite ? 1 : 0;
  }
  lds_barrier();
  const int tid = threadIdx.x;
  const int lx = tid & (kSurfBX - 1), ly = (tid / kSurfBX) & (kSurfBY - 1), lz = tid / (kSurfBX * kSurfBY);
  const int at = ((lz + 1) * kMeshCY + ly + 1) * kMeshCX + lx + 1;
  // bit s: the cube with corner 0 at u - s is live
  unsigned live = 0;
#pragma unroll
  for (int s = 0; s < 8; ++s)
    live |= (unsigned)s_live[((lz + 1 - (s >> 2)) * kSurfVY + ly + 1 - ((s >> 1) & 1)) * kSurfVX + lx + 1 - (s & 1)] << s;
  const bool in_u = s_v[at] >= iso;
  unsigned mask = 0;
#pragma unroll
  for (int d = 1; d < 8; ++d) {
    const bool in_w = s_v[at + mesh_offset<kMeshCX, kMeshCY>(d)] >= iso;
    mask |= ((live & mesh_holders(d)) != 0 && in_u != in_w ? 1u : 0u) << (d - 1);
  }
  const int n = __popc(mask);
  int total;
  const int incl = surf_block_scan<int>(n, s_wave, total);
  const int vi = bi * kSurfBX + lx, vj = bj * kSurfBY + ly, vk = bk * kSurfBZ + lz;
  // (a brick without a vertex -- most are -- leaves its words as they were: a triangle corner only ever looks up a voxel
  // that owns a vertex, and k_mesh_vertex_emit skips the brick by its offsets)
  if (total > 0 && vi < g.n[0] && vj < g.n[1] && vk < g.n[2])
    words[((size_t)vk * g.n[1] + vj) * g.n[0] + vi] = ((unsigned)(incl - n) << 7) | mask;
  if (tid == 0) counts[b] = (surf_u64)total;
}

__global__ __launch_bounds__(kSurfBlock) void k_mesh_vertex_emit(const float* __restrict__ vol, MeshLattice m, float iso,
                                                                 const unsigned* __restrict__ words,
                                                                 const surf_u64* __restrict__ offsets,
                                                                 const surf_u64* __restrict__ grand_total, float* __restrict__ pos,
                                                                 float* __restrict__ nrm, surf_u64 cap) {
  __shared__ float s_v[kMeshStaged];
  const surf_u64 brick_off = offsets[blockIdx.x];
  const surf_u64 brick_end = blockIdx.x + 1 < gridDim.x ? offsets[blockIdx.x + 1] : *grand_total;
  // (uniform) a brick without vertices -- most are -- or with none below cap costs two loads
  if (brick_end == brick_off || brick_off >= cap) return;
  const SurfLattice& g = m.g;
  const int b = blockIdx.x;
  const int bi = b % m.nvx, bjk = b / m.nvx, bj = bjk % m.nvy, bk = bjk / m.nvy;
  mesh_stage(vol, g, bi, bj, bk, s_v);  // (the kernel's only barrier)
  const int tid = threadIdx.x;
  const int lx = tid & (kSurfBX - 1), ly = (tid / kSurfBX) & (kSurfBY - 1), lz = tid / (kSurfBX * kSurfBY);
  const int vi = bi * kSurfBX + lx, vj = bj * kSurfBY + ly, vk = bk * kSurfBZ + lz;
  if (!(vi < g.n[0] && vj < g.n[1] && vk < g.n[2])) return;
  const unsigned word = words[((size_t)vk * g.n[1] + vj) * g.n[0] + vi];
  const unsigned mask = word & 127u;
  if (mask == 0) return;
  const surf_u64 first = brick_off + (surf_u64)(word >> 7);
  const int at = ((lz + 1) * kMeshSY + ly + 1) * kMeshSX + lx + 1;
  const float vu = s_v[at];
  const float xu = lattice_coord(g.o[0], g.s[0], vi), yu = lattice_coord(g.o[1], g.s[1], vj), zu = lattice_coord(g.o[2], g.s[2], vk);
  const float x1 = lattice_coord(g.o[0], g.s[0], vi + 1), y1 = lattice_coord(g.o[1], g.s[1], vj + 1), z1 = lattice_coord(g.o[2], g.s[2], vk + 1);
  float gux = 0.0f, guy = 0.0f, guz = 0.0f;
  if (nrm) {
    gux = mesh_grad(s_v, at, 1, vu, g.o[0], g.s[0], vi);
    guy = mesh_grad(s_v, at, kMeshSX, vu, g.o[1], g.s[1], vj);
    guz = mesh_grad(s_v, at, kMeshSX * kMeshSY, vu, g.o[2], g.s[2], vk);
  }
#pragma unroll 1
  for (int d = 1; d < 8; ++d) {
    if (!((mask >> (d - 1)) & 1u)) continue;
    const surf_u64 id = first + (surf_u64)__popc(mask & ((1u << (d - 1)) - 1u));
    if (id >= cap) return;  // (ids only grow with d)
    const int aw = at + mesh_offset(d);
    const float vw = s_v[aw];
    // the soup's edge point, operation by operation
    const float f = __fsub_rn(iso, vu) / __fsub_rn(vw, vu);
    const float xw = (d & 1) ? x1 : xu, yw = (d & 2) ? y1 : yu, zw = (d & 4) ? z1 : zu;
    float* p = pos + 3 * id;
    p[0] = __fadd_rn(xu, __fmul_rn(f, __fsub_rn(xw, xu)));
    p[1] = __fadd_rn(yu, __fmul_rn(f, __fsub_rn(yw, yu)));
    p[2] = __fadd_rn(zu, __fmul_rn(f, __fsub_rn(zw, zu)));
    if (nrm) {
      const float gwx = mesh_grad(s_v, aw, 1, vw, g.o[0], g.s[0], vi + (d & 1));
      const float gwy = mesh_grad(s_v, aw, kMeshSX, vw, g.o[1], g.s[1], vj + ((d >> 1) & 1));
      const float gwz = mesh_grad(s_v, aw, kMeshSX * kMeshSY, vw, g.o[2], g.s[2], vk + (d >> 2));
      const float Gx = __fadd_rn(gux, __fmul_rn(f, __fsub_rn(gwx, gux)));
      const float Gy = __fadd_rn(guy, __fmul_rn(f, __fsub_rn(gwy, guy)));
      const float Gz = __fadd_rn(guz, __fmul_rn(f, __fsub_rn(gwz, guz)));
      const float len = __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(Gx, Gx), __fmul_rn(Gy, Gy)), __fmul_rn(Gz, Gz)));
      const bool ok = len > 0.0f;  // (false for a flat spot and for NaN)
      float* o = nrm + 3 * id;
      o[0] = ok ? (-Gx) / len : 0.0f;
      o[1] = ok ? (-Gy) / len : 0.0f;
      o[2] = ok ? (-Gz) / len : 0.0f;
    }
  }
}

__global__ __launch_bounds__(kSurfBlock) void k_mesh_index_emit(const float* __restrict__ vol, MeshLattice m, float iso,
                                                                const surf_u64* __restrict__ offsets,
                                                                const surf_u64* __restrict__ grand_total,
                                                                const unsigned* __restrict__ words,
                                                                const surf_u64* __restrict__ vertex_offsets, int* __restrict__ indices,
                                                                surf_u64 cap) {
  __shared__ float s_v[kSurfVoxels];
  __shared__ unsigned s_w[kSurfVoxels];
  __shared__ int s_first[8];
  __shared__ int s_wave[kSurfBlock / kWave];
  const surf_u64 brick_off = offsets[blockIdx.x];
  const surf_u64 brick_end = blockIdx.x + 1 < gridDim.x ? offsets[blockIdx.x + 1] : *grand_total;
  // (uniform) as k_surface_emit: a brick without triangles, or with none below cap, costs two loads
  if (brick_end == brick_off || brick_off >= cap) return;
  const SurfLattice& g = m.g;
  const SurfBrick k = surf_brick(g, blockIdx.x);
  const int tid = threadIdx.x;
  // the words of the brick's 9 x 9 x 5 voxels (a brick of cubes starts where the brick of voxels with its coordinates does,
  // and reaches one voxel into the next one along every axis), and the first vertex id of those up to 8 bricks of voxels
  for (int e = tid; e < kSurfVoxels; e += kSurfBlock) {
    const int row = e / kSurfVX, xo = e - row * kSurfVX;
    const int ry = row % kSurfVY, rz = row / kSurfVY;
    const int vi = k.bi * kSurfBX + xo, vj = k.bj * kSurfBY + ry, vk = k.bk * kSurfBZ + rz;
    unsigned w = 0;
    if (vi < g.n[0] && vj < g.n[1] && vk < g.n[2]) w = words[((size_t)vk * g.n[1] + vj) * g.n[0] + vi];
    s_w[e] = w;
  }
  if (tid < 8) {
    const int vbi = k.bi + (tid & 1), vbj = k.bj + ((tid >> 1) & 1), vbk = k.bk + (tid >> 2);
    int first = 0;
    // (a brick of voxels past the lattice holds no voxel: no word of the image points at it)
    if (vbi * kSurfBX < g.n[0] && vbj * kSurfBY < g.n[1] && vbk * kSurfBZ < g.n[2])
      first = (int)vertex_offsets[((size_t)vbk * m.nvy + vbj) * m.nvx + vbi];  // (< 7 * 2^28)
    s_first[tid] = first;
  }
  surf_stage(vol, g, k, s_v);  // (ends in the barrier that covers s_w and s_first too)
  const int base = surf_lane_base(tid);
  const unsigned mask = surf_mask(s_v, iso, base);
  const int n = kSurfCubeTriangles[mask];
  int total;
  const int incl = surf_block_scan<int>(n, s_wave, total);
  if (n == 0) return;
  surf_u64 at = brick_off + (surf_u64)(incl - n);
  const int cx = tid & (kSurfBX - 1), cy = (tid / kSurfBX) & (kSurfBY - 1), cz = tid / (kSurfBX * kSurfBY);

  for (int t = 0; t < kSurfTets; ++t) {
    unsigned m4 = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) m4 |= ((mask >> kSurfTetCorner[t][c]) & 1u) << c;
    const int nt = kSurfTetTriangles[t][m4];
    for (int q = 0; q < nt; ++q, ++at) {
      if (at >= cap) return;  // (at only grows)
      int id[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int pair = kSurfTetEdge[t][m4][3 * q + e];
        const int u = pair & 7, d = (pair >> 3) ^ u;  // (every edge of a Kuhn tetrahedron runs from u to u | d)
        const unsigned w = s_w[surf_corner_at(base, u)];
        const int owner = ((cx + (u & 1)) >> 3) | (((cy + ((u >> 1) & 1)) >> 3) << 1) | (((cz + (u >> 2)) >> 2) << 2);
        id[e] = s_first[owner] + (int)(w >> 7) + __popc(w & ((1u << (d - 1)) - 1u));
      }
      int* o = indices + 3 * at;
      o[0] = id[0];
      o[1] = id[1];
      o[2] = id[2];
    }
  }
}

namespace {
MeshLattice mesh_lattice(const SurfLattice& g, long long* nvb) {
  MeshLattice m;
  m.g = g;
  m.nvx = (g.n[0] + kSurfBX - 1) / kSurfBX;
  m.nvy = (g.n[1] + kSurfBY - 1) / kSurfBY;
  *nvb = (long long)m.nvx * m.nvy * ((g.n[2] + kSurfBZ - 1) / kSurfBZ);
  return m;
}

// (dims that are refused for another reason are left to that refusal)
bool mesh_too_many_voxels(const int32_t* dims) {
  if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return false;
  long long nvox = 1;
  for (int a = 0; a < 3; ++a) {
    nvox *= dims[a];  // (each factor < 2^31 and the running product is checked: no overflow)
    if (nvox > kMeshMaxVoxels) return true;
  }
  return false;
}

// the counts and the scans: surf_scan / surf_ctr hold the triangles' offsets and T (surf_count), mesh_scan every voxel
// brick's first vertex id, mesh_words every voxel's word, mesh_ctr[0] V.  dev_counts: device memory for (V, T), or NULL
int mesh_count(dsl_handle* h, const float* vol, const SurfLattice& g, long long nb, float iso, long long* dev_counts) {
  if (!h->mesh_ctr) {
    if (int rc = dev_alloc(h, &h->mesh_ctr, 2)) return rc;
  }
  h->mesh_clock.reset();
  if (int rc = surf_count(h, vol, g, nb, iso, dev_counts ? dev_counts + 1 : nullptr)) return rc;
  if (nb == 0) {  // no cubes: no live cube, no vertex
    HIP_TRY(h, hipMemsetAsync(h->mesh_ctr, 0, 2 * sizeof(surf_u64), h->stream));
    if (dev_counts) HIP_TRY(h, hipMemsetAsync(dev_counts, 0, sizeof(long long), h->stream));
    return DSL_OK;
  }
  long long nvb = 0;
  const MeshLattice m = mesh_lattice(g, &nvb);
  std::vector<long long> len;
  std::vector<size_t> first;
  const size_t all = surf_scan_layout(nvb, &len, &first);
  if (int rc = reserve(h, h->mesh_scan, all, "the vertex scan array")) return rc;
  const size_t nvox = (size_t)g.n[0] * g.n[1] * g.n[2];
  if (int rc = reserve(h, h->mesh_words, nvox, "the per-voxel vertex words")) return rc;
  h->mesh_clock.begin(h, 0);
  int rc = timed(h, DSL_K_SURFACE_MESH, [&] {
    hipLaunchKernelGGL(k_mesh_vertex_count, dim3((unsigned)nvb), dim3(kSurfBlock), 0, h->stream, vol, m, iso, h->mesh_words.p, h->mesh_scan.p);
  });
  if (rc) return rc;
  h->mesh_clock.end(h, 0);
  h->mesh_clock.begin(h, 1);
  if ((rc = surf_scan_run(h, DSL_K_SURFACE_MESH, h->mesh_scan.p, len, first, h->mesh_ctr, dev_counts))) return rc;
  h->mesh_clock.end(h, 1);
  return DSL_OK;
}

int mesh_emit(dsl_handle* h, const float* vol, const SurfLattice& g, long long nb, float iso, float* pos, float* nrm, size_t cap_v,
              int32_t* idx, size_t cap_t) {
  if (nb == 0) return DSL_OK;
  long long nvb = 0;
  const MeshLattice m = mesh_lattice(g, &nvb);
  if (cap_v > 0) {
    h->mesh_clock.begin(h, 2);
    const int rc = timed(h, DSL_K_SURFACE_MESH, [&] {
      hipLaunchKernelGGL(k_mesh_vertex_emit, dim3((unsigned)nvb), dim3(kSurfBlock), 0, h->stream, vol, m, iso, h->mesh_words.p,
                         h->mesh_scan.p, h->mesh_ctr, pos, nrm, (surf_u64)cap_v);
    });
    if (rc) return rc;
    h->mesh_clock.end(h, 2);
  }
  if (cap_t > 0) {
    h->mesh_clock.begin(h, 3);
    const int rc = timed(h, DSL_K_SURFACE_MESH, [&] {
      hipLaunchKernelGGL(k_mesh_index_emit, dim3((unsigned)nb), dim3(kSurfBlock), 0, h->stream, vol, m, iso, h->surf_scan.p, h->surf_ctr,
                         h->mesh_words.p, h->mesh_scan.p, (int*)idx, (surf_u64)cap_t);
    });
    if (rc) return rc;
    h->mesh_clock.end(h, 3);
  }
  return DSL_OK;
}

// (V, T) of the last call, blocking
int mesh_read_counts(dsl_handle* h, surf_u64* vt) {
  surf_u64 two[2];
  if (int rc = surf_read_ctr(h, two)) return rc;  // (synchronises the stream)
  vt[0] = 0;
  vt[1] = two[0];
  if (!h->mesh_ctr) return DSL_OK;
  HIP_TRY(h, hipMemcpyAsync(vt, h->mesh_ctr, sizeof(surf_u64), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DSL_OK;
}

}  // namespace

int surface_mesh_option(dsl_handle* h, int option, double* value) {
  *value = 0.0;
  if (option == DSL_OPT_SURFACE_VERTICES) {
    surf_u64 vt[2];
    if (int rc = mesh_read_counts(h, vt)) return rc;
    *value = (double)vt[0];
    return DSL_OK;
  }
  // the last call's launches by phase, from device events of their own (recorded while dsl_timing_enable(1) holds)
  const int p = option - DSL_OPT_SURFACE_MESH_VCOUNT_MS;
  if (p < 0 || p > 3) return DSL_OK;
  return h->mesh_clock.ms(h, p, value);
}

void surface_mesh_free(dsl_handle* h) {
  release(h->mesh_words);
  release(h->mesh_scan);
  (void)hipFree(h->mesh_ctr);
  release(h->mesh_stage);
  h->mesh_clock.destroy();
}

}  // namespace dsl

using namespace dsl;

int dsl_surface_extract_indexed(dsl_handle* h, const float* dev_volume, const float origin[3], const float step[3],
                                const int32_t dims[3], float iso, float* dev_positions, float* dev_normals, size_t cap_vertices,
                                int32_t* dev_indices, size_t cap_triangles, int64_t* dev_counts, int64_t* host_counts) {
  CHECK_HANDLE_ONLY(h);  // (no particle state is read: a live skin episode stays live, a slab handle is as good as any)
  const char* who = "dsl_surface_extract_indexed";
  if (!dev_volume) return fail(h, DSL_ERR_INVALID, std::string(who) + ": dev_volume must not be NULL");
  if (mesh_too_many_voxels(dims)) return fail(h, DSL_ERR_INVALID, std::string(who) + ": dims holds more than 2^28 voxels");
  SurfLattice g;
  long long nb = 0;
  if (int rc = surf_lattice(h, who, origin, step, dims, &g, &nb)) return rc;
  if (!std::isfinite(iso)) return fail(h, DSL_ERR_INVALID, std::string(who) + ": iso must be finite");
  if (cap_vertices > 0 && !dev_positions)
    return fail(h, DSL_ERR_INVALID, std::string(who) + ": dev_positions must not be NULL while cap_vertices > 0");
  if (cap_triangles > 0 && !dev_indices)
    return fail(h, DSL_ERR_INVALID, std::string(who) + ": dev_indices must not be NULL while cap_triangles > 0");
  static_assert(sizeof(long long) == sizeof(int64_t), "the device word is 64 bits");
  if (int rc = mesh_count(h, dev_volume, g, nb, iso, (long long*)dev_counts)) return rc;
  if (int rc = mesh_emit(h, dev_volume, g, nb, iso, dev_positions, dev_normals, cap_vertices, dev_indices, cap_triangles)) return rc;
  if (host_counts) {
    surf_u64 vt[2];
    if (int rc = mesh_read_counts(h, vt)) return rc;
    host_counts[0] = (int64_t)vt[0];
    host_counts[1] = (int64_t)vt[1];
  }
  return DSL_OK;
}

int dsl_field_surface_indexed(dsl_handle* h, int scalar_buffer, const float origin[3], const float step[3], const int32_t dims[3],
                              float iso, float* host_positions, float* host_normals, size_t cap_vertices, int32_t* host_indices,
                              size_t cap_triangles, int64_t counts[2]) {
  CHECK_HANDLE_ONLY(h);
  const char* who = "dsl_field_surface_indexed";
  // every refusal comes before anything is touched: the mesh's own here, the volume's in field_volume_staged
  if (!std::isfinite(iso)) return fail(h, DSL_ERR_INVALID, std::string(who) + ": iso must be finite");
  if (mesh_too_many_voxels(dims)) return fail(h, DSL_ERR_INVALID, std::string(who) + ": dims holds more than 2^28 voxels");
  if (cap_vertices > 0 && !host_positions)
    return fail(h, DSL_ERR_INVALID, std::string(who) + ": host_positions must not be NULL while cap_vertices > 0");
  if (cap_triangles > 0 && !host_indices)
    return fail(h, DSL_ERR_INVALID, std::string(who) + ": host_indices must not be NULL while cap_triangles > 0");
  if (int rc = field_volume_staged(h, scalar_buffer, origin, step, dims)) return rc;
  SurfLattice g;
  long long nb = 0;
  if (int rc = surf_lattice(h, who, origin, step, dims, &g, &nb)) return rc;
  if (int rc = mesh_count(h, h->vol_stage.p, g, nb, iso, nullptr)) return rc;
  surf_u64 vt[2];
  if (int rc = mesh_read_counts(h, vt)) return rc;
  const size_t take_v = (size_t)std::min<surf_u64>(vt[0], (surf_u64)cap_vertices);
  const size_t take_t = (size_t)std::min<surf_u64>(vt[1], (surf_u64)cap_triangles);
  if (take_v + take_t > 0) {
    // positions, normals, then the index triples (32-bit words like the floats) in one array of the library's own
    static_assert(sizeof(int32_t) == sizeof(float), "one array holds both");
    if (int rc = reserve(h, h->mesh_stage, 6 * take_v + 3 * take_t, "dsl_field_surface_indexed: the mesh array")) return rc;
    float* pos = h->mesh_stage.p;
    float* nrm = host_normals ? pos + 3 * take_v : nullptr;
    int32_t* idx = (int32_t*)(pos + 6 * take_v);
    if (int rc = mesh_emit(h, h->vol_stage.p, g, nb, iso, pos, nrm, take_v, idx, take_t)) return rc;
    if (take_v > 0) {
      HIP_TRY(h, hipMemcpyAsync(host_positions, pos, 3 * take_v * sizeof(float), hipMemcpyDeviceToHost, h->stream));
      if (nrm) HIP_TRY(h, hipMemcpyAsync(host_normals, nrm, 3 * take_v * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    if (take_t > 0) HIP_TRY(h, hipMemcpyAsync(host_indices, idx, 3 * take_t * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  if (counts) {
    counts[0] = (int64_t)vt[0];
    counts[1] = (int64_t)vt[1];
  }
  return DSL_OK;
}
