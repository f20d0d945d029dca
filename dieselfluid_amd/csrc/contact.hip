// contact.hip -- the rigid bodies' contact stage (dsl_contact_*, DSL_OPT_BODIES_CONTACT): contact with the wall box and with each
// other.  A translation unit of its own, so that bodies.hip's, sdf.hip's and sdf_rigid.hip's kernels come out as they are; its
// kernel list is tests/golden/device_kernels_contact.txt.  The record, the pose helpers and body_contact are
// bodies_device.hpp's, the cell evaluation is lattice.hpp's.  Same flags as every unit: -ffp-contract=off keeps every
// operation at one rounding, `/` and sqrtf are the correctly rounded ones.  The rule is build-defined (include/dslsph.h,
// DESIGN.md 4.6) and restated operation for operation in tests/contact_ref.py; it is the same in both math modes.
//
//   k_contact_count   one lane per voxel of a body's volume: is it a contact point (finite, <= 0, an axis neighbour finite
//                     and > 0)?  One count per workgroup of 256 voxels
//   k_contact_scan    one workgroup: the counts into offsets, the total behind them
//   k_contact_emit    the same test again; a point's place is its workgroup's offset plus its rank among the workgroup's
//                     lanes -- counts and a scan, no atomic decides an order
//   k_contact_detect  one lane per contact point, the grid flattened over the bodies through a block table: q = R pl and
//                     x = trans + q in registers across the 6 + K targets; per target, behind a workgroup vote, the eight
//                     sums in the fixed tree and the largest depth, to partial[A][t][9][workgroup]
//   k_contact_fold    one workgroup per (A, t): the partials in k_bodies_fold's order, the table entry E[A][t]
//   k_contact_solve   one lane, plain C++: the entries in order, impulses and push-outs into the records
//
// Limits of the rule: there is no friction and no stacking solver; a body rests with its innermost voxel shell on the wall; a
// body that moves more than its own thickness per step tunnels; contact between bodies reaches as deep as B's band, because
// beyond it |g| = 0; and since a point contributes only where d < 0, a body with an unsigned volume neither initiates a contact
// nor is found by another body's points.
#include "bodies_device.hpp"
#include "engine.hpp"
#include "sph_device.hpp"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

namespace dsl {

// a body's share of the detection's flattened grid
struct ContactBody {
  const int* pts;       // its contact points
  int m, nb;            // their number, and its workgroups: ceil(m / 256)
  int first_block;      // the first of them in the grid
  int pad;
  size_t partial_base;  // its partial sums: [t][9][nb] from here
};
struct WallBox {
  float lo[3], hi[3];
};

namespace {
constexpr int kSums = 8;  // (pen q, pen n, pen, 1); the ninth word of an entry is the depth

// voxel idx of the lattice: a contact point?
__device__ __forceinline__ bool contact_point(const Lattice& g, const float* __restrict__ vol, int idx) {
  const float v = vol[idx];
  if (!(isfinite(v) && v <= 0.f)) return false;
  const int nx = g.n[0], ny = g.n[1], nz = g.n[2];
  const int ix = idx % nx, iy = (idx / nx) % ny, iz = idx / (nx * ny);
  const int nxy = nx * ny;
  bool out = false;
  auto look = [&](bool inside, int at) {
    if (inside) {
      const float u = vol[at];
      out = out || (isfinite(u) && u > 0.f);
    }
  };
  look(ix > 0, idx - 1);
  look(ix < nx - 1, idx + 1);
  look(iy > 0, idx - nx);
  look(iy < ny - 1, idx + nx);
  look(iz > 0, idx - nxy);
  look(iz < nz - 1, idx + nxy);
  return out;
}

// rigid_tree's order over the workgroup's 256 values of each of the eight sums -- for off in 128, 64, ..., 1:
// c[l] += c[l + off] for l < off -- and the largest depth beside them (a maximum is order-free).  lds: 9 x 256 floats
__device__ __forceinline__ void contact_tree(float (&c)[kSums], float& depth, float* lds) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kSums; ++k) lds[k * kRigidBlock + tid] = c[k];
  lds[kSums * kRigidBlock + tid] = depth;
  lds_barrier();
  if (tid < kWave) {  // (wave-uniform)
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
      const float* q = lds + k * kRigidBlock + tid;
      c[k] = (q[0] + q[128]) + (q[64] + q[192]);
    }
    const float* q = lds + kSums * kRigidBlock + tid;
    depth = fmaxf(fmaxf(q[0], q[128]), fmaxf(q[64], q[192]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
      for (int k = 0; k < kSums; ++k) c[k] = c[k] + __shfl_down(c[k], off);
      depth = fmaxf(depth, __shfl_down(depth, off));
    }
  }
}
}  // namespace

__global__ __launch_bounds__(kRigidBlock) void k_contact_count(Lattice g, const float* __restrict__ vol, int nvox,
                                                               int* __restrict__ counts) {
  const int idx = blockIdx.x * kRigidBlock + threadIdx.x;
  const bool pt = idx < nvox && contact_point(g, vol, idx);
  const int c = __syncthreads_count(pt ? 1 : 0);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// counts[0 .. nblk) -> their exclusive prefix, counts[nblk] = the total.  One workgroup, 256 counts per trip
__global__ __launch_bounds__(kRigidBlock) void k_contact_scan(int nblk, int* counts) {
  __shared__ int s[kRigidBlock];
  const int tid = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < nblk; base += kRigidBlock) {
    const int i = base + tid;
    const int v = i < nblk ? counts[i] : 0;
    s[tid] = v;
    lds_barrier();
    for (int off = 1; off < kRigidBlock; off <<= 1) {
      const int t = tid >= off ? s[tid - off] : 0;
      lds_barrier();
      s[tid] += t;
      lds_barrier();
    }
    if (i < nblk) counts[i] = carry + (s[tid] - v);
    carry += s[kRigidBlock - 1];
    lds_barrier();  // (the next trip writes s)
  }
  if (tid == 0) counts[nblk] = carry;
}

__global__ __launch_bounds__(kRigidBlock) void k_contact_emit(Lattice g, const float* __restrict__ vol, int nvox,
                                                              const int* __restrict__ offsets, int m, int* __restrict__ pts) {
  __shared__ int s_wave[kRigidBlock / kWave];
  const int idx = blockIdx.x * kRigidBlock + threadIdx.x;
  const bool pt = idx < nvox && contact_point(g, vol, idx);
  const unsigned long long bal = __ballot(pt);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) s_wave[wave] = __popcll(bal);
  lds_barrier();
  int at = offsets[blockIdx.x];
  for (int w = 0; w < wave; ++w) at += s_wave[w];
  at += __popcll(bal & ((1ull << lane) - 1ull));
  if (pt && at < m) pts[at] = idx;  // (at < m by construction: the volume is the library's own copy, unchanged since the count)
}

// No bounding test skips a body for a point: every point goes through volume_cell_eval for every other body, and only its own
// `cell` decides, as in k_bodies_pass.  The records of A and of each B are read at wave-uniform addresses.
__global__ __launch_bounds__(kRigidBlock) void k_contact_detect(int n_bodies, int kinds, int walls, WallBox box,
                                                                const BodyRec* __restrict__ rec,
                                                                const ContactBody* __restrict__ cb,
                                                                const int* __restrict__ block_body,
                                                                float* __restrict__ partial) {
  __shared__ float s_c[(kSums + 1) * kRigidBlock];
  const int A = block_body[blockIdx.x];  // (wave-uniform, like everything read through it)
  const ContactBody& me = cb[A];
  const BodyRec& ma = rec[A];
  const int blk = (int)blockIdx.x - me.first_block, nb = me.nb;
  const int i = blk * kRigidBlock + (int)threadIdx.x;
  const bool live = i < me.m;
  float qx = 0.f, qy = 0.f, qz = 0.f, xx = 0.f, xy = 0.f, xz = 0.f;
  if (live) {
    const int idx = me.pts[i];
    const int nx = ma.g.n[0], ny = ma.g.n[1];
    const float plx = lattice_coord(ma.g.o[0], ma.g.s[0], idx % nx);
    const float ply = lattice_coord(ma.g.o[1], ma.g.s[1], (idx / nx) % ny);
    const float plz = lattice_coord(ma.g.o[2], ma.g.s[2], idx / (nx * ny));
    qx = dot3(ma.rot[0], ma.rot[1], ma.rot[2], plx, ply, plz);
    qy = dot3(ma.rot[3], ma.rot[4], ma.rot[5], plx, ply, plz);
    qz = dot3(ma.rot[6], ma.rot[7], ma.rot[8], plx, ply, plz);
    xx = ma.s.trans[0] + qx;
    xy = ma.s.trans[1] + qy;
    xz = ma.s.trans[2] + qz;
  }
  float* mine = partial + me.partial_base + blk;
  // one target: the point's contribution (or nine +0), the vote, the tree, lane 0's nine words.  The vote's barrier also
  // stands between wave 0's reads of the last tree and the next tree's writes
  auto target = [&](int t, bool on, float pen, float nx, float ny, float nz) {
    float c[kSums] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float depth = 0.f;
    if (on) {
      c[0] = pen * qx, c[1] = pen * qy, c[2] = pen * qz;
      c[3] = pen * nx, c[4] = pen * ny, c[5] = pen * nz;
      c[6] = pen, c[7] = 1.0f;
      depth = pen;
    }
    if (__syncthreads_or(on ? 1 : 0) != 0) contact_tree(c, depth, s_c);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < kSums; ++k) mine[((size_t)t * (kSums + 1) + k) * nb] = c[k];
      mine[((size_t)t * (kSums + 1) + kSums) * nb] = depth;
    }
  };
  const bool wall_on = live && (kinds & 1) != 0 && walls != 0;
  {
    const float px = box.lo[0] - xx, py = box.lo[1] - xy, pz = box.lo[2] - xz;
    const float rx = xx - box.hi[0], ry = xy - box.hi[1], rz = xz - box.hi[2];
    target(0, wall_on && px > 0.f, px, 1.f, 0.f, 0.f);
    target(1, wall_on && rx > 0.f, rx, -1.f, 0.f, 0.f);
    target(2, wall_on && py > 0.f, py, 0.f, 1.f, 0.f);
    target(3, wall_on && ry > 0.f, ry, 0.f, -1.f, 0.f);
    target(4, wall_on && pz > 0.f, pz, 0.f, 0.f, 1.f);
    target(5, wall_on && rz > 0.f, rz, 0.f, 0.f, -1.f);
  }
  const bool body_on = live && (kinds & 2) != 0;
  for (int b = 0; b < n_bodies; ++b) {
    bool on = false;
    float pen = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    if (body_on && b != A) {
      const BodyContact k = body_contact(rec[b], xx, xy, xz);
      if (k.has_n && k.d < 0.f) {
        on = true;
        pen = -k.d;
        nx = k.nx, ny = k.ny, nz = k.nz;
      }
    }
    target(6 + b, on, pen, nx, ny, nz);
  }
}

// workgroup A (6 + K) + t: lane l adds the partials l, l + 256, ... of (A, t) in ascending order from +0, then the same tree
// over the 256 lane sums: k_bodies_fold's order
__global__ __launch_bounds__(kRigidBlock) void k_contact_fold(int n_bodies, const ContactBody* __restrict__ cb,
                                                              const float* __restrict__ partial, float* __restrict__ table) {
  __shared__ float s_c[(kSums + 1) * kRigidBlock];
  const int T = 6 + n_bodies;
  const int A = (int)blockIdx.x / T, t = (int)blockIdx.x % T;
  const ContactBody& me = cb[A];
  const int nb = me.nb;
  const float* mine = partial + me.partial_base + (size_t)t * (kSums + 1) * nb;
  float c[kSums] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float depth = 0.f;
  for (int b = threadIdx.x; b < nb; b += kRigidBlock) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) c[k] = c[k] + mine[(size_t)k * nb + b];
    depth = fmaxf(depth, mine[(size_t)kSums * nb + b]);
  }
  contact_tree(c, depth, s_c);
  if (threadIdx.x == 0) {
    float* e = table + (size_t)blockIdx.x * (kSums + 1);
#pragma unroll
    for (int k = 0; k < kSums; ++k) e[k] = c[k];
    e[kSums] = depth;
  }
}

namespace {
__device__ __forceinline__ void cross3(const float (&u)[3], const float (&v)[3], float (&o)[3]) {
  o[0] = u[1] * v[2] - u[2] * v[1];
  o[1] = u[2] * v[0] - u[0] * v[2];
  o[2] = u[0] * v[1] - u[1] * v[0];
}
// the integration's step 2 on a vector: tl = R^T t, wl_a = tl_a inv_inertia_a, out = R wl
__device__ __forceinline__ void inertia_apply(const BodyRec& m, const float (&t)[3], float (&o)[3]) {
  const float* r = m.rot;
  float wl[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) wl[a] = dot3(r[a], r[3 + a], r[6 + a], t[0], t[1], t[2]) * m.p.inv_inertia[a];
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = dot3(r[3 * a], r[3 * a + 1], r[3 * a + 2], wl[0], wl[1], wl[2]);
}
}  // namespace

// One lane.  A ascending and, inside A, t ascending; every quantity of a body is read from its record as the earlier
// contacts of this solve left it.  count: the entries that got past k > 0
__global__ void k_contact_solve(int n_bodies, const float* __restrict__ table, BodyRec* rec, int* __restrict__ count) {
  const int T = 6 + n_bodies;
  int done = 0;
  for (int A = 0; A < n_bodies; ++A) {
    for (int t = 0; t < T; ++t) {
      const float* e = table + ((size_t)A * T + t) * (kSums + 1);
      const float W = e[6], D = e[8];
      if (!(W > 0.f)) continue;
      const bool wall = t < 6;
      BodyRec& ma = rec[A];
      BodyRec& mb = rec[wall ? A : t - 6];  // (a wall has no second body: never written, its k and u stay out)
      float qc[3], n[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) qc[a] = e[a] / W;
      if (wall) {
        const float sign = (t & 1) ? -1.f : 1.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) n[a] = (t >> 1) == a ? sign : 0.f;
      } else {
        const float len = sqrtf(dot3(e[3], e[4], e[5], e[3], e[4], e[5]));
        if (!(len > 0.f)) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a) n[a] = e[3 + a] / len;
      }
      float x[3], tA[3], y[3], rB[3] = {0.f, 0.f, 0.f}, tB[3] = {0.f, 0.f, 0.f};
      cross3(qc, n, x);
      inertia_apply(ma, x, tA);
      cross3(tA, qc, y);
      float k = ma.p.inv_mass + dot3(y[0], y[1], y[2], n[0], n[1], n[2]);
      if (!wall) {
#pragma unroll
        for (int a = 0; a < 3; ++a) rB[a] = (ma.s.trans[a] + qc[a]) - mb.s.trans[a];
        cross3(rB, n, x);
        inertia_apply(mb, x, tB);
        cross3(tB, rB, y);
        const float kB = mb.p.inv_mass + dot3(y[0], y[1], y[2], n[0], n[1], n[2]);
        k = k + kB;
      }
      if (!(k > 0.f)) continue;
      ++done;
      float wA[3] = {ma.s.ang_vel[0], ma.s.ang_vel[1], ma.s.ang_vel[2]}, uA[3], uB[3] = {0.f, 0.f, 0.f};
      cross3(wA, qc, x);
#pragma unroll
      for (int a = 0; a < 3; ++a) uA[a] = ma.s.lin_vel[a] + x[a];
      if (!wall) {
        float wB[3] = {mb.s.ang_vel[0], mb.s.ang_vel[1], mb.s.ang_vel[2]};
        cross3(wB, rB, x);
#pragma unroll
        for (int a = 0; a < 3; ++a) uB[a] = mb.s.lin_vel[a] + x[a];
      }
      const float vn = dot3(uA[0] - uB[0], uA[1] - uB[1], uA[2] - uB[2], n[0], n[1], n[2]);
      if (vn < 0.f) {
        const float rest = wall ? ma.p.restitution : fminf(ma.p.restitution, mb.p.restitution);
        const float f = (1.0f + rest) * vn;
        const float j = (-f) / k;
        const float jA = j * ma.p.inv_mass;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          ma.s.lin_vel[a] = ma.s.lin_vel[a] + jA * n[a];
          ma.s.ang_vel[a] = ma.s.ang_vel[a] + j * tA[a];
        }
        if (!wall) {
          const float jB = j * mb.p.inv_mass;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            mb.s.lin_vel[a] = mb.s.lin_vel[a] - jB * n[a];
            mb.s.ang_vel[a] = mb.s.ang_vel[a] - j * tB[a];
          }
        }
      }
      if (wall) {
        if (ma.p.inv_mass > 0.f) {
#pragma unroll
          for (int a = 0; a < 3; ++a) ma.s.trans[a] = ma.s.trans[a] + D * n[a];
        }
      } else {
        const float s = ma.p.inv_mass + mb.p.inv_mass;
        if (s > 0.f) {
          const float hA = (0.5f * D) * (ma.p.inv_mass / s), hB = (0.5f * D) * (mb.p.inv_mass / s);
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            ma.s.trans[a] = ma.s.trans[a] + hA * n[a];
            mb.s.trans[a] = mb.s.trans[a] - hB * n[a];
          }
        }
      }
    }
  }
  *count = done;
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
namespace {
inline int blocks_of(long long n) { return (int)((n + kRigidBlock - 1) / kRigidBlock); }
inline const BodyRec* recs(const dsl_handle* h) { return reinterpret_cast<const BodyRec*>(h->body_rec.p); }
inline size_t meta_table_at() { return sizeof(ContactBody) * DSL_MAX_BODIES; }
inline size_t table_words(int K) { return (size_t)(kSums + 1) * K * (6 + K); }

// the contact points of body b: count, scan, (blocking) the total, emit
int build_list(dsl_handle* h, int b) {
  const Lattice& g = h->body_g[b];
  const long long nvox = (long long)g.n[0] * g.n[1] * g.n[2];  // (<= 2^30: lattice_check)
  const int nblk = blocks_of(nvox);
  if (int rc = reserve(h, h->contact_scan, (size_t)nblk + 1, "contact points: the scan")) return rc;
  const float* vol = h->body_vol[b].p;
  hipLaunchKernelGGL(k_contact_count, dim3((unsigned)nblk), dim3(kRigidBlock), 0, h->stream, g, vol, (int)nvox, h->contact_scan.p);
  hipLaunchKernelGGL(k_contact_scan, dim3(1), dim3(kRigidBlock), 0, h->stream, nblk, h->contact_scan.p);
  HIP_TRY(h, hipGetLastError());
  int m = 0;
  HIP_TRY(h, hipMemcpyAsync(&m, h->contact_scan.p + nblk, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (m > 0) {
    if (int rc = reserve(h, h->contact_pts[b], (size_t)m, "contact points: the list")) return rc;
    hipLaunchKernelGGL(k_contact_emit, dim3((unsigned)nblk), dim3(kRigidBlock), 0, h->stream, g, vol, (int)nvox,
                       (const int*)h->contact_scan.p, m, h->contact_pts[b].p);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  h->contact_m[b] = m;
  h->contact_built |= 1u << b;
  h->contact_k = 0;  // (the grid's layout is stale)
  return DSL_OK;
}

// the lists, then the layout of the detection's grid for the bodies that exist: the per-body records, the block table, and
// room for the partial sums, the table and the counter
int prepare(dsl_handle* h) {
  if (int rc = contact_lists(h)) return rc;
  const int K = h->n_bodies;
  if (h->contact_k == K) return DSL_OK;
  std::vector<ContactBody> cb(DSL_MAX_BODIES, ContactBody{});
  std::vector<int> table;
  size_t words = 0;
  for (int b = 0; b < K; ++b) {
    ContactBody& c = cb[b];
    c.pts = h->contact_pts[b].p;
    c.m = h->contact_m[b];
    c.nb = blocks_of(c.m) > 0 ? blocks_of(c.m) : 1;  // (a body without points keeps one workgroup: its entries are written, +0)
    c.first_block = (int)table.size();
    c.partial_base = words;
    words += (size_t)(6 + K) * (kSums + 1) * c.nb;
    table.insert(table.end(), (size_t)c.nb, b);
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (a pass in flight still reads what may be replaced)
  if (int rc = reserve(h, h->contact_meta, meta_table_at() + table.size() * sizeof(int), "contact: the block table")) return rc;
  if (int rc = reserve(h, h->contact_partial, words, "contact: the partial sums")) return rc;
  if (int rc = reserve(h, h->contact_table, table_words(DSL_MAX_BODIES), "contact: the table")) return rc;
  if (int rc = reserve(h, h->contact_ctr, 1, "contact: the counter")) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->contact_meta.p, cb.data(), meta_table_at(), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->contact_meta.p + meta_table_at(), table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice,
                            h->stream));
  HIP_TRY(h, hipMemsetAsync(h->contact_ctr.p, 0, sizeof(int), h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (cb and table are the host's)
  h->contact_blocks = (int)table.size();
  h->contact_k = K;
  h->contact_table_k = 0;
  return DSL_OK;
}

// detection at the current poses, the table fold, and (solve) the solve: two or three launches under DSL_K_COLLIDE
int run(dsl_handle* h, int kinds, bool solve) {
  if (int rc = prepare(h)) return rc;
  const int K = h->n_bodies;
  const ContactBody* cb = reinterpret_cast<const ContactBody*>(h->contact_meta.p);
  const int* block_body = reinterpret_cast<const int*>(h->contact_meta.p + meta_table_at());
  WallBox box;
  for (int a = 0; a < 3; ++a) box.lo[a] = h->prm.box_min[a], box.hi[a] = h->prm.box_max[a];
  int rc = timed(h, DSL_K_COLLIDE, [&] {
    hipLaunchKernelGGL(k_contact_detect, dim3((unsigned)h->contact_blocks), dim3(kRigidBlock), 0, h->stream, K, kinds,
                       (int)h->prm.walls, box, recs(h), cb, block_body, h->contact_partial.p);
  });
  if (rc) return rc;
  rc = timed(h, DSL_K_COLLIDE, [&] {
    hipLaunchKernelGGL(k_contact_fold, dim3((unsigned)(K * (6 + K))), dim3(kRigidBlock), 0, h->stream, K, cb,
                       (const float*)h->contact_partial.p, h->contact_table.p);
  });
  if (rc) return rc;
  h->contact_table_k = K;
  if (!solve) return DSL_OK;
  return timed(h, DSL_K_COLLIDE, [&] {
    hipLaunchKernelGGL(k_contact_solve, dim3(1), dim3(1), 0, h->stream, K, (const float*)h->contact_table.p,
                       reinterpret_cast<BodyRec*>(h->body_rec.p), h->contact_ctr.p);
  });
}

int check_handle(dsl_handle* h, const std::string& w) {
  if (h->c.slab_axis >= 0 || h->c.n_ptr) return fail(h, DSL_ERR_UNSUPPORTED, w + ": rigid bodies are not supported in slab mode");
  return DSL_OK;
}
}  // namespace

void contact_release(dsl_handle* h) {
  auto drop = [&](auto& a) {
    h->dev_bytes -= a.count * sizeof(*a.p);
    release(a);
  };
  for (auto& p : h->contact_pts) drop(p);
  drop(h->contact_scan);
  drop(h->contact_meta);
  drop(h->contact_partial);
  drop(h->contact_table);
  drop(h->contact_ctr);
  h->contact_built = 0;
  h->contact_k = h->contact_blocks = h->contact_table_k = 0;
}

// (dsl_body_add, before body b exists: body_g[b] and body_vol[b] are set, n_bodies is still b)
int contact_list_of(dsl_handle* h, int b) { return build_list(h, b); }

int contact_lists(dsl_handle* h) {
  for (int b = 0; b < h->n_bodies; ++b)
    if (!((h->contact_built >> b) & 1u))
      if (int rc = build_list(h, b)) return rc;
  return DSL_OK;
}

int contact_step(dsl_handle* h) { return run(h, h->bodies_contact, true); }

int contact_option_set(dsl_handle* h, double value) {
  if (!(value == 0.0 || value == 1.0 || value == 2.0 || value == 3.0))
    return fail(h, DSL_ERR_INVALID, "dsl_set_option: DSL_OPT_BODIES_CONTACT is 0, or bit 1 (walls) | bit 2 (bodies)");
  // (the lists of the bodies that exist: a build that fails leaves the option as it was)
  if (value != 0.0 && h->bodies_contact == 0)
    if (int rc = contact_lists(h)) return rc;
  h->bodies_contact = (int)value;
  return DSL_OK;
}

int contact_option_get(dsl_handle* h, int option, double* value) {
  if (option == DSL_OPT_BODIES_CONTACT) {
    *value = (double)h->bodies_contact;
    return DSL_OK;
  }
  int n = 0;  // DSL_OPT_BODIES_CONTACTS
  if (h->contact_ctr.p) {
    HIP_TRY(h, hipMemcpyAsync(&n, h->contact_ctr.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  *value = (double)n;
  return DSL_OK;
}

}  // namespace dsl

using namespace dsl;

int dsl_contact_points(dsl_handle* h, int body, int32_t* host_voxels, size_t cap, int64_t* count) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_contact_points";
  if (int rc = check_handle(h, w)) return rc;
  if (body < 0 || body >= h->n_bodies)
    return fail(h, DSL_ERR_INVALID, w + ": unknown body id " + std::to_string(body) + " (" + std::to_string(h->n_bodies) + " bodies exist)");
  if (cap > 0 && !host_voxels) return fail(h, DSL_ERR_INVALID, w + ": host_voxels must not be NULL while cap > 0");
  if (int rc = contact_lists(h)) return rc;
  const size_t m = (size_t)h->contact_m[body], take = m < cap ? m : cap;
  if (take > 0) {
    HIP_TRY(h, hipMemcpyAsync(host_voxels, h->contact_pts[body].p, take * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  if (count) *count = (int64_t)m;
  return DSL_OK;
}

int dsl_contact_pass(dsl_handle* h, int kinds, int solve) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_contact_pass";
  if (int rc = check_handle(h, w)) return rc;
  if (h->n_bodies == 0) return fail(h, DSL_ERR_INVALID, w + ": there are no bodies");
  if (kinds < 0 || kinds > 3) return fail(h, DSL_ERR_INVALID, w + ": kinds is bit 1 (walls) | bit 2 (bodies)");
  return run(h, kinds, solve != 0);
}

int dsl_contact_table(dsl_handle* h, float* host, size_t count) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_contact_table";
  if (int rc = check_handle(h, w)) return rc;
  if (!host) return fail(h, DSL_ERR_INVALID, w + ": host must not be NULL");
  const int K = h->contact_table_k;
  if (K == 0 || K != h->n_bodies) return fail(h, DSL_ERR_INVALID, w + ": no detection has run for the bodies that exist");
  if (count != table_words(K))
    return fail(h, DSL_ERR_INVALID, w + ": count must be 9 K (6 + K) = " + std::to_string(table_words(K)));
  HIP_TRY(h, hipMemcpyAsync(host, h->contact_table.p, count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DSL_OK;
}
