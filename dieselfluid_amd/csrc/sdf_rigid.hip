// sdf_rigid.hip -- the volume collider in rigid motion (dsl_collider_volume_motion, dsl_collider_volume_impulse): the collide
// pass and the query of sdf.hip with the particle taken into the body's frame and the normal back out of it, the response
// against the body's surface velocity, and the momentum the fluid hands to the body.  A translation unit of its own, so
// that sdf.hip's kernels come out as they are; its kernel list is tests/golden/device_kernels_sdf_rigid.txt.  The cell
// evaluation is k_collide_volume's (lattice.hpp: volume_cell_eval).  Same flags as every unit: -ffp-contract=off keeps every
// operation at one rounding, `/` and sqrtf are the correctly rounded ones.  The rule is build-defined (include/dslsph.h,
// DESIGN.md 4.6) and restated operation for operation in tests/sdf_rigid_ref.py; it is the same in both math modes.
//
//   k_collide_volume_rigid  one lane per particle slot: x into the body's frame, eight loads, the trilinear value and its
//                           gradient, the response against u = lin_vel + ang_vel x q; RESPOND: the workgroup's six sums of
//                           J and q x J, in a fixed tree, to partial[6][nb]
//   k_colv_impulse_fold     one workgroup: the partials in a fixed order, added once into the six accumulator words
#include "engine.hpp"
#include "sph_device.hpp"

#include <cmath>

namespace dsl {

// (kRigidBlock and the workgroup tree rigid_tree: lattice.hpp, shared with bodies.hip)

// the lattice and the response's constants, then the motion: all by value, wave-uniform
struct RigidVol {
  const float* vol;
  Lattice g;
  float radius, rest, mass;
  float rot[9], trans[3], lin[3], ang[3];
};

template <bool RESPOND>
__global__ __launch_bounds__(kRigidBlock) void k_collide_volume_rigid(int n, int nb, Bnd bnd, RigidVol m, Soa3 p, Soa3 v,
                                                                      float* __restrict__ qdist, float* __restrict__ qnormal,
                                                                      const int* __restrict__ ids, int* __restrict__ hits,
                                                                      float* __restrict__ partial) {
  __shared__ float s_c[RESPOND ? 6 * kRigidBlock : 1];
  const int s = blockIdx.x * kRigidBlock + threadIdx.x;
  const bool live = s < n && !bnd.is(s);  // boundary particles are not touched
  bool moved = false, responded = false;
  float c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const float px = p.x[s], py = p.y[s], pz = p.z[s];
    const float qx = px - m.trans[0], qy = py - m.trans[1], qz = pz - m.trans[2];
    // xl = R^T q
    const float lx = dot3(m.rot[0], m.rot[3], m.rot[6], qx, qy, qz);
    const float ly = dot3(m.rot[1], m.rot[4], m.rot[7], qx, qy, qz);
    const float lz = dot3(m.rot[2], m.rot[5], m.rot[8], qx, qy, qz);
    const CellEval e = volume_cell_eval(m.g, m.vol, lx, ly, lz);
    const bool cell = e.cell, has_n = cell && e.mag > 0.f;
    const float d = e.d, lnx = e.gx / e.mag, lny = e.gy / e.mag, lnz = e.gz / e.mag;
    // n = R nl
    const float nx_ = dot3(m.rot[0], m.rot[1], m.rot[2], lnx, lny, lnz);
    const float ny_ = dot3(m.rot[3], m.rot[4], m.rot[5], lnx, lny, lnz);
    const float nz_ = dot3(m.rot[6], m.rot[7], m.rot[8], lnx, lny, lnz);
    if constexpr (RESPOND) {
      moved = has_n && d < m.radius;
      if (moved) {
        const float pen = m.radius - d;
        p.x[s] = px + pen * nx_;
        p.y[s] = py + pen * ny_;
        p.z[s] = pz + pen * nz_;
        // the body's velocity at the particle: u = lin_vel + ang_vel x q
        const float bx = m.lin[0] + (m.ang[1] * qz - m.ang[2] * qy);
        const float by = m.lin[1] + (m.ang[2] * qx - m.ang[0] * qz);
        const float bz = m.lin[2] + (m.ang[0] * qy - m.ang[1] * qx);
        const float vx = v.x[s], vy = v.y[s], vz = v.z[s];
        const float vn = dot3(vx - bx, vy - by, vz - bz, nx_, ny_, nz_);
        if (vn < 0.f) {
          responded = true;
          const float f = (1.0f + m.rest) * vn;
          v.x[s] = vx - f * nx_;
          v.y[s] = vy - f * ny_;
          v.z[s] = vz - f * nz_;
          const float mf = m.mass * f;
          c[0] = mf * nx_;
          c[1] = mf * ny_;
          c[2] = mf * nz_;
          c[3] = qy * c[2] - qz * c[1];
          c[4] = qz * c[0] - qx * c[2];
          c[5] = qx * c[1] - qy * c[0];
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
    // a workgroup without a responder: the tree of 256 times +0 is +0 (most workgroups of a real scene)
    if (__syncthreads_or(responded ? 1 : 0) != 0) rigid_tree(c, s_c);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) partial[(size_t)k * nb + blockIdx.x] = c[k];
    }
  }
}

// lane l adds the partials l, l + 256, ... in ascending order from +0, the tree combines the 256 lane sums, acc += total
__global__ __launch_bounds__(kRigidBlock) void k_colv_impulse_fold(int nb, const float* __restrict__ partial, float* __restrict__ acc) {
  __shared__ float s_c[6 * kRigidBlock];
  float c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // four trips' 24 loads in flight at a time (one workgroup reads every partial: latency is all there is); the additions
  // stay in ascending order, a trip past the end adding +0
  for (int b = threadIdx.x; b < nb; b += 4 * kRigidBlock) {
    float t[4][6];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int br = b + r * kRigidBlock;
#pragma unroll
      for (int k = 0; k < 6; ++k) t[r][k] = br < nb ? partial[(size_t)k * nb + br] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int k = 0; k < 6; ++k) c[k] = c[k] + t[r][k];
    }
  }
  rigid_tree(c, s_c);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] = acc[k] + c[k];
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
namespace {
RigidVol rigid_vol(const dsl_handle* h) {
  RigidVol m;
  m.vol = h->colv_vol.p;
  m.g = h->colv_g;
  for (int a = 0; a < 3; ++a) m.trans[a] = h->colv_trans[a], m.lin[a] = h->colv_lin[a], m.ang[a] = h->colv_ang[a];
  for (int a = 0; a < 9; ++a) m.rot[a] = h->colv_rot[a];
  m.radius = h->colv_radius;
  m.rest = h->colv_rest;
  m.mass = h->c.mass;
  return m;
}
inline int rigid_blocks(int n) { return (n + kRigidBlock - 1) / kRigidBlock; }

// partial[6][ceil(cap / 256)] and the six accumulator words, the library's own
int rigid_reserve(dsl_handle* h) {
  if (int rc = reserve(h, h->colv_partial, (size_t)6 * rigid_blocks(h->cap), "dsl_collider_volume_motion: the partial sums")) return rc;
  if (!h->colv_acc)
    if (int rc = dev_alloc(h, &h->colv_acc, 6)) return rc;  // (zeroed)
  return DSL_OK;
}
}  // namespace

void sdf_rigid_free(dsl_handle* h) {
  release(h->colv_partial);
  (void)hipFree(h->colv_acc);
}

// dsl_collider_set_volume: motion off, the accumulators at zero (behind whatever pass is still in flight on the stream)
int collide_volume_rigid_reset(dsl_handle* h) {
  h->colv_moving = false;
  if (h->colv_acc) HIP_TRY(h, hipMemsetAsync(h->colv_acc, 0, 6 * sizeof(float), h->stream));
  return DSL_OK;
}

// The collide pass while a motion is set: the rigid pass, then the fold, in place on the current state.
int collide_volume_rigid_pass(dsl_handle* h) {
  const int nb = rigid_blocks(h->n);
  if ((size_t)6 * nb > h->colv_partial.count)  // (the arrays cover the capacity: n never exceeds it)
    if (int rc = rigid_reserve(h)) return rc;
  HIP_TRY(h, hipMemsetAsync(h->col_hits, 0, sizeof(int), h->stream));
  int rc = timed(h, DSL_K_COLLIDE, [&] {
    hipLaunchKernelGGL(k_collide_volume_rigid<true>, dim3((unsigned)nb), dim3(kRigidBlock), 0, h->stream, h->n, nb, bnd_of(h),
                       rigid_vol(h), mpos(h, h->cur_pv), mvel(h, h->cur_pv), (float*)nullptr, (float*)nullptr, (const int*)nullptr,
                       h->col_hits, h->colv_partial.p);
  });
  if (rc) return rc;
  rc = timed(h, DSL_K_COLLIDE, [&] {
    hipLaunchKernelGGL(k_colv_impulse_fold, dim3(1), dim3(kRigidBlock), 0, h->stream, nb, (const float*)h->colv_partial.p, h->colv_acc);
  });
  if (rc) return rc;
  h->grid_valid = false;  // positions moved
  h->masks_valid = false;
  return DSL_OK;
}

// dsl_collider_volume_query at the pose in force: d and the world-space n into the staging arrays
int collide_volume_rigid_query(dsl_handle* h, float* qd, float* qn) {
  hipLaunchKernelGGL(k_collide_volume_rigid<false>, dim3((unsigned)rigid_blocks(h->n)), dim3(kRigidBlock), 0, h->stream, h->n, 0,
                     bnd_of(h), rigid_vol(h), mpos(h, h->cur_pv), mvel(h, h->cur_pv), qd, qn, (const int*)h->ids[h->cur_ids],
                     (int*)nullptr, (float*)nullptr);
  HIP_TRY(h, hipGetLastError());
  return DSL_OK;
}

}  // namespace dsl

using namespace dsl;

int dsl_collider_volume_motion(dsl_handle* h, const float rot[9], const float trans[3], const float lin_vel[3], const float ang_vel[3]) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_collider_volume_motion";
  // every refusal comes before anything is touched
  if (h->c.slab_axis >= 0 || h->c.n_ptr) return fail(h, DSL_ERR_UNSUPPORTED, w + ": a volume collider is not supported in slab mode");
  if (!h->colv_on) return fail(h, DSL_ERR_INVALID, w + ": no volume collider is set (dsl_collider_set_volume comes first)");
  const struct {
    const float* p;
    int n;
    const char* name;
  } args[4] = {{rot, 9, "rot"}, {trans, 3, "trans"}, {lin_vel, 3, "lin_vel"}, {ang_vel, 3, "ang_vel"}};
  for (const auto& a : args)
    for (int k = 0; a.p && k < a.n; ++k)
      if (!std::isfinite(a.p[k])) return fail(h, DSL_ERR_INVALID, w + ": every entry of " + a.name + " must be finite");
  if (!rot && !trans && !lin_vel && !ang_vel) {  // motion off: the static pass runs again
    h->colv_moving = false;
    return DSL_OK;
  }
  if (int rc = rigid_reserve(h)) return rc;  // (a failed allocation leaves the motion as it was before the first one: off)
  static const float kIdentity[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  for (int k = 0; k < 9; ++k) h->colv_rot[k] = rot ? rot[k] : kIdentity[k];
  for (int k = 0; k < 3; ++k) {
    h->colv_trans[k] = trans ? trans[k] : 0.0f;
    h->colv_lin[k] = lin_vel ? lin_vel[k] : 0.0f;
    h->colv_ang[k] = ang_vel ? ang_vel[k] : 0.0f;
  }
  h->colv_moving = true;
  return DSL_OK;
}

int dsl_collider_volume_impulse(dsl_handle* h, float impulse[3], float torque[3], int reset) {
  CHECK_HANDLE(h);
  if (h->c.slab_axis >= 0 || h->c.n_ptr) return fail(h, DSL_ERR_UNSUPPORTED, "dsl_collider_volume_impulse: a volume collider is not supported in slab mode");
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (h->colv_acc) {  // (never allocated: no motion was ever set, nothing was handed over)
    HIP_TRY(h, hipMemcpyAsync(acc, h->colv_acc, sizeof(acc), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (reset) HIP_TRY(h, hipMemsetAsync(h->colv_acc, 0, sizeof(acc), h->stream));
  }
  for (int k = 0; k < 3; ++k) {
    if (impulse) impulse[k] = acc[k];
    if (torque) torque[k] = acc[3 + k];
  }
  return DSL_OK;
}
