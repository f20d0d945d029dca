// bodies.hip -- rigid bodies (dsl_body_*): up to DSL_MAX_BODIES volume colliders, each with a pose of its own, applied in one
// pass in the order they were added, and the poses integrated on the device from what the fluid hands to each body.  A
// translation unit of its own, so that sdf.hip's and sdf_rigid.hip's kernels come out as they are; its kernel list is
// tests/golden/device_kernels_bodies.txt.  The cell evaluation and the workgroup tree are lattice.hpp's (volume_cell_eval,
// rigid_tree), the per-body response is k_collide_volume_rigid's rule.  Same flags as
// every unit: -ffp-contract=off keeps every operation at one rounding, `/` and sqrtf are the correctly rounded ones.  The
// rule is build-defined (include/dslsph.h) and restated operation for operation in tests/bodies_ref.py; it is
// the same in both math modes.
//
//   k_bodies_pass   one lane per particle slot, x and v in registers across the bodies: per body the record from device
//                   memory at a wave-uniform address, x into the body's frame, the cell evaluation, the response; behind a
//                   workgroup vote the six sums of J and q x J in the fixed tree, to partial[body][6][nb]
//   k_body_query    d and the world-space n against one body, no response
//   k_bodies_fold   one workgroup per body: the partials in a fixed order, added once into the body's accumulators; then,
//                   for a step driver, one lane integrates the body's pose and stores it for the next pass
#include "bodies_device.hpp"
#include "engine.hpp"
#include "sph_device.hpp"

#include <cmath>
#include <cstddef>
#include <cstring>

namespace dsl {

// (BodyRec, the pose helpers and body_contact: bodies_device.hpp, shared with contact.hip)
namespace {
// The integration of include/dslsph.h, steps 1 to 5, on one lane: (J, tau) = c, R the pose the pass used.  No gyroscopic term
__device__ __forceinline__ void body_integrate(BodyRec& m, const float (&c)[6], float dt) {
  float lin[3], ang[3], tl[3], wl[3], q[4], r[9];
#pragma unroll
  for (int a = 0; a < 9; ++a) r[a] = m.rot[a];
#pragma unroll
  for (int a = 0; a < 3; ++a) lin[a] = m.s.lin_vel[a] + (c[a] * m.p.inv_mass + m.p.accel[a] * dt);
#pragma unroll
  for (int a = 0; a < 3; ++a) tl[a] = dot3(r[a], r[3 + a], r[6 + a], c[3], c[4], c[5]);
#pragma unroll
  for (int a = 0; a < 3; ++a) wl[a] = tl[a] * m.p.inv_inertia[a];
#pragma unroll
  for (int a = 0; a < 3; ++a) ang[a] = m.s.ang_vel[a] + dot3(r[3 * a], r[3 * a + 1], r[3 * a + 2], wl[0], wl[1], wl[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    m.s.lin_vel[a] = lin[a];
    m.s.ang_vel[a] = ang[a];
    m.s.trans[a] = m.s.trans[a] + dt * lin[a];
  }
  const float qw = m.s.quat[0], qx = m.s.quat[1], qy = m.s.quat[2], qz = m.s.quat[3];
  const float dw = -((ang[0] * qx + ang[1] * qy) + ang[2] * qz);
  const float dx = qw * ang[0] + (ang[1] * qz - ang[2] * qy);
  const float dy = qw * ang[1] + (ang[2] * qx - ang[0] * qz);
  const float dz = qw * ang[2] + (ang[0] * qy - ang[1] * qx);
  const float hd = 0.5f * dt;
  q[0] = qw + hd * dw;
  q[1] = qx + hd * dx;
  q[2] = qy + hd * dy;
  q[3] = qz + hd * dz;
  quat_normalize(q);
  quat_to_rot(q, r);
#pragma unroll
  for (int a = 0; a < 4; ++a) m.s.quat[a] = q[a];
#pragma unroll
  for (int a = 0; a < 9; ++a) m.rot[a] = r[a];
}
}  // namespace

// No body is skipped for a particle by any test of the kernel's own: every live slot goes through volume_cell_eval for every
// body, and only its own `cell` decides -- so a particle with a cell is never skipped.  (A bounding test in world space
// would have to bound the rounding of R^T q; none is made.)
__global__ __launch_bounds__(kRigidBlock) void k_bodies_pass(int n, int nb, int n_bodies, Bnd bnd, float mass,
                                                             const BodyRec* __restrict__ rec, Soa3 p, Soa3 v,
                                                             int* __restrict__ hits, float* __restrict__ partial) {
  __shared__ float s_c[6 * kRigidBlock];
  const int s = blockIdx.x * kRigidBlock + threadIdx.x;
  const bool live = s < n && !bnd.is(s);  // boundary particles are not touched
  float px = 0.f, py = 0.f, pz = 0.f, vx = 0.f, vy = 0.f, vz = 0.f;
  if (live) px = p.x[s], py = p.y[s], pz = p.z[s];
  bool have_v = false, x_moved = false, v_changed = false;
  int my_hits = 0;
  for (int b = 0; b < n_bodies; ++b) {
    const BodyRec& m = rec[b];  // (wave-uniform address)
    bool responded = false;
    float c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live) {
      const BodyContact k = body_contact(m, px, py, pz);
      if (k.has_n && k.d < m.p.radius) {
        ++my_hits;
        x_moved = true;
        const float pen = m.p.radius - k.d;
        px = px + pen * k.nx;
        py = py + pen * k.ny;
        pz = pz + pen * k.nz;
        if (!have_v) {
          vx = v.x[s], vy = v.y[s], vz = v.z[s];
          have_v = true;
        }
        // the body's velocity at the particle: u = lin_vel + ang_vel x q
        const float bx = m.s.lin_vel[0] + (m.s.ang_vel[1] * k.qz - m.s.ang_vel[2] * k.qy);
        const float by = m.s.lin_vel[1] + (m.s.ang_vel[2] * k.qx - m.s.ang_vel[0] * k.qz);
        const float bz = m.s.lin_vel[2] + (m.s.ang_vel[0] * k.qy - m.s.ang_vel[1] * k.qx);
        const float vn = dot3(vx - bx, vy - by, vz - bz, k.nx, k.ny, k.nz);
        if (vn < 0.f) {
          responded = true;
          v_changed = true;
          const float f = (1.0f + m.p.restitution) * vn;
          vx = vx - f * k.nx;
          vy = vy - f * k.ny;
          vz = vz - f * k.nz;
          const float mf = mass * f;
          c[0] = mf * k.nx;
          c[1] = mf * k.ny;
          c[2] = mf * k.nz;
          c[3] = k.qy * c[2] - k.qz * c[1];
          c[4] = k.qz * c[0] - k.qx * c[2];
          c[5] = k.qx * c[1] - k.qy * c[0];
        }
      }
    }
    // a workgroup without a responder to this body: the tree of 256 times +0 is +0 (most workgroups of a real scene).  The
    // vote's barrier also stands between wave 0's reads of the last tree and the next tree's writes
    if (__syncthreads_or(responded ? 1 : 0) != 0) rigid_tree(c, s_c);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) partial[((size_t)b * 6 + k) * nb + blockIdx.x] = c[k];
    }
  }
  if (x_moved) p.x[s] = px, p.y[s] = py, p.z[s] = pz;
  if (v_changed) v.x[s] = vx, v.y[s] = vy, v.z[s] = vz;
  // the moved (particle, body) pairs: one integer atomic per wave that has any
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) my_hits += __shfl_down(my_hits, off);
  if ((threadIdx.x & (kWave - 1)) == 0 && my_hits != 0) atomicAdd(hits, my_hits);
}

__global__ __launch_bounds__(kRigidBlock) void k_body_query(int n, Bnd bnd, const BodyRec* __restrict__ rec, CSoa3 p,
                                                            float* __restrict__ qdist, float* __restrict__ qnormal,
                                                            const int* __restrict__ ids) {
  const int s = blockIdx.x * kRigidBlock + threadIdx.x;
  if (!(s < n && !bnd.is(s))) return;
  const BodyContact k = body_contact(*rec, p.x[s], p.y[s], p.z[s]);
  const size_t o = (size_t)ids[s];
  if (qdist) qdist[o] = k.cell ? k.d : 0.f;
  if (qnormal) {
    qnormal[3 * o] = k.has_n ? k.nx : 0.f;
    qnormal[3 * o + 1] = k.has_n ? k.ny : 0.f;
    qnormal[3 * o + 2] = k.has_n ? k.nz : 0.f;
  }
}

// workgroup b: body b's partials as k_colv_impulse_fold adds them, acc_b += total_b, then (integrate != 0) the pose
__global__ __launch_bounds__(kRigidBlock) void k_bodies_fold(int nb, const float* __restrict__ partial, BodyRec* rec, float dt,
                                                             int integrate) {
  __shared__ float s_c[6 * kRigidBlock];
  float c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // lane l adds its body's partials l, l + 256, ... in ascending order from +0, a trip past the end adding +0: the order of
  // k_colv_impulse_fold (whose device code is pinned, so the loop is restated here), four trips' loads in flight at a time
  const float* mine = partial + (size_t)blockIdx.x * 6 * nb;
  for (int b = threadIdx.x; b < nb; b += 4 * kRigidBlock) {
    float t[4][6];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int br = b + r * kRigidBlock;
#pragma unroll
      for (int k = 0; k < 6; ++k) t[r][k] = br < nb ? mine[(size_t)k * nb + br] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int k = 0; k < 6; ++k) c[k] = c[k] + t[r][k];
    }
  }
  rigid_tree(c, s_c);
  if (threadIdx.x == 0) {
    BodyRec& m = rec[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 6; ++k) m.acc[k] = m.acc[k] + c[k];
    if (integrate) body_integrate(m, c, dt);
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
namespace {
inline int rigid_blocks(int n) { return (n + kRigidBlock - 1) / kRigidBlock; }
inline BodyRec* recs(const dsl_handle* h) { return reinterpret_cast<BodyRec*>(h->body_rec.p); }

// props and state as a caller gave them: DSL_ERR_INVALID with the argument's name, or DSL_OK
int check_props(dsl_handle* h, const std::string& w, const dsl_body_props* p) {
  if (!p) return fail(h, DSL_ERR_INVALID, w + ": props must not be NULL");
  const float* f = &p->inv_mass;
  for (size_t k = 0; k < sizeof(dsl_body_props) / sizeof(float); ++k)
    if (!std::isfinite(f[k])) return fail(h, DSL_ERR_INVALID, w + ": every entry of props must be finite");
  if (p->inv_mass < 0.0f) return fail(h, DSL_ERR_INVALID, w + ": props.inv_mass must be >= 0");
  for (int a = 0; a < 3; ++a)
    if (p->inv_inertia[a] < 0.0f) return fail(h, DSL_ERR_INVALID, w + ": every entry of props.inv_inertia must be >= 0");
  if (p->radius < 0.0f) return fail(h, DSL_ERR_INVALID, w + ": props.radius must be >= 0");
  return DSL_OK;
}
int check_state(dsl_handle* h, const std::string& w, const dsl_body_state* s) {
  const float* f = s->quat;
  for (size_t k = 0; k < sizeof(dsl_body_state) / sizeof(float); ++k)
    if (!std::isfinite(f[k])) return fail(h, DSL_ERR_INVALID, w + ": every entry of state must be finite");
  const float* q = s->quat;
  const float len2 = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
  if (!(len2 > 0.0f && std::isfinite(len2))) return fail(h, DSL_ERR_INVALID, w + ": state.quat must have a finite squared length > 0");
  return DSL_OK;
}
int check_handle_and_body(dsl_handle* h, const std::string& w, int body) {
  if (h->c.slab_axis >= 0 || h->c.n_ptr) return fail(h, DSL_ERR_UNSUPPORTED, w + ": rigid bodies are not supported in slab mode");
  if (body < 0 || body >= h->n_bodies)
    return fail(h, DSL_ERR_INVALID, w + ": unknown body id " + std::to_string(body) + " (" + std::to_string(h->n_bodies) + " bodies exist)");
  return DSL_OK;
}
// the state a record holds: the unit quaternion and its R
void posed(const dsl_body_state& in, BodyRec* r) {
  r->s = in;
  quat_normalize(r->s.quat);
  quat_to_rot(r->s.quat, r->rot);
}
}  // namespace

namespace {
// no bodies: the volumes, the records and the partial sums go, and leave DSL_OPT_DEVICE_BYTES
void bodies_release(dsl_handle* h) {
  for (auto& v : h->body_vol) {
    h->dev_bytes -= v.count * sizeof(float);
    release(v);
  }
  h->dev_bytes -= h->body_rec.count + h->body_partial.count * sizeof(float);
  release(h->body_rec);
  release(h->body_partial);
  contact_release(h);
  h->n_bodies = 0;
}
}  // namespace

void bodies_free(dsl_handle* h) {
  bodies_release(h);
  (void)hipFree(h->body_query);
}

// The collide pass while bodies exist: the pass over all bodies, then the fold (one workgroup per body), in place on the
// current state; integrate: the fold's last act advances the poses.
int bodies_pass(dsl_handle* h, bool integrate) {
  const int nb = rigid_blocks(h->n), K = h->n_bodies;
  if ((size_t)6 * K * nb > h->body_partial.count)  // (the array covers the capacity: n never exceeds it)
    return fail(h, DSL_ERR_INVALID, "rigid bodies: the partial sums do not cover the particle count");
  HIP_TRY(h, hipMemsetAsync(h->col_hits, 0, sizeof(int), h->stream));
  int rc = timed(h, DSL_K_COLLIDE, [&] {
    hipLaunchKernelGGL(k_bodies_pass, dim3((unsigned)nb), dim3(kRigidBlock), 0, h->stream, h->n, nb, K, bnd_of(h), h->c.mass,
                       (const BodyRec*)recs(h), mpos(h, h->cur_pv), mvel(h, h->cur_pv), h->col_hits, h->body_partial.p);
  });
  if (rc) return rc;
  rc = timed(h, DSL_K_COLLIDE, [&] {
    hipLaunchKernelGGL(k_bodies_fold, dim3((unsigned)K), dim3(kRigidBlock), 0, h->stream, nb, (const float*)h->body_partial.p,
                       recs(h), h->c.dt, integrate ? 1 : 0);
  });
  if (rc) return rc;
  h->grid_valid = false;  // positions moved
  h->masks_valid = false;
  // the bodies against the wall box and each other, at the poses the integration left (contact.hip)
  if (integrate && h->bodies_contact != 0) return contact_step(h);
  return DSL_OK;
}

}  // namespace dsl

using namespace dsl;

int dsl_body_add(dsl_handle* h, const float* dev_volume, const float* host_volume, const float origin[3], const float step[3],
                 const int32_t dims[3], const dsl_body_props* props, const dsl_body_state* state, int* body_id) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_body_add";
  // every refusal comes before anything is touched
  if (h->c.slab_axis >= 0 || h->c.n_ptr) return fail(h, DSL_ERR_UNSUPPORTED, w + ": rigid bodies are not supported in slab mode");
  if (h->n_bodies >= DSL_MAX_BODIES) return fail(h, DSL_ERR_INVALID, w + ": there are DSL_MAX_BODIES = " + std::to_string(DSL_MAX_BODIES) + " bodies already");
  if (h->col_tri > 0)
    return fail(h, DSL_ERR_INVALID, w + ": a mesh collider is set, and a mesh collider, a volume collider and rigid bodies exclude each "
                                        "other; remove the mesh first (dsl_collider_set_mesh with n_triangles = 0)");
  if (h->colv_on)
    return fail(h, DSL_ERR_INVALID, w + ": a volume collider is set, and a mesh collider, a volume collider and rigid bodies exclude each "
                                        "other; remove the volume first (dsl_collider_set_volume with dims = NULL)");
  if ((dev_volume != nullptr) == (host_volume != nullptr)) return fail(h, DSL_ERR_INVALID, w + ": exactly one of dev_volume and host_volume must be given");
  BodyRec r{};
  long long nvox = 0;
  if (int rc = lattice_check(h, w, origin, step, dims, 2, &r.g, &nvox)) return rc;
  if (int rc = check_props(h, w, props)) return rc;
  static const dsl_body_state kAtRest = {{1.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  if (state)
    if (int rc = check_state(h, w, state)) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (a pass in flight still reads the partial sums that may grow)
  const int b = h->n_bodies;
  if (int rc = reserve(h, h->body_rec, sizeof(BodyRec) * DSL_MAX_BODIES, "dsl_body_add: the body records")) return rc;
  if (int rc = reserve(h, h->body_partial, (size_t)6 * (b + 1) * rigid_blocks(h->cap), "dsl_body_add: the partial sums")) return rc;
  if (int rc = reserve(h, h->body_vol[b], (size_t)nvox, "dsl_body_add: the volume")) return rc;
  if (!h->col_hits)
    if (int rc = dev_alloc(h, &h->col_hits, 1)) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->body_vol[b].p, dev_volume ? dev_volume : host_volume, (size_t)nvox * sizeof(float),
                            dev_volume ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  r.vol = h->body_vol[b].p;
  r.p = *props;
  posed(state ? *state : kAtRest, &r);  // (acc: zeros)
  HIP_TRY(h, hipMemcpyAsync(recs(h) + b, &r, sizeof(BodyRec), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (the caller's array and `r` are never retained after the call returns)
  h->body_g[b] = r.g;
  h->contact_built &= ~(1u << b);
  // its contact points, before the body exists: a build that fails leaves the bodies as they were (while
  // DSL_OPT_BODIES_CONTACT is 0 a body gets no list)
  if (h->bodies_contact != 0)
    if (int rc = contact_list_of(h, b)) return rc;
  h->n_bodies = b + 1;
  if (body_id) *body_id = b;
  return DSL_OK;
}

int dsl_bodies_clear(dsl_handle* h) {
  CHECK_HANDLE(h);
  if (h->n_bodies == 0) return DSL_OK;
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (a pass in flight may still read what is freed)
  bodies_release(h);  // (the query's staging array stays for the next bodies)
  return DSL_OK;
}

int dsl_body_set_state(dsl_handle* h, int body, const dsl_body_state* state) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_body_set_state";
  if (int rc = check_handle_and_body(h, w, body)) return rc;
  if (!state) return fail(h, DSL_ERR_INVALID, w + ": state must not be NULL");
  if (int rc = check_state(h, w, state)) return rc;
  BodyRec r{};
  posed(*state, &r);
  // state and rot lie next to each other in the record: one copy, behind whatever pass is in flight on the stream
  static_assert(offsetof(BodyRec, rot) == offsetof(BodyRec, s) + sizeof(dsl_body_state), "state and rot are contiguous");
  HIP_TRY(h, hipMemcpyAsync(reinterpret_cast<char*>(recs(h) + body) + offsetof(BodyRec, s), &r.s, sizeof(r.s) + sizeof(r.rot),
                            hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DSL_OK;
}

int dsl_body_set_props(dsl_handle* h, int body, const dsl_body_props* props) {
  CHECK_HANDLE(h);
  const std::string w = "dsl_body_set_props";
  if (int rc = check_handle_and_body(h, w, body)) return rc;
  if (int rc = check_props(h, w, props)) return rc;
  HIP_TRY(h, hipMemcpyAsync(reinterpret_cast<char*>(recs(h) + body) + offsetof(BodyRec, p), props, sizeof(dsl_body_props),
                            hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DSL_OK;
}

int dsl_body_get_state(dsl_handle* h, int body, dsl_body_state* state, float impulse[3], float torque[3], int reset) {
  CHECK_HANDLE(h);
  if (int rc = check_handle_and_body(h, "dsl_body_get_state", body)) return rc;
  BodyRec r{};
  HIP_TRY(h, hipMemcpyAsync(&r, recs(h) + body, sizeof(BodyRec), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (reset)
    HIP_TRY(h, hipMemsetAsync(reinterpret_cast<char*>(recs(h) + body) + offsetof(BodyRec, acc), 0, sizeof(r.acc), h->stream));
  if (state) *state = r.s;
  for (int k = 0; k < 3; ++k) {
    if (impulse) impulse[k] = r.acc[k];
    if (torque) torque[k] = r.acc[3 + k];
  }
  return DSL_OK;
}

int dsl_body_query(dsl_handle* h, int body, float* dist, float* normal) {
  CHECK_HANDLE(h);
  if (int rc = check_handle_and_body(h, "dsl_body_query", body)) return rc;
  if (h->ids_global) return fail(h, DSL_ERR_INVALID, "dsl_body_query: host order is gone after dsl_set_ids");
  const size_t nf = (size_t)n_fluid_of(h);
  if (!h->body_query)
    if (int rc = dev_alloc(h, &h->body_query, (size_t)4 * h->cap)) return rc;
  float* qd = h->body_query;
  float* qn = h->body_query + nf;
  hipLaunchKernelGGL(k_body_query, dim3((unsigned)rigid_blocks(h->n)), dim3(kRigidBlock), 0, h->stream, h->n, bnd_of(h),
                     (const BodyRec*)(recs(h) + body), cpos(h), dist ? qd : nullptr, normal ? qn : nullptr,
                     (const int*)h->ids[h->cur_ids]);
  HIP_TRY(h, hipGetLastError());
  if (dist) HIP_TRY(h, hipMemcpyAsync(dist, qd, nf * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (normal) HIP_TRY(h, hipMemcpyAsync(normal, qn, 3 * nf * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return DSL_OK;
}
