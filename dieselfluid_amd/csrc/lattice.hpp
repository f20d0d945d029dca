// lattice.hpp -- what the lattice units share (volume.hip, surface.hip, surface_mesh.hip, sdf.hip, sdf_rigid.hip): the lattice
// and its check, the volume collider's cell evaluation, and the two kinds of state a unit keeps in the handle -- a device
// array that grows on demand, and the events around a call's phases.  engine.hpp includes it in front of the handle, whose
// members DevArray and PhaseClock are; that is why the functions below take the handle as H.  No __global__ function lives
// here, and the device helper is __forceinline__ in an unnamed namespace, so any unit may include it.
#pragma once

#include "../../include/dslsph.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "sph_device.hpp"

struct dsl_handle;

namespace dsl {

int fail(dsl_handle* h, int code, const std::string& msg);  // (engine.hpp)

// voxel (i, j, k) lies at o + s * (i, j, k) (lattice_coord), x fastest in memory.  The units' own lattices put their brick
// counts behind this head
struct Lattice {
  float o[3], s[3];
  int n[3];
};

// The one check of a caller's lattice: no NULL, then axis by axis dims >= min_dim, at most 2^30 voxels so far, step finite
// and > 0, origin finite.  out (or NULL) gets the lattice, nvox the voxel count
inline int lattice_check(dsl_handle* h, const std::string& who, const float* origin, const float* step, const int32_t* dims,
                         int min_dim, Lattice* out, long long* nvox) {
  if (!origin || !step || !dims) return fail(h, DSL_ERR_INVALID, who + ": origin, step and dims must not be NULL");
  *nvox = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < min_dim) return fail(h, DSL_ERR_INVALID, who + ": every entry of dims must be >= " + std::to_string(min_dim));
    *nvox *= dims[a];  // (each factor < 2^31 and the running product is checked: no overflow)
    if (*nvox > (1ll << 30)) return fail(h, DSL_ERR_INVALID, who + ": dims holds more than 2^30 voxels");
    if (!(std::isfinite(step[a]) && step[a] > 0.0f)) return fail(h, DSL_ERR_INVALID, who + ": every entry of step must be finite and > 0");
    if (!std::isfinite(origin[a])) return fail(h, DSL_ERR_INVALID, who + ": every entry of origin must be finite");
    if (out) out->o[a] = origin[a], out->s[a] = step[a], out->n[a] = dims[a];
  }
  return DSL_OK;
}

namespace {
// The volume collider's trilinear value and analytic gradient at a point (include/dslsph.h; tests/sdf_ref.py: collider_eval
// restates it operation for operation).  cell: the point lies in a cell whose eight corners are finite
struct CellEval {
  bool cell;
  float d, gx, gy, gz, mag;
};
__device__ __forceinline__ CellEval volume_cell_eval(const Lattice& m, const float* vol, float px, float py, float pz) {
  const float ux = (px - m.o[0]) / m.s[0], uy = (py - m.o[1]) / m.s[1], uz = (pz - m.o[2]) / m.s[2];
  const float fx = floorf(ux), fy = floorf(uy), fz = floorf(uz);
  CellEval e = {false, 0.f, 0.f, 0.f, 0.f, 0.f};
  // (false for NaN and the infinities)
  e.cell = fx >= 0.f && fx <= (float)(m.n[0] - 2) && fy >= 0.f && fy <= (float)(m.n[1] - 2) && fz >= 0.f && fz <= (float)(m.n[2] - 2);
  if (e.cell) {
    const float tx = ux - fx, ty = uy - fy, tz = uz - fz;
    const size_t nx = (size_t)m.n[0], nxy = nx * (size_t)m.n[1];
    const float* c = vol + ((size_t)fz * nxy + (size_t)fy * nx + (size_t)fx);
    const float c000 = c[0], c100 = c[1], c010 = c[nx], c110 = c[nx + 1];
    const float c001 = c[nxy], c101 = c[nxy + 1], c011 = c[nxy + nx], c111 = c[nxy + nx + 1];
    e.cell = isfinite(c000) && isfinite(c100) && isfinite(c010) && isfinite(c110) && isfinite(c001) && isfinite(c101) &&
             isfinite(c011) && isfinite(c111);
    auto lerp = [](float a, float b, float t) { return a + t * (b - a); };
    const float e00 = lerp(c000, c100, tx), e10 = lerp(c010, c110, tx), e01 = lerp(c001, c101, tx), e11 = lerp(c011, c111, tx);
    const float f0 = lerp(e00, e10, ty), f1 = lerp(e01, e11, ty);
    e.d = lerp(f0, f1, tz);
    e.gz = (f1 - f0) / m.s[2];
    e.gy = (lerp(e10, e11, tz) - lerp(e00, e01, tz)) / m.s[1];
    const float x0 = lerp(lerp(c000, c010, ty), lerp(c001, c011, ty), tz);
    const float x1 = lerp(lerp(c100, c110, ty), lerp(c101, c111, ty), tz);
    e.gx = (x1 - x0) / m.s[0];
    e.mag = sqrtf(dot3(e.gx, e.gy, e.gz, e.gx, e.gy, e.gz));
  }
  return e;
}

// The workgroup sum of the rigid passes (sdf_rigid.hip, bodies.hip): workgroups of 256 lanes, six components per lane.
constexpr int kRigidBlock = 256;
// The tree of include/dslsph.h over the workgroup's 256 values per component: for off in 128, 64, ..., 1: c[l] += c[l + off]
// for l < off.  Offsets 128 and 64 through LDS -- lane l < 64 forms (c[l] + c[l + 128]) + (c[l + 64] + c[l + 192]), which is
// what the two steps leave in c[l] -- the rest by __shfl_down inside wave 0, whose lane 0 ends with the sums.
__device__ __forceinline__ void rigid_tree(float (&c)[6], float* lds) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 6; ++k) lds[k * kRigidBlock + tid] = c[k];
  lds_barrier();
  if (tid < kWave) {  // (wave-uniform)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const float* q = lds + k * kRigidBlock + tid;
      c[k] = (q[0] + q[128]) + (q[64] + q[192]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
      for (int k = 0; k < 6; ++k) c[k] = c[k] + __shfl_down(c[k], off);
    }
  }
}
}  // namespace

// a library-owned device array that grows on demand and is counted in DSL_OPT_DEVICE_BYTES
template <class T>
struct DevArray {
  T* p = nullptr;
  size_t count = 0;
};
template <class T, class H>
int reserve(H* h, DevArray<T>& a, size_t want, const char* what) {
  if (a.count >= want) return DSL_OK;
  (void)hipFree(a.p);
  h->dev_bytes -= a.count * sizeof(T);
  a.p = nullptr;
  a.count = 0;
  const hipError_t e = hipMalloc((void**)&a.p, want * sizeof(T));
  if (e != hipSuccess) {
    a.p = nullptr;
    (void)hipGetLastError();  // (the handle stays usable: the next launch check must not meet this error)
    return fail(h, DSL_ERR_NOMEM, std::string(what) + ": hipMalloc: " + hipGetErrorString(e));
  }
  a.count = want;
  h->dev_bytes += want * sizeof(T);
  return DSL_OK;
}
template <class T>
void release(DevArray<T>& a) {
  (void)hipFree(a.p);
  a = DevArray<T>();
}

// N phases of a call, an event pair each, recorded while dsl_timing_enable(1) holds; bit p of `recorded`: the last call ran
// phase p between begin and end
template <int N>
struct PhaseClock {
  hipEvent_t ev[2 * N] = {};
  unsigned recorded = 0;

  void reset() { recorded = 0; }
  template <class H>
  void begin(H* h, int p) { mark(h, 2 * p); }
  template <class H>
  void end(H* h, int p) {
    if (mark(h, 2 * p + 1)) recorded |= 1u << p;
  }
  // the phase's time on the device; 0 if the last call did not record it.  Blocks until the phase has ended
  template <class H>
  int ms(H* h, int p, double* value) {
    *value = 0.0;
    if (!((recorded >> p) & 1u)) return DSL_OK;
    float t = 0.f;
    hipError_t e = hipEventSynchronize(ev[2 * p + 1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ev[2 * p], ev[2 * p + 1]);
    if (e != hipSuccess) return fail(h, DSL_ERR_DEVICE, std::string("phase time: ") + hipGetErrorString(e));
    *value = (double)t;
    return DSL_OK;
  }
  void destroy() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }

 private:
  template <class H>
  bool mark(H* h, int k) {
    if (h->timing != 1) return false;
    if (!ev[k]) (void)hipEventCreate(&ev[k]);
    (void)hipEventRecord(ev[k], h->stream);
    return true;
  }
};

}  // namespace dsl
