// bodies_device.hpp -- what the rigid bodies' units share (bodies.hip, contact.hip): the body's record in device memory, the
// pose helpers, and a point against one body.  No __global__ function lives here, and the helpers are inline in an unnamed
// namespace, so both units may include it; bodies.hip's device code comes out as it did while these lived there.
#pragma once

#include "engine.hpp"
#include "sph_device.hpp"

#include <cmath>

namespace dsl {

// A body in device memory: the device writes state and rot (the fold's integration, the contact solve) and acc, the host
// the rest
struct BodyRec {
  const float* vol;
  Lattice g;
  dsl_body_props p;
  dsl_body_state s;  // quat is kept at unit length
  float rot[9];      // row-major R of quat
  float acc[6];      // impulse and torque impulse about s.trans since the last reset
};

namespace {
// q / |q|, |q| = sqrt(((ww + xx) + yy) + zz)
__host__ __device__ inline void quat_normalize(float (&q)[4]) {
  const float len = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) q[k] = q[k] / len;
}
// the row-major R of q = (w, x, y, z): every product, sum and difference rounded, each parenthesis formed first
__host__ __device__ inline void quat_to_rot(const float (&q)[4], float (&r)[9]) {
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  r[0] = 1.0f - 2.0f * (yy + zz);
  r[1] = 2.0f * (xy - wz);
  r[2] = 2.0f * (xz + wy);
  r[3] = 2.0f * (xy + wz);
  r[4] = 1.0f - 2.0f * (xx + zz);
  r[5] = 2.0f * (yz - wx);
  r[6] = 2.0f * (xz - wy);
  r[7] = 2.0f * (yz + wx);
  r[8] = 1.0f - 2.0f * (xx + yy);
}

// The particle against one body: q = x - trans, xl = R^T q, the cell evaluation at xl, n = R (g / |g|)
struct BodyContact {
  float qx, qy, qz, d, nx, ny, nz;
  bool cell, has_n;
};
__device__ __forceinline__ BodyContact body_contact(const BodyRec& m, float px, float py, float pz) {
  BodyContact k;
  k.qx = px - m.s.trans[0], k.qy = py - m.s.trans[1], k.qz = pz - m.s.trans[2];
  const float lx = dot3(m.rot[0], m.rot[3], m.rot[6], k.qx, k.qy, k.qz);
  const float ly = dot3(m.rot[1], m.rot[4], m.rot[7], k.qx, k.qy, k.qz);
  const float lz = dot3(m.rot[2], m.rot[5], m.rot[8], k.qx, k.qy, k.qz);
  const CellEval e = volume_cell_eval(m.g, m.vol, lx, ly, lz);
  k.cell = e.cell;
  k.has_n = e.cell && e.mag > 0.f;
  k.d = e.d;
  const float lnx = e.gx / e.mag, lny = e.gy / e.mag, lnz = e.gz / e.mag;
  k.nx = dot3(m.rot[0], m.rot[1], m.rot[2], lnx, lny, lnz);
  k.ny = dot3(m.rot[3], m.rot[4], m.rot[5], lnx, lny, lnz);
  k.nz = dot3(m.rot[6], m.rot[7], m.rot[8], lnx, lny, lnz);
  return k;
}
}  // namespace

}  // namespace dsl
