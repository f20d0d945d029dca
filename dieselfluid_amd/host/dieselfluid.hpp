// dieselfluid.hpp -- C++ host side above the C ABI (include/dslsph.h), mirroring the
// reference's Go interfaces for the SPH hot path one to one: same type and method names,
// same argument meaning, same error behaviour.  The reference is Go; this image has no
// Go toolchain, so the host layer that a Go maintainer would write in Go (see
// bindings/go/dslsph and INTEGRATION.md) is provided in C++ where the tests can build and
// run it.  Nothing here computes particle physics on the CPU: every pass is a call into
// libdslsph.so.  Host-side work is limited to what the reference itself does on the host
// before handing buffers to the device: the initial lattice (geom/grid/point-grid.go) and
// the PCISPH delta scalar (model/sph/fluid.go:221-277).
//
// Mirrors (file:line in the dieselfluid repository):
//   dsl::sph::SPH                 model/sph/fluid.go:23-277
//   dsl::mesh::Mesh / InitMesh    geom/mesh/mesh.go:11-76, geom/triangle/tri.go:37-101 (Collision: one point, on the host)
//   dsl::solver::SPHMethod        solver/method.go:3-6
//   dsl::solver::WCSPH            solver/wcsph/wcsph.go:9-75
//   dsl::solver::PciMethod        solver/pcisph/pcisph_darwin.go:11-118
//   dsl::solver::GPUPredictorCorrector  solver/pcisph/pcisph_gpu_darwin.go:22-286
//   dsl::compute::Descriptor / ComputeGPU   compute/compute.go:9-53, compute/gpu/gpu.go:20-425
//   dsl::Chan<T>                  Go unbuffered channel used by the drivers
#pragma once

#include <array>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dslsph.h"

namespace dsl {

// model/model.go:11-15 thread message enums
constexpr int THREAD_WAIT = 100;
constexpr int THREAD_GO = 101;
constexpr int THREAD_ERR = 102;
constexpr int THREAD_DONE = 103;
constexpr int SPH_THREAD_WAITING = 104;

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// Minimal stand-in for a Go channel: blocking send/recv plus the non-blocking forms the
// PCISPH driver uses in its select{} statements (pcisph_darwin.go:103-116).
template <class T>
class Chan {
 public:
  void send(T v) {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return !slot_.has_value(); });
    slot_ = std::move(v);
    cv_.notify_all();
  }
  T recv() {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return slot_.has_value(); });
    T v = std::move(*slot_);
    slot_.reset();
    cv_.notify_all();
    return v;
  }
  bool try_send(T v) {
    std::lock_guard<std::mutex> lk(m_);
    if (slot_.has_value()) return false;
    slot_ = std::move(v);
    cv_.notify_all();
    return true;
  }
  bool try_recv(T& out) {
    std::lock_guard<std::mutex> lk(m_);
    if (!slot_.has_value()) return false;
    out = std::move(*slot_);
    slot_.reset();
    cv_.notify_all();
    return true;
  }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  std::optional<T> slot_;
};

// ---------------------------------------------------------------------------------------
// model/sph
// ---------------------------------------------------------------------------------------
namespace sph {

constexpr float VISCOSITY_WATER = 1.3059f;  // fluid.go:18
constexpr float CACHE_L = 0.8f;             // fluid.go:19

// geom/grid/point-grid.go:26-28,39-40,53-63 + model/field/sph_field.go:87-108.
// origin_len != 3 reproduces V.Add's length-mismatch result (vector.go:171-173).
inline std::vector<float> LatticePositions(int n3, const float* origin, int origin_len) {
  std::vector<float> pos((size_t)n3 * n3 * n3 * 3);
  float minb[3], step[3];
  const float dim = (float)n3;
  for (int a = 0; a < 3; ++a) {
    const float m = -1.0f * 1.0f;
    minb[a] = origin_len == 3 ? m + origin[a] : 0.0f;
  }
  const float inv = 1.0f / dim;
  for (int a = 0; a < 3; ++a) {
    const float t = minb[a] * -2.0f;
    step[a] = inv * t;
  }
  for (int i = 0; i < n3; ++i)
    for (int j = 0; j < n3; ++j)
      for (int k = 0; k < n3; ++k) {
        const int id = k + n3 * (i * n3 + j);
        const float ijk[3] = {(float)i, (float)j, (float)k};
        for (int a = 0; a < 3; ++a) {
          const float sv = step[a] * ijk[a];
          pos[(size_t)3 * id + a] = minb[a] + sv;
        }
      }
  return pos;
}

}  // namespace sph

// geom/mesh/mesh.go: the part of Mesh the SPH path touches.  Host arithmetic is float32 in the reference's operation
// order (vector.go: Dot :268-276, Cross :283-297, Mag :301-308, Norm :322-331), like the lattice above.
namespace mesh {
using Vec = std::array<float, 3>;
inline float Dot(const Vec& a, const Vec& b) {
  const float t0 = a[0] * b[0], t1 = a[1] * b[1], t2 = a[2] * b[2];
  return (t0 + t1) + t2;
}
inline float Mag(const Vec& v) { return (float)std::sqrt((double)Dot(v, v)); }
inline Vec Sub(const Vec& b, const Vec& a) { return {b[0] - a[0], b[1] - a[1], b[2] - a[2]}; }
inline Vec Add(const Vec& a, const Vec& b) { return {a[0] + b[0], a[1] + b[1], a[2] + b[2]}; }
inline Vec Scale(const Vec& a, float k) { return {a[0] * k, a[1] * k, a[2] * k}; }

// Mesh.Collision's four returns (mesh.go:41): normal, barycentric coordinates, collision point, collision; `tri` is the
// index of the colliding triangle (-1: none), which dsl_collider_query returns as well
struct CollisionResult {
  Vec normal{0.f, 0.f, 0.f}, coord{0.f, 0.f, 0.f}, point{0.f, 0.f, 0.f};
  bool collision = false;
  int tri = -1;
};

struct Mesh {
  std::vector<Vec> Vertexes;
  std::vector<Vec> Normals;  // one per triangle (mesh.go:13,20)
  // mesh.go:60-76: one particle per vertex (`density` is unused there too); the bound check
  // `x < len(particle_list)-3` leaves the LAST vertex's particle at the origin
  std::vector<float> GenerateBoundaryParticles(float /*density*/) const {
    const int len = (int)Vertexes.size() * 3;
    std::vector<float> particle_list((size_t)len, 0.0f);
    for (int index = 0; index < (int)Vertexes.size(); ++index) {
      const int x = index * 3;
      if (x < len - 3) {
        particle_list[(size_t)x] = Vertexes[(size_t)index][0];
        particle_list[(size_t)x + 1] = Vertexes[(size_t)index][1];
        particle_list[(size_t)x + 2] = Vertexes[(size_t)index][2];
      }
    }
    return particle_list;
  }

  // Mesh.Collision (mesh.go:41-57) through Triangle.BarycentricCollision / Barycentric (tri.go:37-101) for ONE point on
  // the host: the same query dsl_collider_query answers for every particle on the device, operation for operation.
  CollisionResult Collision(const Vec& P, const Vec& V, double dt, float r) const {
    CollisionResult out;
    if (Mag(V) == 0.0f) return out;  // tri.go:39, for every triangle alike
    const int VERTS = (int)Vertexes.size();
    for (int i = 0; i + 2 < VERTS; i += 3) {
      const Vec& n = Normals[(size_t)i / 3];
      const Vec &a = Vertexes[(size_t)i], &b = Vertexes[(size_t)i + 1], &c = Vertexes[(size_t)i + 2];
      float nDotRay = Dot(n, V);
      if (nDotRay == 0.0f) nDotRay = 0.0001f;
      const float d = Dot(Sub(a, P), n);
      const float k = d / nDotRay;
      const Vec p0 = Add(P, Scale(V, k));
      const float dist = Mag(Sub(P, p0));
      if (!(dist <= r)) continue;
      const Vec v0 = Sub(b, a), v1 = Sub(c, a), v2 = Sub(P, a);  // Barycentric, tri.go:79-101
      const float d00 = Dot(v0, v0), d01 = Dot(v0, v1), d11 = Dot(v1, v1), d20 = Dot(v2, v0), d21 = Dot(v2, v1);
      const float q0 = d00 * d11, q1 = d01 * d01;
      const float denom = q0 - q1;
      const float a0 = d11 * d20, a1 = d01 * d21, b0 = d00 * d21, b1 = d01 * d20;
      const float u = (a0 - a1) / denom;
      const float v = (b0 - b1) / denom;
      const float w = (1.0f - v) - u;
      const float sum = (u + v) + w;
      if (u <= 1.0f && v <= 1.0f && w <= 1.0f && sum <= 1.0f && u >= 0.0f && v >= 0.0f && w >= 0.0f) {
        out.normal = n;
        out.coord = {u, v, w};
        out.point = Add(P, Scale(V, -1.0f * (float)dt));  // tri.go:70
        out.collision = true;
        out.tri = i / 3;
        return out;  // the first triangle in list order (mesh.go:50-52)
      }
    }
    return out;
  }
};

// mesh.InitMesh (mesh.go:17-37), its two quirks included: the loop stops at `i < len(vertices)-3`, so the LAST
// triangle's normal stays the zero vector; and the flip towards `origin` is computed and thrown away (vector.Scale
// returns a new vector, mesh.go:30), so the sign of a normal means nothing.
inline Mesh InitMesh(const std::vector<Vec>& vertices, const Vec& origin) {
  Mesh nMesh;
  nMesh.Vertexes = vertices;
  nMesh.Normals.assign(vertices.size() / 3, Vec{0.f, 0.f, 0.f});
  for (int i = 0; i < (int)vertices.size() - 3; i += 3) {
    const Vec e0 = Sub(vertices[(size_t)i + 1], vertices[(size_t)i]), e1 = Sub(vertices[(size_t)i + 2], vertices[(size_t)i]);
    const float c0a = e0[1] * e1[2], c0b = e0[2] * e1[1], c1a = e0[2] * e1[0], c1b = e1[2] * e0[0], c2a = e0[0] * e1[1],
                c2b = e1[0] * e0[1];
    const Vec N{c0a - c0b, c1a - c1b, c2a - c2b};  // Cross
    Vec n{0.f, 0.f, 0.f};                         // Norm: the zero vector stays zero
    const float l = Mag(N);
    if (l != 0.0f) n = {N[0] / l, N[1] / l, N[2] / l};
    const float dv0 = Dot(n, Sub(vertices[(size_t)i], origin));
    if (dv0 > 0.0f) (void)Scale(n, -1.0f);  // (dropped, as in the reference)
    nMesh.Normals[(size_t)i / 3] = n;
  }
  return nMesh;
}
}  // namespace mesh

namespace sph {

class SPH {
 public:
  // sph.Init(scl, origin, colliders, n3, pci)  fluid.go:41-88.  `colliders` is accepted and
  // ignored exactly as the reference does (BoundaryParticles is commented out, fluid.go:70; Colliders() below
  // hands a list to the device);
  // `boundary_capacity` reserves device slots for a later BoundaryParticles() call.
  static SPH Init(float scl, const std::vector<float>& origin, const std::vector<mesh::Mesh*>* colliders, int n3, bool pci,
                  int device = 0, int math_mode = DSL_MATH_EXACT, int boundary_capacity = 0) {
    (void)scl;
    (void)colliders;
    SPH core;
    if (dsl_params_reference(&core.prm_, n3) != DSL_OK) throw Error(dsl_last_error(nullptr));
    core.prm_.math_mode = math_mode;
    if (boundary_capacity > 0) core.prm_.capacity = core.prm_.n_particles + boundary_capacity;
    core.particles_ = core.prm_.n_particles;
    core.cache_life_ = CACHE_L;
    core.mu_ = VISCOSITY_WATER;
    if (dsl_create(&core.prm_, device, &core.h_) != DSL_OK) throw Error(dsl_last_error(nullptr));
    std::vector<float> pos = LatticePositions(n3, origin.data(), (int)origin.size());
    core.ck(dsl_upload(core.h_, DSL_BUF_POSITIONS, pos.data(), pos.size()));  // AlignWithGrid :71
    core.NN();                                                                 // UpdateSampler :72
    core.DensityAll();                                                         // :73
    const float g[3] = {0.0f, -9.81f * core.prm_.mass, 0.0f};
    core.ExternalAll(g);                                                       // :74
    core.ViscousAll();                                                         // :75
    core.CFL();                                                                // :76
    if (pci) {                                                                 // :78-82
      if (core.pcidelta() == 0.0f) core.delta_ = core.prm_.h;
      core.prm_.delta = core.delta_;
      core.ck(dsl_set_params(core.h_, &core.prm_));
    }
    return core;
  }

  SPH() = default;
  SPH(const SPH&) = delete;
  SPH& operator=(const SPH&) = delete;
  SPH(SPH&& o) noexcept { *this = std::move(o); }
  SPH& operator=(SPH&& o) noexcept {
    if (this != &o) {
      release();
      std::memcpy(&prm_, &o.prm_, sizeof(prm_));
      h_ = o.h_;
      o.h_ = nullptr;
      time_ = o.time_;
      cache_life_ = o.cache_life_;
      mu_ = o.mu_;
      delta_ = o.delta_;
      particles_ = o.particles_;
      boundary_ = o.boundary_;
      motion_ = o.motion_;
    }
    return *this;
  }
  ~SPH() { release(); }

  // SPHField.BoundaryParticles (model/field/sph_field.go:75-85): every collider's vertex particles go
  // to ParticleArray.AddBoundaryParticles (particle_array.go:123-128); returns the last collider's list
  std::vector<float> BoundaryParticles(const std::vector<mesh::Mesh*>& colliders) {
    std::vector<float> colliderPositions;
    for (mesh::Mesh* m : colliders) {
      colliderPositions = m->GenerateBoundaryParticles(2.0f);
      if (!colliderPositions.empty()) {
        ck(dsl_add_boundary_particles(h_, colliderPositions.data(), colliderPositions.size()));
        ck(dsl_get_params(h_, &prm_));  // n_boundary has grown: dsl_set_params wants the current count back
      }
      boundary_ += (int)colliderPositions.size() / 3;
    }
    return colliderPositions;
  }
  int Total() const { return particles_ + boundary_; }  // particle_array.go:134-136

  // The collider list of sph.Init (fluid.go:28,41) handed to the device: the meshes' triangles and normals concatenated in
  // list order (Mesh.Collision per mesh in list order is Mesh.Collision of the concatenation), queried with radius r;
  // `e` is the build-defined response's restitution.  An empty list removes the collider.  From then on the step
  // drivers run the collide pass after Update (include/dslsph.h: dsl_collider_set_mesh).  (A slab handle takes a mesh
  // only with DSL_OPT_COLLIDE_SLAB = 1, set through dsl_set_option on handle(); this single-domain mirror never needs it.)
  void Colliders(const std::vector<mesh::Mesh*>& meshes, float r, float e) {
    std::vector<float> verts, normals;
    for (const mesh::Mesh* m : meshes) {
      const size_t T = m->Vertexes.size() / 3;
      for (size_t k = 0; k < 3 * T; ++k) verts.insert(verts.end(), m->Vertexes[k].begin(), m->Vertexes[k].end());
      for (size_t t = 0; t < T; ++t) {
        const mesh::Vec n = t < m->Normals.size() ? m->Normals[t] : mesh::Vec{0.f, 0.f, 0.f};
        normals.insert(normals.end(), n.begin(), n.end());
      }
    }
    ck(dsl_collider_set_mesh(h_, verts.data(), normals.data(), normals.size() / 3, r, e));
  }

  // Implicit colliders (README.MD:35-37 "SPH/Fluid Implicit Collision Techniques / SDF Processing"; the collider interface
  // "for SDF representation", render/mesh/collider.go:10-36): the signed distance of every point of the lattice
  // origin + step * (i, j, k) to a mesh, negative inside, cut off at `band`, computed on the device
  // (include/dslsph.h: dsl_mesh_distance_volume).  Values are x fastest.
  struct DistanceVolume {
    float origin[3] = {0.f, 0.f, 0.f}, step[3] = {1.f, 1.f, 1.f};
    int32_t dims[3] = {0, 0, 0};
    bool isUnsigned = false;
    std::vector<float> Values;
    float At(int i, int j, int k) const { return Values[((size_t)k * dims[1] + j) * dims[0] + i]; }
  };
  DistanceVolume MeshDistance(const mesh::Mesh& m, const float origin[3], const float step[3], const int32_t dims[3],
                              float band = INFINITY, bool isUnsigned = false) {
    DistanceVolume v;
    std::vector<float> verts;
    for (const mesh::Vec& p : m.Vertexes) verts.insert(verts.end(), p.begin(), p.end());
    for (int a = 0; a < 3; ++a) v.origin[a] = origin[a], v.step[a] = step[a], v.dims[a] = dims[a];
    v.isUnsigned = isUnsigned;
    if (dims[0] > 0 && dims[1] > 0 && dims[2] > 0) v.Values.resize((size_t)dims[0] * dims[1] * dims[2]);
    ck(dsl_mesh_distance_volume(h_, verts.data(), verts.size() / 9, origin, step, dims, band, isUnsigned ? DSL_SDF_UNSIGNED : 0,
                                nullptr, v.Values.data()));
    return v;
  }
  // A collider that wraps a distance volume: a particle closer than `Radius` to the surface is pushed out along the
  // volume's gradient and reflected with `Restitution` (include/dslsph.h: dsl_collider_set_volume).  Any volume will do,
  // MeshDistance's or one the host filled in.  It excludes a mesh list: set one or the other.
  // The reference's collider interface expects movement (render/mesh/collider.go:10-36: Origin, UpdateOrigin, IsStatic).
  // Motion is the rigid motion of the volume's own frame: `Rot` row-major, its columns the body's axes in world
  // coordinates; `Origin` the body frame's origin; `LinVel` the body's velocity there and `AngVel` its angular velocity,
  // world.  The voxels never move: UpdateOrigin / UpdateMotion hand 18 numbers to the next step
  // (include/dslsph.h: dsl_collider_volume_motion).  The library does not integrate the pose.
  struct VolumeCollider {
    DistanceVolume Volume;
    float Radius = 0.f, Restitution = 0.f;
    struct Motion {
      float Rot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
      float Origin[3] = {0.f, 0.f, 0.f}, LinVel[3] = {0.f, 0.f, 0.f}, AngVel[3] = {0.f, 0.f, 0.f};
    };
    struct Momentum {
      float Impulse[3] = {0.f, 0.f, 0.f}, Torque[3] = {0.f, 0.f, 0.f};  // torque impulse about Motion::Origin
    };
  };
  void Collider(const VolumeCollider& c) {
    ck(dsl_collider_set_volume(h_, nullptr, c.Volume.Values.data(), c.Volume.origin, c.Volume.step, c.Volume.dims, c.Radius,
                               c.Restitution, c.Volume.isUnsigned ? DSL_SDF_UNSIGNED : 0));
    motion_ = VolumeCollider::Motion{};  // (a new volume starts where it was built, at rest: the library turns motion off)
  }
  // The mirror keeps the motion last set, so that UpdateOrigin changes the origin alone.
  void UpdateMotion(const VolumeCollider::Motion& m) {
    ck(dsl_collider_volume_motion(h_, m.Rot, m.Origin, m.LinVel, m.AngVel));
    motion_ = m;
  }
  // Collider.UpdateOrigin: the body frame's origin moves; orientation and velocities stay what UpdateMotion last set (the
  // identity and zero after Collider, RemoveVolumeCollider or ClearMotion)
  void UpdateOrigin(const float origin[3]) {
    VolumeCollider::Motion m = motion_;
    for (int a = 0; a < 3; ++a) m.Origin[a] = origin[a];
    UpdateMotion(m);
  }
  // Collider.Origin
  const VolumeCollider::Motion& Motion() const { return motion_; }
  // back to Collider.IsStatic() == true: the static pass runs again
  void ClearMotion() {
    ck(dsl_collider_volume_motion(h_, nullptr, nullptr, nullptr, nullptr));
    motion_ = VolumeCollider::Motion{};
  }
  bool IsStatic() {
    double v = 0.0;
    ck(dsl_get_option(h_, DSL_OPT_COLLIDER_VOLUME_MOVING, &v));
    return v == 0.0;
  }
  // what the fluid handed to the body since the last reset (dsl_collider_volume_impulse): a host integrates the body with it
  VolumeCollider::Momentum Impulse(bool reset = false) {
    VolumeCollider::Momentum m;
    ck(dsl_collider_volume_impulse(h_, m.Impulse, m.Torque, reset ? 1 : 0));
    return m;
  }
  void RemoveVolumeCollider() {
    ck(dsl_collider_set_volume(h_, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, 0));
    motion_ = VolumeCollider::Motion{};
  }
  // distance and unit gradient of the volume collider at every fluid particle (dsl_collider_volume_query)
  void ColliderDistances(std::vector<float>* dist, std::vector<float>* normal) {
    if (dist) dist->resize((size_t)particles_);
    if (normal) normal->resize(3 * (size_t)particles_);
    ck(dsl_collider_volume_query(h_, dist ? dist->data() : nullptr, normal ? normal->data() : nullptr));
  }

  // Rigid bodies: sph.Init's collider list (fluid.go:28,41) for distance volumes -- several VolumeColliders, each with a pose
  // and velocities of its own, applied in list order, their poses integrated on the device from what the fluid hands to them
  // (include/dslsph.h: dsl_body_add).  A Body's voxels stay in its own frame; State.Origin is the frame's origin in world
  // coordinates, the point torques refer to (put it at the centre of mass).  InvMass = 0, InvInertia = 0, Accel = 0: a
  // kinematic body.  Bodies exclude Colliders and Collider.
  struct Body {
    DistanceVolume Volume;
    float Radius = 0.f, Restitution = 0.f;
    float InvMass = 0.f, InvInertia[3] = {0.f, 0.f, 0.f}, Accel[3] = {0.f, 0.f, 0.f};
    struct State {
      float Quat[4] = {1.f, 0.f, 0.f, 0.f};  // w, x, y, z
      float Origin[3] = {0.f, 0.f, 0.f}, LinVel[3] = {0.f, 0.f, 0.f}, AngVel[3] = {0.f, 0.f, 0.f};
    } Pose;
    dsl_body_props props() const {
      dsl_body_props p{};
      p.inv_mass = InvMass, p.radius = Radius, p.restitution = Restitution;
      for (int a = 0; a < 3; ++a) p.inv_inertia[a] = InvInertia[a], p.accel[a] = Accel[a];
      return p;
    }
  };
  static dsl_body_state body_state(const Body::State& s) {
    dsl_body_state out{};
    for (int a = 0; a < 4; ++a) out.quat[a] = s.Quat[a];
    for (int a = 0; a < 3; ++a) out.trans[a] = s.Origin[a], out.lin_vel[a] = s.LinVel[a], out.ang_vel[a] = s.AngVel[a];
    return out;
  }
  // what Bodies::Get returns: the state the device holds and what the fluid handed to the body since the last reset
  struct BodyReading {
    Body::State Pose;
    VolumeCollider::Momentum Momentum;
  };
  // The list itself, bound to the solver: ids are list positions.  There is no removal of one body (the order is part of the rule).
  struct Bodies {
    explicit Bodies(SPH& s) : s_(s) {}
    int Add(const Body& b) {
      const dsl_body_props p = b.props();
      const dsl_body_state st = body_state(b.Pose);
      int id = -1;
      s_.ck(dsl_body_add(s_.h_, nullptr, b.Volume.Values.data(), b.Volume.origin, b.Volume.step, b.Volume.dims, &p, &st, &id));
      return id;
    }
    void Clear() { s_.ck(dsl_bodies_clear(s_.h_)); }
    int Count() {
      double v = 0.0;
      s_.ck(dsl_get_option(s_.h_, DSL_OPT_BODIES, &v));
      return (int)v;
    }
    void Update(int id, const Body::State& pose) {
      const dsl_body_state st = body_state(pose);
      s_.ck(dsl_body_set_state(s_.h_, id, &st));
    }
    void UpdateProps(int id, const Body& b) {
      const dsl_body_props p = b.props();
      s_.ck(dsl_body_set_props(s_.h_, id, &p));
    }
    BodyReading Get(int id, bool reset = false) {
      dsl_body_state st{};
      BodyReading r;
      s_.ck(dsl_body_get_state(s_.h_, id, &st, r.Momentum.Impulse, r.Momentum.Torque, reset ? 1 : 0));
      for (int a = 0; a < 4; ++a) r.Pose.Quat[a] = st.quat[a];
      for (int a = 0; a < 3; ++a) r.Pose.Origin[a] = st.trans[a], r.Pose.LinVel[a] = st.lin_vel[a], r.Pose.AngVel[a] = st.ang_vel[a];
      return r;
    }
    // false: the step drivers leave the poses alone and the host scripts all motion (DSL_OPT_BODIES_INTEGRATE)
    void Integrate(bool on) { s_.ck(dsl_set_option(s_.h_, DSL_OPT_BODIES_INTEGRATE, on ? 1.0 : 0.0)); }
    void Distances(int id, std::vector<float>* dist, std::vector<float>* normal) {
      if (dist) dist->resize((size_t)s_.particles_);
      if (normal) normal->resize(3 * (size_t)s_.particles_);
      s_.ck(dsl_body_query(s_.h_, id, dist ? dist->data() : nullptr, normal ? normal->data() : nullptr));
    }
    // The bodies against the wall box and each other (include/dslsph.h: dsl_contact_points).  kinds: 1 walls | 2 bodies;
    // Contact(kinds) has the step drivers detect and solve behind each integration (DSL_OPT_BODIES_CONTACT), 0 turns it off
    void Contact(int kinds) { s_.ck(dsl_set_option(s_.h_, DSL_OPT_BODIES_CONTACT, (double)kinds)); }
    int Contacts() {
      double v = 0.0;
      s_.ck(dsl_get_option(s_.h_, DSL_OPT_BODIES_CONTACTS, &v));
      return (int)v;
    }
    std::vector<int32_t> ContactPoints(int id) {
      int64_t m = 0;
      s_.ck(dsl_contact_points(s_.h_, id, nullptr, 0, &m));
      std::vector<int32_t> out((size_t)m);
      if (m > 0) s_.ck(dsl_contact_points(s_.h_, id, out.data(), out.size(), &m));
      return out;
    }
    void ContactPass(int kinds, bool solve) { s_.ck(dsl_contact_pass(s_.h_, kinds, solve ? 1 : 0)); }
    // E of the last detection: [body][target][9] = S (3), N (3), W, C, D
    std::vector<float> ContactTable() {
      const size_t K = (size_t)Count();
      std::vector<float> out(9 * K * (6 + K));
      s_.ck(dsl_contact_table(s_.h_, out.data(), out.size()));
      return out;
    }

   private:
    SPH& s_;
  };
  Bodies RigidBodies() { return Bodies(*this); }

  // Sources and sinks (include/dslsph.h: dsl_particles_append): fluid emitted from lattice faces and removed by boxes, on the
  // device, at step counts fixed in advance.  The reference has no counterpart.  N() follows every call made here; after
  // solver steps with an emitter or a sink in place, SyncCount() brings it up to date.
  struct Emitter {
    float Origin[3] = {0.f, 0.f, 0.f}, U[3] = {1.f, 0.f, 0.f}, V[3] = {0.f, 0.f, 1.f};  // point (a, b): Origin + a U + b V
    int Nu = 1, Nv = 1;
    bool Ellipse = false;  // the ellipse inscribed in the Nu x Nv rectangle
    float Velocity[3] = {0.f, 0.f, 0.f};
    int Period = 1;  // a layer every Period-th step from FirstStep on (the handle's step counter), MaxLayers of them (0: no limit)
    int64_t FirstStep = 0, MaxLayers = 0;
  };
  struct Sink {
    float Min[3] = {0.f, 0.f, 0.f}, Max[3] = {0.f, 0.f, 0.f};  // [Min, Max) per axis; entries may be +-infinity
    bool Outside = false;                                      // true: particles outside the box go
  };
  int SyncCount() {
    ck(dsl_get_params(h_, &prm_));
    particles_ = prm_.n_particles;
    return particles_;
  }
  // xyz interleaved, as Positions() returns them; velocities empty: zeros
  void AppendParticles(const std::vector<float>& positions, const std::vector<float>& velocities = {}) {
    ck(dsl_particles_append(h_, positions.data(), velocities.empty() ? nullptr : velocities.data(), positions.size() / 3));
    SyncCount();
  }
  int AddEmitter(const Emitter& e) {
    dsl_emitter d{};
    for (int a = 0; a < 3; ++a) d.origin[a] = e.Origin[a], d.u[a] = e.U[a], d.v[a] = e.V[a], d.velocity[a] = e.Velocity[a];
    d.nu = e.Nu, d.nv = e.Nv, d.shape = e.Ellipse ? 1 : 0, d.period = e.Period;
    d.first_step = e.FirstStep, d.max_layers = e.MaxLayers;
    int id = -1;
    ck(dsl_emitter_add(h_, &d, &id));
    return id;
  }
  void ClearEmitters() { ck(dsl_emitters_clear(h_)); }
  // one layer now, between steps
  void Emit(int emitter) {
    ck(dsl_emit(h_, emitter));
    SyncCount();
  }
  int AddSink(const Sink& s) {
    dsl_sink d{};
    for (int a = 0; a < 3; ++a) d.box_min[a] = s.Min[a], d.box_max[a] = s.Max[a];
    d.outside = s.Outside ? 1 : 0;
    int id = -1;
    ck(dsl_sink_add(h_, &d, &id));
    return id;
  }
  void ClearSinks() { ck(dsl_sinks_clear(h_)); }
  // applies the sinks now; returns how many particles went
  int64_t RemoveParticles() {
    int64_t gone = 0;
    ck(dsl_particles_remove(h_, &gone));
    SyncCount();
    return gone;
  }
  // the step drivers apply the sinks at steps s with s % every == 0 (DSL_OPT_SINK_EVERY; 0: only RemoveParticles does)
  void SinkEvery(int every) { ck(dsl_set_option(h_, DSL_OPT_SINK_EVERY, (double)every)); }

  // The frame recorder (include/dslsph.h: dsl_recorder_set) -- "Fluid Animation Export" (README.MD:39): frames packed on the
  // device at step counts fixed in advance and copied to pinned host memory behind the steps that follow, in place of the
  // reference's blocking read-back of every position after every step (pcisph_gpu_darwin.go:276-279).
  struct Recorder {
    int Every = 1, Stride = 1;  // a frame at steps s >= FirstStep with (s - FirstStep) % Every == 0; every Stride-th particle
    bool Velocities = false, Densities = false;  // beside the positions
    bool Q16 = false;            // 16-bit planes: positions against [BoxMin, BoxMax] or, with AutoBox, each frame's own bounds
    bool AutoBox = true;
    float BoxMin[3] = {0.f, 0.f, 0.f}, BoxMax[3] = {0.f, 0.f, 0.f};
    int Slots = 4;               // 1..64 frames of pinned host memory
    int64_t FirstStep = 0, MaxFrames = 0;  // MaxFrames 0: no limit
  };
  void SetRecorder(const Recorder& r) {
    dsl_recorder d{};
    d.every = r.Every, d.stride = r.Stride, d.slots = r.Slots;
    d.fields = (r.Velocities ? DSL_REC_VELOCITY : 0) | (r.Densities ? DSL_REC_DENSITY : 0);
    d.encoding = r.Q16 ? DSL_REC_Q16 : DSL_REC_F32;
    d.auto_box = (r.Q16 && r.AutoBox) ? 1 : 0;
    for (int a = 0; a < 3; ++a) d.box_min[a] = r.BoxMin[a], d.box_max[a] = r.BoxMax[a];
    d.first_step = r.FirstStep, d.max_frames = r.MaxFrames;
    ck(dsl_recorder_set(h_, &d));
  }
  void ClearRecorder() { ck(dsl_recorder_set(h_, nullptr)); }
  void RecordNow() { ck(dsl_record_now(h_)); }  // one frame of the current state, between steps
  // frames recorded so far; *ready: landed and unreleased; *dropped: found no released slot.  Never blocks
  int64_t PollFrames(int64_t* ready = nullptr, int64_t* dropped = nullptr) {
    int64_t recorded = 0;
    ck(dsl_record_poll(h_, &recorded, ready, dropped));
    return recorded;
  }
  // the oldest unreleased frame, copied out and released (waits for its copy only)
  std::vector<unsigned char> NextFrame() {
    const void* frame = nullptr;
    size_t bytes = 0;
    ck(dsl_record_peek(h_, &frame, &bytes));
    std::vector<unsigned char> out((const unsigned char*)frame, (const unsigned char*)frame + bytes);
    ck(dsl_record_release(h_));
    return out;
  }
  // The animation file: 16 bytes -- "DSLANIM\0", u32 version 1, u32 zero -- then the frames back to back as the library
  // wrote them (each finds the next through its frame_bytes).  Writes the header and every unreleased frame, oldest first;
  // append = true: the frames only, behind a file that has its header.  Returns the frames written
  int WriteAnimation(const std::string& path, bool append = false) {
    std::FILE* f = std::fopen(path.c_str(), append ? "ab" : "wb");
    if (!f) throw std::runtime_error("WriteAnimation: cannot open " + path);
    const unsigned char head[16] = {'D', 'S', 'L', 'A', 'N', 'I', 'M', 0, 1, 0, 0, 0, 0, 0, 0, 0};
    bool ok = append || std::fwrite(head, 1, sizeof(head), f) == sizeof(head);
    int frames = 0;
    const void* frame = nullptr;
    size_t bytes = 0;
    while (ok && dsl_record_peek(h_, &frame, &bytes) == DSL_OK) {  // (DSL_ERR_INVALID: nothing unreleased is left)
      ok = std::fwrite(frame, 1, bytes, f) == bytes;
      ck(dsl_record_release(h_));
      frames += 1;
    }
    ok = std::fclose(f) == 0 && ok;
    if (!ok) throw std::runtime_error("WriteAnimation: write to " + path + " failed");
    return frames;
  }

  // The fluid's surface as a mesh.Mesh (README.MD:38 "SPH/Fluid Surfaces"; the reference's renderer draws meshes): the
  // iso-surface of SPHField.Interpolate on the lattice origin + step * (i, j, k), evaluated, triangulated and wound on the
  // device (include/dslsph.h: dsl_field_surface).  density = false: the pressure field.  The buffer is sized from a guess --
  // four triangles per voxel of the lattice's three faces -- and the library is called again only when that was short.
  mesh::Mesh Surface(const float origin[3], const float step[3], const int32_t dims[3], float iso, bool density = true) {
    size_t cap = 4 * ((size_t)dims[0] * dims[1] + (size_t)dims[1] * dims[2] + (size_t)dims[2] * dims[0]);
    if (cap < 1024) cap = 1024;
    std::vector<float> verts, normals;
    int64_t T = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
      verts.resize(9 * cap);
      normals.resize(3 * cap);
      ck(dsl_field_surface(h_, density ? DSL_BUF_DENSITIES : DSL_BUF_PRESSURES, origin, step, dims, iso, verts.data(), normals.data(),
                           cap, &T));
      if ((size_t)T <= cap) break;
      cap = (size_t)T;
    }
    mesh::Mesh m;
    m.Vertexes.resize(3 * (size_t)T);
    m.Normals.resize((size_t)T);
    for (size_t v = 0; v < 3 * (size_t)T; ++v) m.Vertexes[v] = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
    for (size_t t = 0; t < (size_t)T; ++t) m.Normals[t] = {normals[3 * t], normals[3 * t + 1], normals[3 * t + 2]};
    return m;
  }

  // The same surface as an indexed mesh, what a renderer of indexed (glTF) meshes draws smooth-shaded: every vertex once
  // with the volume's negated, normalised gradient as its normal, three vertex ids per triangle (include/dslsph.h:
  // dsl_field_surface_indexed).  Triangle t is Indices[3 t .. 3 t + 2]; Positions[Indices[..]] are Surface()'s vertices.
  struct IndexedMesh {
    std::vector<mesh::Vec> Positions, Normals;  // V each
    std::vector<int32_t> Indices;               // 3 T
  };
  IndexedMesh SurfaceIndexed(const float origin[3], const float step[3], const int32_t dims[3], float iso, bool density = true) {
    const size_t area = (size_t)dims[0] * dims[1] + (size_t)dims[1] * dims[2] + (size_t)dims[2] * dims[0];
    size_t cap_v = 2 * area < 1024 ? 1024 : 2 * area, cap_t = 4 * area < 1024 ? 1024 : 4 * area;
    std::vector<float> pos, normals;
    IndexedMesh m;
    int64_t counts[2] = {0, 0};
    for (int attempt = 0; attempt < 2; ++attempt) {
      pos.resize(3 * cap_v);
      normals.resize(3 * cap_v);
      m.Indices.resize(3 * cap_t);
      ck(dsl_field_surface_indexed(h_, density ? DSL_BUF_DENSITIES : DSL_BUF_PRESSURES, origin, step, dims, iso, pos.data(),
                                   normals.data(), cap_v, m.Indices.data(), cap_t, counts));
      if ((size_t)counts[0] <= cap_v && (size_t)counts[1] <= cap_t) break;
      if ((size_t)counts[0] > cap_v) cap_v = (size_t)counts[0];
      if ((size_t)counts[1] > cap_t) cap_t = (size_t)counts[1];
    }
    const size_t V = (size_t)counts[0];
    m.Indices.resize(3 * (size_t)counts[1]);
    m.Positions.resize(V);
    m.Normals.resize(V);
    for (size_t v = 0; v < V; ++v) {
      m.Positions[v] = {pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]};
      m.Normals[v] = {normals[3 * v], normals[3 * v + 1], normals[3 * v + 2]};
    }
    return m;
  }

  int N() const { return particles_; }                 // fluid.go:106-108
  void NN() { ck(dsl_build_neighbours(h_)); }          // fluid.go:100-102
  float CFL() {                                        // fluid.go:111-114
    time_ = 0.01f;
    return time_;
  }
  float Time() { return CFL(); }                       // fluid.go:199-202
  float Viscosity() const { return mu_; }
  void SetViscosity(float x) {
    mu_ = x;
    prm_.mu = x;
    ck(dsl_set_params(h_, &prm_));
  }
  float Delta() const { return delta_; }               // fluid.go:204
  float MaxV() {                                       // fluid.go:206
    dsl_stats st;
    ck(dsl_get_stats(h_, &st));
    return st.max_vel;
  }
  void DensityAll() { ck(dsl_density_pass(h_)); }                    // fluid.go:127-131
  int PressureAll() {                                                // fluid.go:134-142
    ck(dsl_pressure_pass(h_));
    return 0;  // SPH_VALID
  }
  void ViscousAll() { ck(dsl_viscous_pass(h_)); }                    // fluid.go:146-152
  void ExternalAll(const float f[3]) { ck(dsl_external_pass(h_, f)); }  // fluid.go:155-161
  void GradientPressureForce() { ck(dsl_gradient_pressure_pass(h_)); }  // fluid.go:164-172
  void Update() { ck(dsl_update_pass(h_)); }                         // fluid.go:175-197
  float CacheIncr() {                                                // fluid.go:208-215
    cache_life_ *= cache_life_;
    if (cache_life_ < 0.1f) {
      cache_life_ = CACHE_L;
      NN();
    }
    return cache_life_;
  }

  // ParticleArray accessors (model/particle_array.go:39-54): blocking device reads in the
  // reference's host layout (xyz interleaved).
  std::vector<float> Positions() {  // Total() particles (particle_array.go:21)
    std::vector<float> out((size_t)Total() * 3);
    ck(dsl_download(h_, DSL_BUF_POSITIONS, out.data(), out.size()));
    return out;
  }
  std::vector<float> Velocities() { return read(DSL_BUF_VELOCITIES, 3); }
  std::vector<float> Forces() { return read(DSL_BUF_FORCES, 3); }
  std::vector<float> Densities() { return read(DSL_BUF_DENSITIES, 1); }
  std::vector<float> Pressures() { return read(DSL_BUF_PRESSURES, 1); }

  dsl_handle* handle() { return h_; }
  dsl_params& params() { return prm_; }
  void ck(int rc) const {
    if (rc != DSL_OK) throw Error(dsl_last_error(h_));
  }

  // fluid.go:221-277 pcidelta/computeBeta -- a host-side scalar in the reference too (it
  // is passed to the device in the "floats" block, pcisph_gpu_darwin.go:61).
  float pcidelta() {
    const int n3 = 8, particles = 512;
    const float origin[3] = {0.f, 0.f, 0.f};
    const std::vector<float> pos = LatticePositions(n3, origin, 3);
    const float h = 1.0f;
    const float B = -45.0f / ((float)3.141592653589 * (h * h * h * h));  // std_kernel.go:27
    float denom = 0.0f, d1[3] = {0.f, 0.f, 0.f}, d2 = 0.0f;
    const int mid = particles / 2;
    int tracking = 0;
    auto mag = [](const float* v) {
      float s = 0.0f;
      for (int i = 0; i < 3; ++i) s += v[i] * v[i];
      return (float)std::sqrt((double)s);
    };
    for (int i = 0; i < particles; ++i) {
      int x = mid + tracking;
      if (i % 2 != 0) {
        x = mid - tracking;
        tracking++;
      }
      if (x < 0 || x > particles) break;
      float p[3] = {0.f, 0.f, 0.f};
      if (x < particles) std::memcpy(p, &pos[(size_t)3 * x], sizeof(p));
      const float m = mag(p);
      const float dist2 = m * m;
      if (dist2 < h * h) {
        const float dist = mag(p);
        float dir[3] = {0.f, 0.f, 0.f};
        if (dist > 0.0f) {
          const float inv = 1.0f / dist;
          for (int a = 0; a < 3; ++a) dir[a] = p[a] * inv;
        }
        float o1 = 0.0f;  // O1D, std_kernel.go:54-60
        if (!(dist >= h)) {
          const float q = 1.0f - dist / h;
          const float bq = B * q;
          o1 = bq * q;
        }
        const float s = -o1;
        float g[3];
        for (int a = 0; a < 3; ++a) g[a] = dir[a] * s;
        for (int a = 0; a < 3; ++a) d1[a] = d1[a] + g[a];
        const float t0 = g[0] * g[0], t1 = g[1] * g[1], t2 = g[2] * g[2];
        const float dd = (t0 + t1) + t2;
        d2 += dd;
      }
    }
    {
      const float t0 = d1[0] * d1[0], t1 = d1[1] * d1[1], t2 = d1[2] * d1[2];
      const float dd = (t0 + t1) + t2;
      denom += -dd - d2;
    }
    if (denom != 0.0f) {
      const float t2 = time_ * time_;
      const float m2 = prm_.mass * prm_.mass;
      const float r2 = prm_.ref_density * prm_.ref_density;
      const float beta = t2 * m2 * (2.0f / r2);
      delta_ = -1.0f / (beta * denom);
      return delta_;
    }
    return 0.0f;
  }

 private:
  std::vector<float> read(int buf, int comps) {
    std::vector<float> out((size_t)particles_ * comps);
    ck(dsl_download(h_, buf, out.data(), out.size()));
    return out;
  }
  void release() {
    if (h_) dsl_destroy(h_);
    h_ = nullptr;
  }
  dsl_params prm_{};
  dsl_handle* h_ = nullptr;
  float time_ = 0.0f, cache_life_ = CACHE_L, mu_ = VISCOSITY_WATER, delta_ = 0.0f;
  int particles_ = 0, boundary_ = 0;
  VolumeCollider::Motion motion_{};  // the motion last handed to the library (UpdateMotion / UpdateOrigin)
};

}  // namespace sph

// ---------------------------------------------------------------------------------------
// solver
// ---------------------------------------------------------------------------------------
namespace solver {

// solver/method.go:3-6
struct SPHMethod {
  virtual ~SPHMethod() = default;
  virtual void Run() = 0;
  virtual void Run_(Chan<int>& t) = 0;
};

// solver/wcsph/wcsph.go:9-75.  The reference's loops never terminate; `max_steps` (0 =
// forever) exists so tests can run them.
class WCSPH : public SPHMethod {
 public:
  explicit WCSPH(sph::SPH& core, long max_steps = 0) : core_(core), max_steps_(max_steps) {}
  void Run() override {  // wcsph.go:14-26: DensityAll, ExternalAll, PressureAll, Update, CFL
    for (long s = 0; max_steps_ == 0 || s < max_steps_; ++s) step();
  }
  void Run_(Chan<int>& t) override {  // wcsph.go:35-75
    bool sync = true;
    for (long s = 0; max_steps_ == 0 || s < max_steps_; ++s) {
      if (sync) {
        step();
        const int status = t.recv();
        if (status == THREAD_WAIT) {
          sync = false;
          t.send(SPH_THREAD_WAITING);
          if (t.recv() == THREAD_GO) sync = true;
        }
        if (status == THREAD_GO) sync = true;
        if (status == THREAD_DONE) return;  // addition: a way out for tests
      }
      if (t.recv() == THREAD_GO) sync = true;
    }
  }
  long steps() const { return steps_; }

 private:
  void step() {
    core_.ck(dsl_wcsph_step(core_.handle(), 1));
    core_.CFL();
    ++steps_;
  }
  sph::SPH& core_;
  long max_steps_, steps_ = 0;
};

// solver/pcisph/pcisph_darwin.go:11-118
class PciMethod {
 public:
  explicit PciMethod(sph::SPH* sys) : system_(sys) {}
  // Run(message chan string, hasGL bool, mRender *render.RenderSystem): the GL arguments
  // belong to the renderer (out of scope) and are dropped.
  void Run(Chan<std::string>& message) {
    system_->ck(dsl_pcisph_begin(system_->handle()));  // :28-41
    bool done = false;
    while (!done) {
      system_->ck(dsl_pcisph_step(system_->handle(), 1));  // :43-101
      ++steps_;
      std::string msg;
      if (message.try_recv(msg) && msg == "QUIT") done = true;  // :103-110
      message.try_send("SAMPLER_UPDATE");                        // :112-116
    }
  }
  long steps() const { return steps_; }

 private:
  sph::SPH* system_;
  long steps_ = 0;
};

}  // namespace solver

// ---------------------------------------------------------------------------------------
// compute / compute/gpu
// ---------------------------------------------------------------------------------------
namespace compute {

// compute/compute.go:9-13
struct Descriptor {
  std::vector<int> Work, Local;
  int Size = 0;
};

// compute/gpu/gpu.go:20-425.  Named buffers map onto the engine's device arrays; the
// kernel names are the reference's (pcisph_gpu_darwin.go:133-139) and select built-in HIP
// kernels instead of compiling OpenCL sources.  Methods return an error string (empty =
// nil) where the Go ones return `error`, and bool where they return bool.
class ComputeGPU {
 public:
  ComputeGPU(Descriptor* desc, sph::SPH* system) : desc_(desc), sys_(system) {}
  std::string RegisterBuffer(int bytes_size, int /*t*/, const std::string& name) {  // gpu.go:314-321
    const int id = buffer_id(name);
    if (id == -2) {
      aux_[name] = bytes_size;  // "sizes","floats","sampler","vecs": parameter blocks, no device array
      return "";
    }
    if (id < 0) return "buffer [" + name + "] is not a buffer of this engine";
    registered_[name] = bytes_size;
    return "";
  }
  std::string PassFloatBuffer(const std::vector<float>& cpu, const std::string& name) {  // gpu.go:343-352
    if (aux_.count(name)) return "";
    if (!registered_.count(name)) return "buffer [" + name + "] not registered";  // gpu.go:305-310
    if (dsl_upload(sys_->handle(), buffer_id(name), cpu.data(), cpu.size()) != DSL_OK)
      return dsl_last_error(sys_->handle());
    return "";
  }
  std::string ReadFloatBuffer(std::vector<float>& cpu, const std::string& name) {  // gpu.go:332-341
    if (!registered_.count(name)) return "buffer [" + name + "] not registered";
    if (dsl_download(sys_->handle(), buffer_id(name), cpu.data(), cpu.size()) != DSL_OK)
      return dsl_last_error(sys_->handle());
    return "";
  }
  bool RegisterKernel(const std::string& name) {  // gpu.go:231-250
    const bool ok = name == "compute_density" || name == "predict_correct";
    if (ok) kernels_[name] = true;
    log_ += ok ? "kernel " + name + " registered\n" : "kernel " + name + " unknown\n";
    return ok;
  }
  std::string AddSourceFile(const std::string&) { return ""; }    // gpu.go:257-271: nothing to compile
  std::string BuildProgram(const std::string&) { return ""; }     // gpu.go:194-229
  std::string Queue(const std::string& name) {                    // gpu.go:286-296
    if (!kernels_.count(name)) return "kernel [" + name + "] not registered";
    pending_ = name;
    return "";
  }
  // ---- the rest of compute.GPUCompute (compute/compute.go:26-53) ----
  bool Setup(bool /*gl_interop*/) { return HasDeviceContext(); }   // compute.go:29: the device context is the handle
  // compute.go:33 Run(x chan int): runs the kernel named by the last Queue() -- the reference's two fused
  // device kernels are phases of the PCISPH step here (pci_density.c:12-23 = NN, density, viscosity;
  // pci_predict.c:9-27 = the correction loop + integrate) -- then reports THREAD_DONE / THREAD_ERR
  void Run(Chan<int>& x) {
    int rc = DSL_OK;
    dsl_handle* h = sys_->handle();
    if (pending_ == "compute_density") {
      rc = dsl_pcisph_begin(h);  // (re-copies the predictor state only the first time it is needed)
      if (rc == DSL_OK) rc = dsl_pcisph_phase(h, DSL_PCI_BEGIN_STEP);
    } else if (pending_ == "predict_correct") {
      for (int it = 0; rc == DSL_OK && it < sys_->params().pci_max_iters; ++it) {
        rc = dsl_pcisph_phase(h, DSL_PCI_ITERATE);
        if (rc == DSL_OK) rc = dsl_pcisph_phase(h, DSL_PCI_CHECK);
      }
      if (rc == DSL_OK) rc = dsl_pcisph_phase(h, DSL_PCI_END_STEP);
    } else {
      rc = DSL_ERR_INVALID;
    }
    if (rc == DSL_OK) rc = dsl_sync(h);
    x.send(rc == DSL_OK ? THREAD_DONE : THREAD_ERR);
  }
  // gpu.go:354-378.  "sizes" = {N, Nboundary, buckets, bucket_size} (pcisph_gpu_darwin.go:60): checked
  // against the engine's parameters instead of being dropped; "sampler" = the host's flattened LSH
  // table (lsh.go:70-80): the engine builds its own neighbour table, the upload is accepted and ignored.
  std::string PassIntBuffer(const std::vector<int>& cpu, const std::string& name) {
    if (!aux_.count(name) && !registered_.count(name)) return "buffer [" + name + "] not registered";
    if (name == "sizes") {
      const dsl_params& p = sys_->params();
      if (cpu.size() < 2 || cpu[0] != p.n_particles || cpu[1] != p.n_boundary)
        return "sizes block {N, Nboundary, ..} does not match the engine's parameters";
    }
    log_ += "Passed Integer Buffer " + name + "\n";
    return "";
  }
  std::string ReadIntBuffer(std::vector<int>& cpu, const std::string& name) {
    if (!aux_.count(name) && !registered_.count(name)) return "buffer [" + name + "] not registered";
    const dsl_params& p = sys_->params();
    if (name == "sizes") {
      const int v[4] = {p.n_particles, p.n_boundary, p.lsh_buckets, p.lsh_bucket_size};
      for (size_t k = 0; k < cpu.size() && k < 4; ++k) cpu[k] = v[k];
      return "";
    }
    if (name == "sampler") {  // HashSampler.GetData1D (DSL_NEIGH_LSH_REF handles only)
      std::vector<int32_t> t(cpu.size());
      if (dsl_lsh_download_table(sys_->handle(), t.data(), t.size()) != DSL_OK) return dsl_last_error(sys_->handle());
      for (size_t k = 0; k < cpu.size(); ++k) cpu[k] = t[k];
      return "";
    }
    return "buffer [" + name + "] holds no integers";
  }
  // gpu.go:378-390 PassLayoutBuffer for the two parameter blocks of pcisph_gpu_darwin.go:60-61
  std::string PassLayoutBuffer(const void* data, int bytes, const std::string& name) {
    if (!aux_.count(name)) return "buffer [" + name + "] not registered";
    const dsl_params& p = sys_->params();
    if (name == "floats" && bytes >= 20) {  // {dt, mass, delta, maxVel, h}
      const float* f = static_cast<const float*>(data);
      if (f[0] != p.dt || f[1] != p.mass || f[4] != p.h) return "floats block {dt, mass, delta, maxVel, h} does not match the engine's parameters";
    }
    if (name == "sizes" && bytes >= 8) {
      const int32_t* v = static_cast<const int32_t*>(data);
      if (v[0] != p.n_particles || v[1] != p.n_boundary) return "sizes block {N, Nboundary, ..} does not match the engine's parameters";
    }
    log_ += "Passed Layout Buffer " + name + "\n";
    return "";
  }
  std::string AddSourceString(const std::string&) { return ""; }  // compute.go:46: nothing to compile
  // gpu.go:323-330 RegisterGLBuffer shares a GL buffer with the device queue so that the renderer draws what
  // the solver wrote without a read-back.  The counterpart here is the other way round: the consumer is
  // handed the live device arrays (dsl_device_pointers); the GL id is recorded, nothing is mapped.
  std::string RegisterGLBuffer(uint32_t gl_buffer_id, int size, const std::string& name) {
    if (buffer_id(name) != DSL_BUF_POSITIONS) return "only the positions buffer has a render hand-off";
    registered_[name] = size;
    log_ += "RegisterGLBuffer() - buffer " + name + " (GL id " + std::to_string(gl_buffer_id) +
            "): read the device arrays through DevicePointers()\n";
    return "";
  }
  // the live SoA device arrays of the positions (x, y, z), slot -> particle id map, slot count
  std::string DevicePointers(const float* xyz[3], const int32_t** ids, int* n) {
    if (dsl_device_pointers(sys_->handle(), DSL_BUF_POSITIONS, xyz, ids, n) != DSL_OK) return dsl_last_error(sys_->handle());
    return "";
  }
  void Set(const Descriptor& d) { *desc_ = d; }     // gpu.go:298-300
  Descriptor Get() const { return *desc_; }         // gpu.go:301-303
  bool HasDeviceContext() const { return sys_ && sys_->handle(); }  // gpu.go:392-398
  bool ValidState() const { return HasDeviceContext(); }            // gpu.go:400-405
  const std::string& Log() const { return log_; }                   // gpu.go:421-425
  sph::SPH* system() { return sys_; }

 private:
  static int buffer_id(const std::string& n) {  // names of pcisph_gpu_darwin.go:67-76
    if (n == "positions") return DSL_BUF_POSITIONS;
    if (n == "velocities") return DSL_BUF_VELOCITIES;
    if (n == "forces") return DSL_BUF_FORCES;
    if (n == "densities") return DSL_BUF_DENSITIES;
    if (n == "pressures") return DSL_BUF_PRESSURES;
    if (n == "temps") return DSL_BUF_PCI_POSITIONS;
    if (n == "sizes" || n == "floats" || n == "sampler" || n == "vecs") return -2;
    return -1;
  }
  Descriptor* desc_;
  sph::SPH* sys_;
  std::map<std::string, int> registered_, aux_;
  std::map<std::string, bool> kernels_;
  std::string pending_, log_;
};

}  // namespace compute

namespace solver {

// solver/pcisph/pcisph_gpu_darwin.go:22-286
class GPUPredictorCorrector {
 public:
  // New_GPUPredictorCorrector(computeGPU, sph, opencl, gl_position_buffer) :36-236
  GPUPredictorCorrector(compute::ComputeGPU* gpu, sph::SPH* system) : gpu_(gpu), system_(system) {
    const int n = system_->N();
    const char* names[] = {"positions", "velocities", "forces", "densities", "pressures"};
    const int bytes[] = {n * 12, n * 12, n * 12, n * 4, n * 4};
    for (int k = 0; k < 5; ++k) must(gpu_->RegisterBuffer(bytes[k], 0, names[k]));  // :67-71
    must(gpu_->RegisterBuffer(4 * 4, 0, "sizes"));                                   // :72
    must(gpu_->RegisterBuffer(5 * 4, 0, "floats"));                                  // :73
    must(gpu_->RegisterBuffer(n * 7 * 4, 0, "temps"));                               // :76
    if (!gpu_->RegisterKernel("compute_density")) throw Error("Register kernel compute density failed");   // :133
    if (!gpu_->RegisterKernel("predict_correct")) throw Error("Register kernel predict_correct failed");  // :137
    system_->ck(dsl_pcisph_begin(system_->handle()));
  }
  // MemoryRequirements() :238-246 (the reference's formula, units as printed there)
  std::string MemoryRequirements() const {
    const int particles = system_->N(), boundary = 0, total = particles;
    const double kb = (double)((total * 4 * 3) + (particles * 4 * 3 * 2) + (2 * particles * 4) / 1024);
    char buf[160];
    std::snprintf(buf, sizeof(buf), "Fluid GPU PCI (Fluid Particles[%d]  Boundary[%d]\nAllocated %.2fkB (%.2fMB)\n\n",
                  particles, boundary, kb, kb * 0.001);
    return buf;
  }
  // Run(message *chan string) error :249-286.  One cycle = both reference kernels
  // (compute_density, predict_correct) = one dsl_pcisph_step, then the blocking position
  // read-back and "CL_REFRESH".  `max_cycles` (0 = forever) lets tests stop the loop.
  std::string Run(Chan<std::string>* message, std::vector<float>* positions, long max_cycles = 0) {
    for (long c = 0; max_cycles == 0 || c < max_cycles; ++c) {
      system_->CFL();        // :253
      system_->CacheIncr();  // :254 (NN every 4th call; the engine also rebuilds every step)
      if (dsl_pcisph_step(system_->handle(), 1) != DSL_OK) return dsl_last_error(system_->handle());  // :256-274
      if (positions) {
        positions->resize((size_t)system_->N() * 3);
        if (dsl_download(system_->handle(), DSL_BUF_POSITIONS, positions->data(), positions->size()) != DSL_OK)
          return dsl_last_error(system_->handle());                                                   // :276-277
      }
      if (message) message->send("CL_REFRESH");                                                       // :279
    }
    return "";
  }

 private:
  static void must(const std::string& e) {
    if (!e.empty()) throw Error(e);
  }
  compute::ComputeGPU* gpu_;
  sph::SPH* system_;
};

}  // namespace solver
}  // namespace dsl
