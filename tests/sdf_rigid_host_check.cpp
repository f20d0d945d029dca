// sdf_rigid_host_check.cpp -- tests/test_gpu_sdf_rigid_host.py: the C++ mirror's moving volume collider (dieselfluid.hpp:
// SPH::VolumeCollider::Motion, SPH::UpdateMotion / UpdateOrigin / ClearMotion / IsStatic, SPH::Impulse) on sph.Init's lattice:
// the query at the pose, one collide pass, the impulse read, read with a reset, and read again.
// usage: sdf_rigid_host_check IN OUT n3 radius restitution
// IN: int32 dims[3], float origin[3], step[3], rot[9], trans[3], lin_vel[3], ang_vel[3], then the voxels.  OUT: int64 N, then
// 3 N floats (positions before), N (dist), 3 N (normal), 3 N (positions after the pass), 3 N (velocities after), 6 (impulse
// and torque), 6 (the same, read with reset), 6 (after the reset)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dieselfluid_amd/host/dieselfluid.hpp"

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  try {
    using SPH = dsl::sph::SPH;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    SPH::VolumeCollider col;
    SPH::VolumeCollider::Motion mo;
    if (std::fread(col.Volume.dims, 4, 3, in) != 3 || std::fread(col.Volume.origin, 4, 3, in) != 3 ||
        std::fread(col.Volume.step, 4, 3, in) != 3 || std::fread(mo.Rot, 4, 9, in) != 9 || std::fread(mo.Origin, 4, 3, in) != 3 ||
        std::fread(mo.LinVel, 4, 3, in) != 3 || std::fread(mo.AngVel, 4, 3, in) != 3)
      return 4;
    col.Volume.Values.resize((size_t)col.Volume.dims[0] * col.Volume.dims[1] * col.Volume.dims[2]);
    if (std::fread(col.Volume.Values.data(), 4, col.Volume.Values.size(), in) != col.Volume.Values.size()) return 4;
    std::fclose(in);
    const int n3 = std::atoi(argv[3]);
    col.Radius = (float)std::atof(argv[4]);
    col.Restitution = (float)std::atof(argv[5]);
    SPH core = SPH::Init(1.0f, std::vector<float>{0.f, 0.f, 0.f}, nullptr, n3, false);
    const size_t N = (size_t)core.N();
    std::vector<float> before(3 * N), after(3 * N), vel(3 * N), dist, normal;
    core.ck(dsl_download(core.handle(), DSL_BUF_POSITIONS, before.data(), before.size()));
    core.Collider(col);
    if (!core.IsStatic()) return 5;
    core.UpdateOrigin(mo.Origin);  // Collider.UpdateOrigin: a translation alone
    if (core.IsStatic()) return 5;
    core.ClearMotion();
    if (!core.IsStatic()) return 5;
    SPH::VolumeCollider::Motion elsewhere = mo;  // the orientation and the velocities first, somewhere else ...
    for (int a = 0; a < 3; ++a) elsewhere.Origin[a] = 0.f;
    core.UpdateMotion(elsewhere);
    if (core.IsStatic()) return 5;
    core.UpdateOrigin(mo.Origin);  // ... then the origin alone: the orientation and the velocities stay
    for (int a = 0; a < 9; ++a)
      if (core.Motion().Rot[a] != mo.Rot[a]) return 5;
    if (core.IsStatic()) return 5;
    core.ColliderDistances(&dist, &normal);
    core.ck(dsl_collide_pass(core.handle()));
    core.ck(dsl_download(core.handle(), DSL_BUF_POSITIONS, after.data(), after.size()));
    core.ck(dsl_download(core.handle(), DSL_BUF_VELOCITIES, vel.data(), vel.size()));
    const SPH::VolumeCollider::Momentum kept = core.Impulse(), taken = core.Impulse(true), left = core.Impulse();
    core.RemoveVolumeCollider();
    if (!core.IsStatic()) return 6;
    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 7;
    const int64_t head = (int64_t)N;
    std::fwrite(&head, sizeof(head), 1, f);
    for (const std::vector<float>* a : {&before, &dist, &normal, &after, &vel}) std::fwrite(a->data(), 4, a->size(), f);
    for (const SPH::VolumeCollider::Momentum* m : {&kept, &taken, &left}) {
      std::fwrite(m->Impulse, 4, 3, f);
      std::fwrite(m->Torque, 4, 3, f);
    }
    std::fclose(f);
    std::printf("sdf_rigid_host_check ok N %lld\n", (long long)head);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sdf_rigid_host_check: %s\n", e.what());
    return 1;
  }
}
