// bodies_host_check.cpp -- tests/test_gpu_bodies_host.py: the C++ mirror's rigid bodies (dieselfluid.hpp: SPH::Body,
// SPH::Bodies) on sph.Init's lattice: two bodies from one volume, the query against the second, one collide pass, every
// body's reading, two WCSPH steps (which integrate the poses), the readings again, a state update, and the clear.
// usage: bodies_host_check IN OUT n3
// IN: int32 dims[3], float origin[3], step[3], then per body (two of them) 9 floats of props (inv_mass, inv_inertia[3],
// accel[3], radius, restitution) and 13 of state (quat[4], trans[3], lin_vel[3], ang_vel[3]), then the voxels.  OUT: int64 N,
// then 3 N floats (positions before), N (dist), 3 N (normal), 3 N (positions after the pass), 3 N (velocities after), per body
// 19 (state, impulse, torque), then after the steps 3 N (positions) and per body 19 again
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dieselfluid_amd/host/dieselfluid.hpp"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  try {
    using SPH = dsl::sph::SPH;
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    SPH::Body body[2];
    SPH::DistanceVolume vol;
    if (std::fread(vol.dims, 4, 3, in) != 3 || std::fread(vol.origin, 4, 3, in) != 3 || std::fread(vol.step, 4, 3, in) != 3) return 4;
    for (SPH::Body& b : body) {
      if (std::fread(&b.InvMass, 4, 1, in) != 1 || std::fread(b.InvInertia, 4, 3, in) != 3 || std::fread(b.Accel, 4, 3, in) != 3 ||
          std::fread(&b.Radius, 4, 1, in) != 1 || std::fread(&b.Restitution, 4, 1, in) != 1 || std::fread(b.Pose.Quat, 4, 4, in) != 4 ||
          std::fread(b.Pose.Origin, 4, 3, in) != 3 || std::fread(b.Pose.LinVel, 4, 3, in) != 3 || std::fread(b.Pose.AngVel, 4, 3, in) != 3)
        return 4;
    }
    vol.Values.resize((size_t)vol.dims[0] * vol.dims[1] * vol.dims[2]);
    if (std::fread(vol.Values.data(), 4, vol.Values.size(), in) != vol.Values.size()) return 4;
    std::fclose(in);
    body[0].Volume = body[1].Volume = vol;
    SPH core = SPH::Init(1.0f, std::vector<float>{0.f, 0.f, 0.f}, nullptr, std::atoi(argv[3]), false);
    const size_t N = (size_t)core.N();
    std::vector<float> before(3 * N), after(3 * N), vel(3 * N), stepped(3 * N), dist, normal;
    core.ck(dsl_download(core.handle(), DSL_BUF_POSITIONS, before.data(), before.size()));
    SPH::Bodies bodies = core.RigidBodies();
    if (bodies.Count() != 0) return 5;
    if (bodies.Add(body[0]) != 0 || bodies.Add(body[1]) != 1 || bodies.Count() != 2) return 5;
    bodies.Distances(1, &dist, &normal);
    core.ck(dsl_collide_pass(core.handle()));
    core.ck(dsl_download(core.handle(), DSL_BUF_POSITIONS, after.data(), after.size()));
    core.ck(dsl_download(core.handle(), DSL_BUF_VELOCITIES, vel.data(), vel.size()));
    const SPH::BodyReading first[2] = {bodies.Get(0), bodies.Get(1)};
    core.ck(dsl_wcsph_step(core.handle(), 2));
    core.ck(dsl_download(core.handle(), DSL_BUF_POSITIONS, stepped.data(), stepped.size()));
    const SPH::BodyReading second[2] = {bodies.Get(0, true), bodies.Get(1)};
    const SPH::BodyReading zeroed = bodies.Get(0);
    for (int a = 0; a < 3; ++a)
      if (zeroed.Momentum.Impulse[a] != 0.f || zeroed.Momentum.Torque[a] != 0.f) return 6;
    bodies.Update(1, body[1].Pose);  // back where it started
    const SPH::BodyReading back = bodies.Get(1);
    for (int a = 0; a < 3; ++a)
      if (back.Pose.Origin[a] != body[1].Pose.Origin[a] || back.Pose.LinVel[a] != body[1].Pose.LinVel[a]) return 6;
    bodies.UpdateProps(0, body[1]);
    bodies.Integrate(false);
    bodies.Clear();
    if (bodies.Count() != 0) return 6;
    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 7;
    const int64_t head = (int64_t)N;
    std::fwrite(&head, sizeof(head), 1, f);
    auto reading = [&](const SPH::BodyReading& r) {
      std::fwrite(r.Pose.Quat, 4, 4, f);
      std::fwrite(r.Pose.Origin, 4, 3, f);
      std::fwrite(r.Pose.LinVel, 4, 3, f);
      std::fwrite(r.Pose.AngVel, 4, 3, f);
      std::fwrite(r.Momentum.Impulse, 4, 3, f);
      std::fwrite(r.Momentum.Torque, 4, 3, f);
    };
    for (const std::vector<float>* a : {&before, &dist, &normal, &after, &vel}) std::fwrite(a->data(), 4, a->size(), f);
    for (const SPH::BodyReading& r : first) reading(r);
    std::fwrite(stepped.data(), 4, stepped.size(), f);
    for (const SPH::BodyReading& r : second) reading(r);
    std::fclose(f);
    std::printf("bodies_host_check ok N %lld\n", (long long)head);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "bodies_host_check: %s\n", e.what());
    return 1;
  }
}
