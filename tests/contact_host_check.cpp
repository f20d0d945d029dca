// contact_host_check.cpp -- tests/test_gpu_contact_host.py: the C++ mirror's contact stage (dieselfluid.hpp: SPH::Bodies::
// ContactPoints, ContactPass, ContactTable, Contact, Contacts) on sph.Init's lattice: two overlapping bodies from one volume,
// the first body's contact points, one detection with its solve, the table, every body's reading, then the option and two
// WCSPH steps, the table and the readings again.
// usage: contact_host_check IN OUT n3
// IN: int32 dims[3], float origin[3], step[3], then per body (two of them) 9 floats of props and 13 of state, then the voxels.
// OUT: int64 N, int64 M, then M int32 (points), 144 floats (table), per body 13 (state), int32 contacts; after the steps 144
// (table), per body 13, int32 contacts
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
    SPH::Bodies bodies = core.RigidBodies();
    if (bodies.Add(body[0]) != 0 || bodies.Add(body[1]) != 1) return 5;
    if (bodies.Contacts() != 0) return 5;
    const std::vector<int32_t> points = bodies.ContactPoints(0);
    bodies.ContactPass(3, true);
    const std::vector<float> first_table = bodies.ContactTable();
    const SPH::BodyReading first[2] = {bodies.Get(0), bodies.Get(1)};
    const int32_t first_contacts = bodies.Contacts();
    bodies.Contact(2);
    core.ck(dsl_wcsph_step(core.handle(), 2));
    const std::vector<float> second_table = bodies.ContactTable();
    const SPH::BodyReading second[2] = {bodies.Get(0), bodies.Get(1)};
    const int32_t second_contacts = bodies.Contacts();
    bodies.Contact(0);
    bodies.Clear();
    if (first_table.size() != 144 || second_table.size() != 144) return 6;
    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 7;
    const int64_t head[2] = {(int64_t)core.N(), (int64_t)points.size()};
    std::fwrite(head, sizeof(head[0]), 2, f);
    std::fwrite(points.data(), 4, points.size(), f);
    auto reading = [&](const SPH::BodyReading& r) {
      std::fwrite(r.Pose.Quat, 4, 4, f);
      std::fwrite(r.Pose.Origin, 4, 3, f);
      std::fwrite(r.Pose.LinVel, 4, 3, f);
      std::fwrite(r.Pose.AngVel, 4, 3, f);
    };
    std::fwrite(first_table.data(), 4, first_table.size(), f);
    for (const SPH::BodyReading& r : first) reading(r);
    std::fwrite(&first_contacts, 4, 1, f);
    std::fwrite(second_table.data(), 4, second_table.size(), f);
    for (const SPH::BodyReading& r : second) reading(r);
    std::fwrite(&second_contacts, 4, 1, f);
    std::fclose(f);
    std::printf("contact_host_check ok M %lld\n", (long long)head[1]);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "contact_host_check: %s\n", e.what());
    return 1;
  }
}
