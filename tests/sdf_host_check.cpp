// sdf_host_check.cpp -- tests/test_gpu_sdf_host.py: the C++ mirror's SPH::MeshDistance, SPH::Collider(VolumeCollider) and
// SPH::ColliderDistances (dieselfluid.hpp) on sph.Init's lattice, then one collide pass.
// usage: sdf_host_check MESH OUT n3 band radius restitution ox oy oz sx sy sz nx ny nz
// MESH: int32 T, 9 T floats.  OUT: int64 voxels, int64 N, then voxels floats (the volume), 3 N (positions before), N (dist),
// 3 N (normal), 3 N (positions after the pass), 3 N (velocities after)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dieselfluid_amd/host/dieselfluid.hpp"

int main(int argc, char** argv) {
  if (argc != 16) return 2;
  try {
    std::FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 3;
    int32_t T = 0;
    if (std::fread(&T, 4, 1, in) != 1 || T < 1) return 4;
    std::vector<float> v((size_t)9 * T);
    if (std::fread(v.data(), 4, v.size(), in) != v.size()) return 4;
    std::fclose(in);
    dsl::mesh::Mesh m;
    m.Vertexes.resize((size_t)3 * T);
    for (size_t k = 0; k < m.Vertexes.size(); ++k) m.Vertexes[k] = {v[3 * k], v[3 * k + 1], v[3 * k + 2]};
    const int n3 = std::atoi(argv[3]);
    const float band = (float)std::atof(argv[4]), radius = (float)std::atof(argv[5]), rest = (float)std::atof(argv[6]);
    const float origin[3] = {(float)std::atof(argv[7]), (float)std::atof(argv[8]), (float)std::atof(argv[9])};
    const float step[3] = {(float)std::atof(argv[10]), (float)std::atof(argv[11]), (float)std::atof(argv[12])};
    const int32_t dims[3] = {std::atoi(argv[13]), std::atoi(argv[14]), std::atoi(argv[15])};
    dsl::sph::SPH core = dsl::sph::SPH::Init(1.0f, std::vector<float>{0.f, 0.f, 0.f}, nullptr, n3, false);
    dsl::sph::SPH::VolumeCollider col;
    col.Volume = core.MeshDistance(m, origin, step, dims, band);
    col.Radius = radius;
    col.Restitution = rest;
    if (col.Volume.Values.size() != (size_t)dims[0] * dims[1] * dims[2]) return 5;
    const size_t N = (size_t)core.N();
    std::vector<float> before(3 * N), after(3 * N), vel(3 * N), dist, normal;
    core.ck(dsl_download(core.handle(), DSL_BUF_POSITIONS, before.data(), before.size()));
    core.Collider(col);
    core.ColliderDistances(&dist, &normal);
    core.ck(dsl_collide_pass(core.handle()));
    core.ck(dsl_download(core.handle(), DSL_BUF_POSITIONS, after.data(), after.size()));
    core.ck(dsl_download(core.handle(), DSL_BUF_VELOCITIES, vel.data(), vel.size()));
    core.RemoveVolumeCollider();
    double voxels = -1.0;
    core.ck(dsl_get_option(core.handle(), DSL_OPT_COLLIDER_VOLUME, &voxels));
    if (voxels != 0.0) return 6;
    std::FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 7;
    const int64_t head[2] = {(int64_t)col.Volume.Values.size(), (int64_t)N};
    std::fwrite(head, sizeof(head), 1, f);
    for (const std::vector<float>* a : {&col.Volume.Values, &before, &dist, &normal, &after, &vel}) std::fwrite(a->data(), 4, a->size(), f);
    std::fclose(f);
    std::printf("sdf_host_check ok voxels %lld N %lld\n", (long long)head[0], (long long)head[1]);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sdf_host_check: %s\n", e.what());
    return 1;
  }
}
