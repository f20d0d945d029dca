// surface_mesh_host_check.cpp -- tests/test_gpu_surface_mesh_host.py: one call of the C++ mirror's SPH::SurfaceIndexed
// (dieselfluid.hpp), next to the volume it was made from.  usage: surface_mesh_host_check OUT n3 iso_over_rho0 ox oy oz sx sy sz nx ny nz
// OUT: int64 V, int64 T, int64 voxels, then voxels floats (dsl_field_volume), 3 V floats (Positions), 3 V floats (Normals),
// 3 T int32 (Indices)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dieselfluid_amd/host/dieselfluid.hpp"

int main(int argc, char** argv) {
  if (argc != 13) return 2;
  try {
    const int n3 = std::atoi(argv[2]);
    const float origin[3] = {(float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6])};
    const float step[3] = {(float)std::atof(argv[7]), (float)std::atof(argv[8]), (float)std::atof(argv[9])};
    const int32_t dims[3] = {std::atoi(argv[10]), std::atoi(argv[11]), std::atoi(argv[12])};
    dsl::sph::SPH core = dsl::sph::SPH::Init(1.0f, std::vector<float>{0.f, 0.f, 0.f}, nullptr, n3, false);
    const float iso = (float)std::atof(argv[3]) * core.params().ref_density;
    const dsl::sph::SPH::IndexedMesh m = core.SurfaceIndexed(origin, step, dims, iso);
    if (m.Positions.size() != m.Normals.size() || m.Indices.size() % 3 != 0) return 3;
    std::vector<float> vol((size_t)dims[0] * dims[1] * dims[2]);
    core.ck(dsl_field_volume(core.handle(), DSL_BUF_DENSITIES, origin, step, dims, nullptr, vol.data()));
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 4;
    const int64_t head[3] = {(int64_t)m.Positions.size(), (int64_t)(m.Indices.size() / 3), (int64_t)vol.size()};
    std::fwrite(head, sizeof(head), 1, f);
    std::fwrite(vol.data(), sizeof(float), vol.size(), f);
    for (const dsl::mesh::Vec& v : m.Positions) std::fwrite(v.data(), sizeof(float), 3, f);
    for (const dsl::mesh::Vec& n : m.Normals) std::fwrite(n.data(), sizeof(float), 3, f);
    std::fwrite(m.Indices.data(), sizeof(int32_t), m.Indices.size(), f);
    std::fclose(f);
    std::printf("surface_mesh_host_check ok V %lld T %lld\n", (long long)head[0], (long long)head[1]);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "surface_mesh_host_check: %s\n", e.what());
    return 1;
  }
}
