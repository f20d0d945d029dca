// sources_host_check.cpp -- tests/test_gpu_sources_host.py: the C++ mirror's sources and sinks (dieselfluid.hpp: SPH::Emitter,
// SPH::Sink and their calls) fill and drain a small tank: sph.Init's lattice with room for more, a 5 x 4 face above it that emits
// a layer per step, an outlet under the lowest lattice layer that the drivers apply every second step, six WCSPH steps one at
// a time, then one layer by hand, three appended particles, one removal by hand, and the clear calls.
// usage: sources_host_check OUT n3 room
// OUT: int64 counts[10] (N after each of the six steps, after the emit, after the append, after the removal; then what the
// removal returned), then 3 N floats (positions) and 3 N (velocities) of the final state
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../dieselfluid_amd/host/dieselfluid.hpp"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  try {
    using SPH = dsl::sph::SPH;
    SPH core = SPH::Init(1.0f, std::vector<float>{0.f, 0.f, 0.f}, nullptr, std::atoi(argv[2]), false, 0, DSL_MATH_EXACT, std::atoi(argv[3]));
    const float inf = std::numeric_limits<float>::infinity();
    SPH::Emitter face;
    const float origin[3] = {-0.7f, 1.25f, -0.5f}, u[3] = {0.33f, 0.0f, 0.02f}, v[3] = {0.01f, 0.0f, 0.34f}, vel[3] = {0.0f, -20.0f, 0.0f};
    for (int a = 0; a < 3; ++a) face.Origin[a] = origin[a], face.U[a] = u[a], face.V[a] = v[a], face.Velocity[a] = vel[a];
    face.Nu = 5, face.Nv = 4;
    SPH::Sink outlet;
    for (int a = 0; a < 3; ++a) outlet.Min[a] = -inf, outlet.Max[a] = inf;
    outlet.Max[1] = -0.9f;
    if (core.AddEmitter(face) != 0 || core.AddSink(outlet) != 0) return 5;
    core.SinkEvery(2);
    std::vector<int64_t> counts;
    for (int s = 0; s < 6; ++s) {
      core.ck(dsl_wcsph_step(core.handle(), 1));
      counts.push_back(core.SyncCount());
    }
    core.Emit(0);
    counts.push_back(core.N());
    core.AppendParticles({2.5f, -0.95f, 0.0f, 2.5f, 0.5f, 0.0f, 2.5f, 0.0f, 0.5f}, {0.f, 1.f, 0.f, 0.f, 2.f, 0.f, 0.f, 3.f, 0.f});
    counts.push_back(core.N());
    const int64_t gone = core.RemoveParticles();
    counts.push_back(core.N());
    counts.push_back(gone);
    core.ClearEmitters();
    core.ClearSinks();
    core.ck(dsl_wcsph_step(core.handle(), 1));
    if (core.SyncCount() != (int)counts[8]) return 6;  // (nothing emits or drains any more)
    const std::vector<float> pos = core.Positions(), velocities = core.Velocities();
    if (pos.size() != 3 * (size_t)core.N() || velocities.size() != pos.size()) return 6;
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 7;
    std::fwrite(counts.data(), sizeof(int64_t), counts.size(), f);
    std::fwrite(pos.data(), 4, pos.size(), f);
    std::fwrite(velocities.data(), 4, velocities.size(), f);
    std::fclose(f);
    std::printf("sources_host_check ok N %d\n", core.N());
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "sources_host_check: %s\n", e.what());
    return 1;
  }
}
