// record_host_check.cpp -- tests/test_gpu_record_host.py: the C++ mirror's frame recorder (dieselfluid.hpp: SPH::Recorder and
// its calls) on sph.Init's lattice: a recorder of float32 positions, velocities and densities every second step, six WCSPH
// steps in one call (frames at steps 0, 2 and 4), one frame by hand at step 6, a Q16 recorder with every third particle and
// two more steps (frames at steps 6 and 7).  The first frame leaves through NextFrame, the others through WriteAnimation.
// usage: record_host_check FRAME0 ANIMATION n3
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../dieselfluid_amd/host/dieselfluid.hpp"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  try {
    using SPH = dsl::sph::SPH;
    SPH core = SPH::Init(1.0f, std::vector<float>{0.f, 0.f, 0.f}, nullptr, std::atoi(argv[3]), false, 0, DSL_MATH_EXACT, 0);
    SPH::Recorder rec;
    rec.Every = 2, rec.Velocities = rec.Densities = true, rec.Slots = 8;
    core.SetRecorder(rec);
    core.ck(dsl_wcsph_step(core.handle(), 6));
    core.RecordNow();
    core.ck(dsl_sync(core.handle()));
    int64_t ready = 0, dropped = 0;
    if (core.PollFrames(&ready, &dropped) != 4 || ready != 4 || dropped != 0) return 5;
    const std::vector<unsigned char> first = core.NextFrame();
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(first.data(), 1, first.size(), f) != first.size() || std::fclose(f) != 0) return 7;
    if (core.WriteAnimation(argv[2]) != 3) return 6;
    SPH::Recorder q;
    q.Stride = 3, q.Velocities = true, q.Q16 = true, q.FirstStep = 6, q.Slots = 2;
    core.SetRecorder(q);
    core.ck(dsl_wcsph_step(core.handle(), 2));
    if (core.WriteAnimation(argv[2], true) != 2) return 6;
    if (core.PollFrames(&ready) != 2 || ready != 0) return 5;
    core.ClearRecorder();
    std::printf("record_host_check ok N %d\n", core.N());
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "record_host_check: %s\n", e.what());
    return 1;
  }
}
