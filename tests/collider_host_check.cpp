// Drives the C++ host mirror's mesh::InitMesh and Mesh::Collision (dieselfluid_amd/host/dieselfluid.hpp) on the cases
// tests/test_collider_cpu.py writes, so that the test can compare them with tests/collider_ref.py bit for bit.
// Input file (binary): int32 T, int32 N, int32 use_init, float dt, float r, float origin[3], 9T vertex floats,
// 3T normal floats, 3N positions, 3N velocities.  Output file: 3T normals used, then per particle int32 tri and 9 floats
// (normal, coord, point).  No device is touched.
#include <cstdio>
#include <vector>

#include "../dieselfluid_amd/host/dieselfluid.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int hdr[3];
  float scal[5];
  if (std::fread(hdr, 4, 3, in) != 3 || std::fread(scal, 4, 5, in) != 5) return 4;
  const int T = hdr[0], N = hdr[1];
  std::vector<float> v((size_t)9 * T), n((size_t)3 * T), P((size_t)3 * N), V((size_t)3 * N);
  if (std::fread(v.data(), 4, v.size(), in) != v.size() || std::fread(n.data(), 4, n.size(), in) != n.size() ||
      std::fread(P.data(), 4, P.size(), in) != P.size() || std::fread(V.data(), 4, V.size(), in) != V.size())
    return 5;
  std::fclose(in);
  std::vector<dsl::mesh::Vec> verts((size_t)3 * T);
  for (size_t k = 0; k < verts.size(); ++k) verts[k] = {v[3 * k], v[3 * k + 1], v[3 * k + 2]};
  dsl::mesh::Mesh m;
  if (hdr[2]) {
    m = dsl::mesh::InitMesh(verts, {scal[2], scal[3], scal[4]});
  } else {
    m.Vertexes = verts;
    m.Normals.resize((size_t)T);
    for (int t = 0; t < T; ++t) m.Normals[(size_t)t] = {n[3 * t], n[3 * t + 1], n[3 * t + 2]};
  }
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 6;
  for (int t = 0; t < T; ++t) std::fwrite(m.Normals[(size_t)t].data(), 4, 3, out);
  for (int i = 0; i < N; ++i) {
    const dsl::mesh::CollisionResult c =
        m.Collision({P[3 * i], P[3 * i + 1], P[3 * i + 2]}, {V[3 * i], V[3 * i + 1], V[3 * i + 2]}, (double)scal[0], scal[1]);
    const int tri = c.collision ? c.tri : -1;
    std::fwrite(&tri, 4, 1, out);
    std::fwrite(c.normal.data(), 4, 3, out);
    std::fwrite(c.coord.data(), 4, 3, out);
    std::fwrite(c.point.data(), 4, 3, out);
  }
  std::fclose(out);
  return 0;
}
