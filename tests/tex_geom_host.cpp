// Host program over csrc/tex_geom.h for tests/test_texture_cpu.py: the texel geometry of a small atlas and the atlas
// coordinates of given surface points, computed by the very inline functions the kernels call, written as raw bytes.
//   tex_geom_host <in> <out>
//   in : int32 F, K, c, m; float32 tris [F, 9]; float32 points [m, 3]; int32 ids [m]
//   out: int32 face [S*S]; float32 position [S*S, 3]; normal [S*S, 3]; bary [S*S, 3]; uv [m, 2]
#include <cstdio>
#include <vector>

#include "tex_geom.h"

using namespace lnrf::tex;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int32_t head[4];
  if (fread(head, 4, 4, in) != 4) return 4;
  const Atlas at{head[0], head[1], head[2], head[1] * head[2]};
  const int m = head[3];
  if (!atlas_ok(&at) || m < 0) return 5;
  std::vector<float> tris(9 * (size_t)at.faces), points(3 * (size_t)m);
  std::vector<int32_t> ids(m);
  if (fread(tris.data(), 4, tris.size(), in) != tris.size()) return 4;
  if (fread(points.data(), 4, points.size(), in) != points.size()) return 4;
  if (fread(ids.data(), 4, ids.size(), in) != ids.size()) return 4;
  fclose(in);

  const size_t n = (size_t)at.size * at.size;
  std::vector<int32_t> face(n);
  std::vector<float> position(3 * n, 0.0f), normal(3 * n, 0.0f), bary(3 * n, 0.0f), uv(2 * (size_t)m);
  for (int y = 0; y < at.size; ++y)
    for (int x = 0; x < at.size; ++x) {
      const size_t o = (size_t)y * at.size + x;
      int i, j;
      const int f = texel_face(at, x, y, &i, &j);
      face[o] = f;
      if (f < 0) continue;
      const Frame fr = face_frame(tris.data() + 9 * (size_t)f);
      float bb, bc;
      texel_bary(at.cell, f & 1, i, j, bb, bc);
      surface_point(fr, bb, bc, &position[3 * o]);
      unit_normal(fr, &normal[3 * o]);
      bary_in_face_order(fr, bb, bc, &bary[3 * o]);
    }
  for (int s = 0; s < m; ++s) {
    if (ids[s] < 0 || ids[s] >= at.faces) return 6;
    point_uv(at, ids[s], face_frame(tris.data() + 9 * (size_t)ids[s]), &points[3 * (size_t)s], &uv[2 * (size_t)s]);
  }

  FILE* out = fopen(argv[2], "wb");
  if (!out) return 3;
  fwrite(face.data(), 4, face.size(), out);
  fwrite(position.data(), 4, position.size(), out);
  fwrite(normal.data(), 4, normal.size(), out);
  fwrite(bary.data(), 4, bary.size(), out);
  fwrite(uv.data(), 4, uv.size(), out);
  return fclose(out) == 0 ? 0 : 7;
}
