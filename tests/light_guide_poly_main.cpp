// light_guide_poly_main.cpp -- csrc/ptmi_light_guide.h with polygon lamps as a stand-alone program (built with
// -fsanitize=address,undefined by tests/test_light_guide_poly_abi.py; nothing is loaded into Python).
//   light_guide_poly_main check                     every rejection of pt_set_light_guide_ex's check, in its order; "ok" on success
//   light_guide_poly_main table BETA MODE < scene   MODE vertices | plain (the four-argument build).  One object per line:
//                                                   shape material cx cy cz radius nx ny nz r g b and nine vertex coordinates;
//                                                   the table is stored as pt_set_scene_ex stores it, then built and printed
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ptmi_light_guide.h"

static int g_failures = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                          \
      fprintf(stderr, "\n");                                 \
      ++g_failures;                                          \
    }                                                        \
  } while (0)

static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static int check_all() {
  const pt_light_guide_ex good{(uint32_t)sizeof(pt_light_guide_ex), 0.5f, PT_LIGHT_GUIDE_POLYGONS};
  CHECK(sizeof(pt_light_guide_ex) == 12, "pt_light_guide_ex is 12 bytes");
  CHECK(ptlight::check_ex(&good).empty() && ptlight::check_ex(&good, 0.4).empty(), "a valid guide: %s", ptlight::check_ex(&good, 0.4).c_str());
  CHECK(has(ptlight::check_ex(nullptr), "null"), "null guide");
  // each guide carries the fault under test and every LATER one
  pt_light_guide_ex bad = good;
  bad.flags = 6; bad.beta = 0.6f;
  CHECK(has(ptlight::check_ex(&bad, 0.5), "flags must be 0 or PT_LIGHT_GUIDE_POLYGONS"), "flags before the sum: %s", ptlight::check_ex(&bad, 0.5).c_str());
  bad.beta = NAN;
  CHECK(has(ptlight::check_ex(&bad, 0.5), "beta must be in"), "beta before flags: %s", ptlight::check_ex(&bad, 0.5).c_str());
  bad.struct_size = 8;
  CHECK(has(ptlight::check_ex(&bad, 0.5), "struct_size must be 12 (got 8)"), "struct_size first: %s", ptlight::check_ex(&bad, 0.5).c_str());
  for (float beta : {-0.1f, 0.95f, NAN, INFINITY, -INFINITY}) {
    bad = good; bad.beta = beta;
    CHECK(has(ptlight::check_ex(&bad), "beta must be in"), "beta %g", (double)beta);
  }
  for (uint32_t flags : {2u, 3u, 0x80000000u, 0xffffffffu}) {
    bad = good; bad.flags = flags;
    CHECK(has(ptlight::check_ex(&bad), "flags") && has(ptlight::check_ex(&bad), std::to_string(flags).c_str()), "flags %u", flags);
  }
  bad = good; bad.flags = 0;
  CHECK(ptlight::check_ex(&bad).empty(), "flags 0 is pt_set_light_guide");
  bad = good;
  CHECK(has(ptlight::check_ex(&bad, 0.5), "alpha + beta"), "the sum: %s", ptlight::check_ex(&bad, 0.5).c_str());
  bad.beta = 0.3f;
  CHECK(ptlight::check_ex(&bad, (double)0.6f).empty(), "0.6f + 0.3f is 0.9 but for rounding");
  // a polygon without vertices is skipped; with them it is listed; black and degenerate-free tables keep the invariants
  pt_scene_object_ex ex[3] = {};
  ex[0].shape = PT_SHAPE_TRIANGLE; ex[0].material = PT_MATERIAL_EMISSIVE;
  ex[0].vertex[1][0] = 2.f; ex[0].vertex[2][1] = 3.f;                       // S = 6, A = 3
  ex[0].colour[0] = ex[0].colour[1] = ex[0].colour[2] = 1.f;
  ex[1].shape = PT_SHAPE_PARALLELOGRAM; ex[1].material = PT_MATERIAL_EMISSIVE;
  ex[1].vertex[1][2] = 0.5f; ex[1].vertex[2][0] = 4.f;                      // S = 2
  ex[1].colour[1] = 1.f;
  ex[2].shape = PT_SHAPE_PARALLELOGRAM; ex[2].material = PT_MATERIAL_DIFFUSE;
  ex[2].vertex[1][0] = 1.f; ex[2].vertex[2][1] = 1.f;
  ptscene::normalise_ex(ex, 3);
  pt_scene_object head[3];
  float vertex[3][3][3];
  for (int i = 0; i < 3; ++i) { memcpy(&head[i], &ex[i], sizeof head[i]); memcpy(vertex[i], ex[i].vertex, sizeof vertex[i]); }
  ptlight::Table T;
  ptlight::build(0.5f, head, 3, T);
  CHECK(T.n == 0 && !T.active() && !T.polygons, "the four-argument call skips polygons");
  ptlight::build(0.5f, head, 3, T, vertex);
  const double pi = 3.14159265358979323846;
  CHECK(T.n == 2 && T.n_draw == 2 && T.polygons && T.object_index[0] == 0 && T.object_index[1] == 1, "polygons listed: n %u", T.n);
  CHECK(std::fabs(T.mass[0] - 2.0 * 3.0 / pi) < 1e-12 && std::fabs(T.mass[1] - 0.7152 * 2.0 * 2.0 / pi) < 1e-12, "masses %g %g", T.mass[0], T.mass[1]);
  CHECK(T.weight[0] + T.weight[1] == (1ull << 32), "weights sum to 2^32");
  CHECK(ptlight::poly_area_s(vertex[0]) == 6.f && ptlight::poly_area_s(vertex[1]) == 2.f, "S");
  if (g_failures) { fprintf(stderr, "%d failures\n", g_failures); return 1; }
  printf("ok\n");
  return 0;
}

static int print_table(float beta, bool with_vertices) {
  std::vector<pt_scene_object_ex> scene;
  pt_scene_object_ex o{};
  float* v = &o.vertex[0][0];
  while (scene.size() < PT_MAX_SCENE_OBJECTS &&
         scanf("%d %d %f %f %f %f %f %f %f %f %f %f %f %f %f %f %f %f %f %f %f", &o.shape, &o.material, &o.centre[0], &o.centre[1], &o.centre[2],
               &o.radius, &o.normal[0], &o.normal[1], &o.normal[2], &o.colour[0], &o.colour[1], &o.colour[2], v, v + 1, v + 2, v + 3, v + 4, v + 5,
               v + 6, v + 7, v + 8) == 21)
    scene.push_back(o);
  const std::string bad = ptscene::check_ex(scene.data(), (uint32_t)scene.size(), (uint32_t)sizeof(pt_scene_object_ex));
  if (!bad.empty()) { fprintf(stderr, "%s\n", bad.c_str()); return 1; }
  ptscene::normalise_ex(scene.data(), (uint32_t)scene.size());
  std::vector<pt_scene_object> head(scene.size());
  float vertex[PT_MAX_SCENE_OBJECTS][3][3] = {};
  for (size_t i = 0; i < scene.size(); ++i) { memcpy(&head[i], &scene[i], sizeof head[i]); memcpy(vertex[i], scene[i].vertex, sizeof vertex[i]); }
  ptlight::Table T;
  if (with_vertices) ptlight::build(beta, head.data(), (uint32_t)head.size(), T, vertex);
  else ptlight::build(beta, head.data(), (uint32_t)head.size(), T);
  printf("%u %u %u %d %d\n", T.n, T.n_draw, T.beta_thr, (int)T.active(), (int)T.polygons);
  for (uint32_t k = 0; k < T.n; ++k)
    printf("%u %u %llu %.9g %.17g\n", T.object_index[k], T.threshold[k], (unsigned long long)T.weight[k], (double)T.probability[k], T.mass[k]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "check")) return check_all();
  if (argc >= 4 && !strcmp(argv[1], "table")) return print_table((float)atof(argv[2]), !strcmp(argv[3], "vertices"));
  fprintf(stderr, "usage: light_guide_poly_main check | table BETA vertices|plain < scene\n");
  return 2;
}
