// light_guide_main.cpp -- csrc/ptmi_light_guide.h as a stand-alone program (built with -fsanitize=address,undefined by
// tests/test_light_guide_model.py; nothing is loaded into Python).
//   light_guide_main check                 the table's invariants and every rejection; exit 0 and "ok" on success
//   light_guide_main table BETA < scene    one object per line: shape material cx cy cz radius nx ny nz r g b; prints the table
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
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

static pt_scene_object object(int shape, int material, float radius, float r, float g, float b) {
  pt_scene_object o{};
  o.shape = shape; o.material = material;
  o.centre[0] = 1.f; o.centre[1] = 2.f; o.centre[2] = -3.f;
  o.radius = radius;
  if (shape == PT_SHAPE_DISC) o.normal[1] = 1.f;
  o.colour[0] = r; o.colour[1] = g; o.colour[2] = b;
  return o;
}

// The invariants every table must satisfy, whatever the scene.
static void invariants(const ptlight::Table& T, const std::vector<pt_scene_object>& scene, const char* what) {
  uint64_t sum = 0;
  uint32_t emitters = 0;
  for (size_t i = 0; i < scene.size(); ++i) emitters += scene[i].material == PT_MATERIAL_EMISSIVE;
  CHECK(T.n == emitters, "%s: %u emitters listed, %u in the scene", what, T.n, emitters);
  CHECK(T.n_draw <= T.n, "%s: n_draw %u > n %u", what, T.n_draw, T.n);
  bool any = false;
  for (uint32_t k = 0; k < T.n; ++k) {
    CHECK(T.object_index[k] < scene.size() && scene[T.object_index[k]].material == PT_MATERIAL_EMISSIVE, "%s: rank %u is no emitter", what, k);
    if (k) CHECK(T.object_index[k] > T.object_index[k - 1], "%s: declaration order at rank %u", what, k);
    any = any || T.mass[k] > 0.0;
  }
  CHECK(T.active() == any, "%s: active %d but positive mass %d", what, (int)T.active(), (int)any);
  if (!T.active()) return;
  CHECK(T.mass[T.n_draw - 1] > 0.0, "%s: the last rank drawn has no mass", what);
  for (uint32_t k = 0; k < T.n; ++k) {
    sum += T.weight[k];
    if (k) CHECK(T.threshold[k] >= T.threshold[k - 1], "%s: thresholds fall at rank %u", what, k);
    if (T.mass[k] == 0.0) CHECK(T.weight[k] == 0 && T.probability[k] == 0.f, "%s: rank %u has no mass but p = %g", what, k, (double)T.probability[k]);
    CHECK(T.probability[k] == (float)((double)T.weight[k] / ptlight::kTwo32), "%s: p of rank %u is not its integer weight", what, k);
    // the weight is what selection really gives rank k: words below c_k and not below c_{k-1}; the last rank drawn takes the rest
    const uint64_t lo = k ? T.threshold[k - 1] : 0;
    const uint64_t hi = k + 1 == T.n_draw ? (1ull << 32) : (k + 1 < T.n_draw ? (uint64_t)T.threshold[k] : lo);
    if (k < T.n_draw) CHECK(T.weight[k] == hi - lo, "%s: weight of rank %u is %llu, selection gives %llu", what, k, (unsigned long long)T.weight[k], (unsigned long long)(hi - lo));
    else CHECK(T.weight[k] == 0, "%s: rank %u beyond the last drawn has weight", what, k);
  }
  CHECK(sum == (1ull << 32), "%s: the weights sum to %llu, not 2^32", what, (unsigned long long)sum);
  double total = 0.0;
  for (uint32_t k = 0; k < T.n; ++k) total += T.mass[k];
  for (uint32_t k = 0; k < T.n; ++k)
    CHECK(std::fabs((double)T.weight[k] / ptlight::kTwo32 - T.mass[k] / total) <= 2.0 / ptlight::kTwo32 + 1e-15 * T.n,
          "%s: p of rank %u is %g, its share of the mass %g", what, k, (double)T.weight[k] / ptlight::kTwo32, T.mass[k] / total);
}

static int check_all() {
  ptlight::Table T;
  std::vector<pt_scene_object> scene;
  // no scene, no emitter, all-black emitters: inert
  ptlight::build(0.5f, nullptr, 0, T);
  CHECK(!T.active() && T.n == 0, "empty scene");
  scene = {object(PT_SHAPE_SPHERE, PT_MATERIAL_DIFFUSE, 1.f, 1, 1, 1), object(PT_SHAPE_DISC, PT_MATERIAL_SPECULAR, 1.f, 1, 1, 1)};
  ptlight::build(0.5f, scene.data(), 2, T);
  invariants(T, scene, "no emitter");
  CHECK(!T.active() && T.n == 0, "no emitter");
  scene.push_back(object(PT_SHAPE_SPHERE, PT_MATERIAL_EMISSIVE, 1.f, 0, 0, 0));
  scene.push_back(object(PT_SHAPE_DISC, PT_MATERIAL_EMISSIVE, 2.f, 0, 0, 0));
  ptlight::build(0.5f, scene.data(), (uint32_t)scene.size(), T);
  invariants(T, scene, "black emitters");
  CHECK(!T.active() && T.n == 2, "black emitters are listed but leave the guide inert");
  // masses: sphere 4 r^2 Y, disc 2 r^2 Y
  scene = {object(PT_SHAPE_SPHERE, PT_MATERIAL_EMISSIVE, 0.5f, 1, 1, 1), object(PT_SHAPE_DISC, PT_MATERIAL_EMISSIVE, 0.5f, 2, 2, 2),
           object(PT_SHAPE_SPHERE, PT_MATERIAL_EMISSIVE, 3.f, 0, 0, 0), object(PT_SHAPE_SPHERE, PT_MATERIAL_DIFFUSE, 1.f, 1, 1, 1),
           object(PT_SHAPE_SPHERE, PT_MATERIAL_EMISSIVE, 0.25f, 0, 8, 0), object(PT_SHAPE_DISC, PT_MATERIAL_EMISSIVE, 1.f, 0, 0, 0)};
  ptlight::build(0.25f, scene.data(), (uint32_t)scene.size(), T);
  invariants(T, scene, "mixed");
  CHECK(T.n == 5 && T.n_draw == 4, "mixed: %u emitters, %u drawn", T.n, T.n_draw);
  CHECK(std::fabs(T.mass[0] - 1.0) < 1e-12 && std::fabs(T.mass[1] - 1.0) < 1e-12 && T.mass[2] == 0.0 &&
            std::fabs(T.mass[3] - 0.7152 * 8 * 4 * 0.0625) < 1e-12,
        "mixed: masses %g %g %g %g", T.mass[0], T.mass[1], T.mass[2], T.mass[3]);
  CHECK(T.probability[2] == 0.f && T.probability[4] == 0.f && T.threshold[2] == T.threshold[1], "mixed: zero-mass emitters get p = 0");
  CHECK(T.beta_thr == 1u << 30 && T.beta == 0.25, "beta 0.25 is 2^30 / 2^32");
  // 32 emitters (the capacity), random masses; and a zero-mass emitter first and last
  std::mt19937 rng(7);
  std::uniform_real_distribution<float> U(0.f, 4.f);
  for (int round = 0; round < 200; ++round) {
    scene.clear();
    const int n = round < 100 ? PT_MAX_SCENE_OBJECTS : 1 + (int)(rng() % PT_MAX_SCENE_OBJECTS);
    for (int i = 0; i < n; ++i) {
      const bool black = rng() % 5 == 0 || (round % 7 == 0 && (i == 0 || i == n - 1));
      const bool emits = round < 100 || rng() % 2 == 0;
      const float e = black ? 0.f : U(rng) * (rng() % 9 == 0 ? 1e-9f : 1.f);
      scene.push_back(object(rng() % 2 ? PT_SHAPE_DISC : PT_SHAPE_SPHERE, emits ? PT_MATERIAL_EMISSIVE : PT_MATERIAL_DIFFUSE, 0.05f + U(rng), e, U(rng) * (black ? 0.f : 1.f), e));
    }
    ptlight::build(U(rng) * 0.2f, scene.data(), (uint32_t)scene.size(), T);
    invariants(T, scene, "random");
    if (round < 100) CHECK(T.n == PT_MAX_SCENE_OBJECTS, "32 emitters");
  }
  // one emitter: it is always selected
  scene = {object(PT_SHAPE_DISC, PT_MATERIAL_EMISSIVE, 0.3f, 100, 100, 100)};
  ptlight::build(0.9f, scene.data(), 1, T);
  invariants(T, scene, "single");
  CHECK(T.n_draw == 1 && T.weight[0] == (1ull << 32) && T.probability[0] == 1.f, "single emitter");
  // rejections, each naming its field, in the order struct_size, beta, alpha + beta
  pt_light_guide g{(uint32_t)sizeof(pt_light_guide), 0.5f};
  CHECK(ptlight::check(&g).empty() && ptlight::check(&g, 0.4).empty(), "a valid guide is accepted: %s", ptlight::check(&g, 0.4).c_str());
  CHECK(ptlight::check(nullptr).find("null") != std::string::npos, "null guide");
  pt_light_guide bad = g;
  bad.struct_size = 12; bad.beta = 7.f;
  CHECK(ptlight::check(&bad).find("struct_size") != std::string::npos, "struct_size comes first: %s", ptlight::check(&bad).c_str());
  for (float beta : {-0.1f, 0.95f, NAN, INFINITY, -INFINITY}) {
    bad = g; bad.beta = beta;
    const std::string why = ptlight::check(&bad, 0.9);
    CHECK(why.find("beta must be in") != std::string::npos, "beta %g: %s", (double)beta, why.c_str());
  }
  bad = g; bad.beta = 0.5f;
  CHECK(ptlight::check(&bad, 0.5).find("alpha + beta") != std::string::npos, "alpha + beta: %s", ptlight::check(&bad, 0.5).c_str());
  bad.beta = 0.3f;
  CHECK(ptlight::check(&bad, (double)0.6f).empty(), "0.6f + 0.3f is 0.9 but for rounding");
  CHECK(ptlight::check_alpha(0.5, 0.5).find("alpha + beta") != std::string::npos && ptlight::check_alpha(0.5, 0.4).empty(), "the sum from the env guide's side");
  bad.beta = 0.f;
  CHECK(ptlight::check(&bad, 0.9).empty(), "beta 0 beside alpha 0.9");
  if (g_failures) { fprintf(stderr, "%d failures\n", g_failures); return 1; }
  printf("ok\n");
  return 0;
}

static int print_table(float beta) {
  std::vector<pt_scene_object> scene;
  pt_scene_object o{};
  while (scene.size() < PT_MAX_SCENE_OBJECTS &&
         scanf("%d %d %f %f %f %f %f %f %f %f %f %f", &o.shape, &o.material, &o.centre[0], &o.centre[1], &o.centre[2], &o.radius, &o.normal[0],
               &o.normal[1], &o.normal[2], &o.colour[0], &o.colour[1], &o.colour[2]) == 12)
    scene.push_back(o);
  ptlight::Table T;
  ptlight::build(beta, scene.data(), (uint32_t)scene.size(), T);
  printf("%u %u %u %d\n", T.n, T.n_draw, T.beta_thr, (int)T.active());
  for (uint32_t k = 0; k < T.n; ++k)
    printf("%u %u %llu %.9g %.17g\n", T.object_index[k], T.threshold[k], (unsigned long long)T.weight[k], (double)T.probability[k], T.mass[k]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "check")) return check_all();
  if (argc >= 3 && !strcmp(argv[1], "table")) return print_table((float)atof(argv[2]));
  fprintf(stderr, "usage: light_guide_main check | table BETA < scene\n");
  return 2;
}
