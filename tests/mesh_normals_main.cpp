// mesh_normals_main.cpp -- vertex normals of meshes (pt_set_mesh_normals) on the CPU, a stand-alone program:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I include -I ipu_path_trace_amd/csrc tests/mesh_normals_main.cpp
// The host validation (ptmi_mesh.h: check_normals), the host preparation (corner_normals, slot_normals) and the shading-normal
// function the kernels run (pt_mesh.h: tri_bary, blend_normal, mirror_guard), which g++ compiles from the same header.
//   --validate                 every message of check_normals, and that valid input passes; prints MESH_NORMALS_VALIDATE_OK.
//   FIXTURE [options]          a fixture written by tests/mesh_normals_fixtures.py (two or three meshes, some with normals): builds
//                              the trees, draws 2^14 rays of the families of tests/mesh_bvh_main.cpp around the meshes, takes the nearest
//                              hit over the meshes in order and forms the shading normal; checks the properties below on every hit and
//                              prints MESH_NORMALS_OK or MESH_NORMALS_FAILED.
//     --dump FILE              rays and results (t, mesh, triangle, a, b, normal facing the ray) for tests/test_gpu_mesh_normals.py,
//                              which puts the same rays through pt_mesh_shade.
//     --sphere K CX CY CZ      mesh K carries the radial normals of a sphere about (CX, CY, CZ): measures, over its hits, the largest
//                              deviation of the shading normal from normalise(hp - centre) evaluated in float64, hp = o + t d with the
//                              binary32 t of the hit -- for the shading normal and for the flat normal (lines "closed-form ...").
//     --fallback K             mesh K is one triangle whose corner normals sum to zero: 256 more rays at its centroid must all
//                              return the geometric normal (rule 2's fallback).
// Properties per hit on a mesh with normals: unit length within 4 ulp; dot(n, d) <= 0 after the two-sided flip (rules 4 and 5);
// dot(v, ng_f) > 0 for the mirror direction after rule 6; the same normal, every component equal, when the corner normals are given
// negated (wound against the triangle), and, once it faces the ray, when the triangle's stored normal is the negated one (its
// winding reversed; a reversed triangle's own barycentrics round differently, so this is checked at the same a, b) -- apart
// from rays on which one of the rules' dot products is exactly 0, which are counted as ties.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ptmi_mesh.h"

namespace {

constexpr uint32_t kRays = 1u << 14;
constexpr float kInf = 3.402823466e+38f;

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failures++ < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  float uniform() { return (float)(next() >> 40) * 5.9604644775390625e-08f; }
  float range(float a, float b) { return a + (b - a) * uniform(); }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct Mesh {
  std::vector<float> v, normals;
  std::vector<uint32_t> idx, nidx;
  std::vector<float> frames, corner;          // world frames; corner normals (empty: flat)
  ptmesh::Built B;
  std::vector<ptmesh::F4> slot_normals;
  uint32_t triangles() const { return (uint32_t)(idx.size() / 3); }
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

bool load(const char* path, std::vector<Mesh>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  uint32_t head[2];
  bool ok = read_exact(f, head, 8) && head[0] == 0x4e524d4cu && head[1] >= 1 && head[1] <= 8;
  for (uint32_t m = 0; ok && m < head[1]; ++m) {
    uint32_t h[4];
    ok = read_exact(f, h, 16) && h[0] >= 1 && h[0] < (1u << 20) && h[1] >= 1 && h[1] < (1u << 20) && h[2] < (1u << 20) && h[3] <= 1;
    if (!ok) break;
    Mesh M;
    M.v.resize(3 * (size_t)h[0]); M.idx.resize(3 * (size_t)h[1]); M.normals.resize(3 * (size_t)h[2]);
    if (h[3]) M.nidx.resize(3 * (size_t)h[1]);
    ok = read_exact(f, M.v.data(), 4 * M.v.size()) && read_exact(f, M.idx.data(), 4 * M.idx.size()) &&
         read_exact(f, M.normals.data(), 4 * M.normals.size()) && read_exact(f, M.nidx.data(), 4 * M.nidx.size());
    out.push_back(std::move(M));
  }
  fclose(f);
  if (!ok) fprintf(stderr, "%s: not a fixture file\n", path);
  return ok;
}

// What pt_set_scene_meshes and pt_set_mesh_normals do on the host, in the world frame.
bool prepare(std::vector<Mesh>& meshes) {
  for (size_t k = 0; k < meshes.size(); ++k) {
    Mesh& M = meshes[k];
    const pt_mesh view{sizeof(pt_mesh), (uint32_t)(M.v.size() / 3), M.triangles(), M.v.data(), M.idx.data()};
    pt_scene_object_ex row{};
    row.shape = PT_SHAPE_MESH; row.material = 0; row.colour[0] = row.colour[1] = row.colour[2] = 0.5f;
    const std::string bad = ptmesh::check(&row, 1, sizeof(row), &view, 1);
    if (!bad.empty()) { fprintf(stderr, "mesh %zu: %s\n", k, bad.c_str()); return false; }
    ptmesh::world_frames(view, M.frames);
    ptmesh::build(M.frames.data(), view.n_triangles, M.B);
    if (M.normals.empty()) continue;
    const std::string badn = ptmesh::check_normals((uint32_t)k, view.n_vertices, view.n_triangles, M.idx.data(), M.normals.data(),
                                                   (uint32_t)(M.normals.size() / 3), M.nidx.empty() ? nullptr : M.nidx.data());
    if (!badn.empty()) { fprintf(stderr, "%s\n", badn.c_str()); return false; }
    ptmesh::corner_normals(view.n_triangles, M.idx.data(), M.normals.data(), M.nidx.empty() ? nullptr : M.nidx.data(), M.corner);
    M.slot_normals.resize(3 * (size_t)view.n_triangles);
    ptmesh::slot_normals(M.corner.data(), M.B.orig.data(), view.n_triangles, nullptr, M.slot_normals.data());
  }
  return true;
}

struct Rays { std::vector<float> o, d; };
void push(Rays& R, const float* o, const float* d) { R.o.insert(R.o.end(), o, o + 3); R.d.insert(R.d.end(), d, d + 3); }
void normalise(float* d) {
  const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (len > 0.f) for (int k = 0; k < 3; ++k) d[k] /= len;
  else { d[0] = 0.f; d[1] = 0.f; d[2] = -1.f; }
}

// The families of tests/mesh_bvh_main.cpp, per mesh in turn: half from points near the mesh towards points of its box, a quarter
// axis-parallel (one or two direction components exactly 0), a quarter aimed exactly at vertices.
Rays make_rays(const std::vector<Mesh>& meshes, uint64_t seed) {
  Rays R;
  Rng rng{seed};
  const uint32_t per = kRays / (uint32_t)meshes.size();
  for (size_t k = 0; k < meshes.size(); ++k) {
    const Mesh& M = meshes[k];
    const uint32_t n = k + 1 == meshes.size() ? kRays - per * (uint32_t)k : per;
    const ptmesh::Node root = M.B.nodes[0];
    float ext = 0.f, mid[3];
    for (int c = 0; c < 3; ++c) { ext = std::max(ext, root.hi[c] - root.lo[c]); mid[c] = 0.5f * (root.lo[c] + root.hi[c]); }
    auto near_point = [&](float* p) { for (int c = 0; c < 3; ++c) p[c] = mid[c] + ext * rng.range(-1.5f, 1.5f); };
    auto box_point = [&](float* p) { for (int c = 0; c < 3; ++c) p[c] = rng.range(root.lo[c], root.hi[c]); };
    for (uint32_t i = 0; i < n; ++i) {
      float o[3], t[3], d[3] = {0.f, 0.f, 0.f};
      const uint32_t family = i < n / 2 ? 0u : (i < n / 2 + n / 4 ? 1u : 2u);
      if (family == 0) {
        near_point(o); box_point(t);
        for (int c = 0; c < 3; ++c) d[c] = t[c] - o[c];
        normalise(d);
      } else if (family == 1) {
        const int axis = (int)rng.below(3);
        if (rng.below(2)) {
          d[axis] = rng.below(2) ? 1.f : -1.f;
          box_point(o);
          o[axis] = mid[axis] - d[axis] * ext * rng.range(0.6f, 2.0f);
        } else {
          near_point(o); box_point(t);
          o[axis] = rng.range(root.lo[axis], root.hi[axis]);
          for (int c = 0; c < 3; ++c) d[c] = c == axis ? 0.f : t[c] - o[c];
          normalise(d);
        }
      } else {
        const uint32_t vi = M.idx[rng.below((uint32_t)M.idx.size())];
        near_point(o);
        for (int c = 0; c < 3; ++c) d[c] = M.v[3 * (size_t)vi + c] - o[c];
        normalise(d);
      }
      push(R, o, d);
    }
  }
  return R;
}

// Equal component for component; the sign of a zero may differ (a ray through a vertex has a barycentric of exactly 0, and
// (+0) + (-0) is +0 whichever way the normals point).
bool same(const float* a, const float* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

struct Result { float t; int32_t mesh, tri; float a, b, n[3]; };

// The nearest hit over the meshes in order (the scene's rule: a later object wins only with a strictly smaller t, which the walk's
// carried tbest gives), then what mesh_shade_kernel does.  `stats` counts the rule's decisions over hits on meshes with normals.
struct Stats { size_t smooth = 0, flat = 0, fallback = 0, oriented = 0, dropped = 0, guarded = 0, ties = 0; };

Result shade(const std::vector<Mesh>& meshes, const float* o, const float* d, Stats& S) {
  Result R{0.f, -1, -1, 0.f, 0.f, {0.f, 0.f, 0.f}};
  float inv[3], tbest = kInf;
  ptmesh::ray_inverse(d, inv);
  int slot = -1;
  for (size_t k = 0; k < meshes.size(); ++k) {
    const ptmesh::Built& B = meshes[k].B;
    const int s = ptmesh::walk(B.nodes.data(), (uint32_t)B.nodes.size(), B.tris.data(), B.orig.data(), o, d, inv, tbest);
    if (s >= 0) { slot = s; R.mesh = (int32_t)k; }
  }
  if (R.mesh < 0) return R;
  const Mesh& M = meshes[(size_t)R.mesh];
  const ptmesh::F4* tri = M.B.tris.data() + 3 * (size_t)slot;
  const ptmesh::Tri T = ptmesh::load_tri(tri);
  const float ng[3] = {tri[2].y, tri[2].z, tri[2].w};
  R.t = tbest;
  R.tri = (int32_t)M.B.orig[(size_t)slot];
  float ns[3];
  if (M.corner.empty()) {
    ptmesh::tri_bary(o, d, T, R.a, R.b);
    for (int k = 0; k < 3; ++k) ns[k] = ng[k];
    S.flat += 1;
  } else {
    const ptmesh::F4* vn = M.slot_normals.data() + 3 * (size_t)slot;
    ptmesh::shading_normal(o, d, T, ng, vn, R.a, R.b, ns);
    S.smooth += 1;
    // the two halves one after the other, as shade_hit calls them: the same bits
    float a2, b2, ns2[3];
    ptmesh::tri_bary(o, d, T, a2, b2);
    ptmesh::blend_normal(a2, b2, d, ng, vn, ns2);
    CHECK(!memcmp(ns, ns2, 12) && !memcmp(&a2, &R.a, 4) && !memcmp(&b2, &R.b, 4), "shading_normal != tri_bary + blend_normal");
    // which rules decided (float64 is not needed: the function's own expressions)
    const float c = (1.0f - R.a) - R.b;
    const float m[3] = {((c * vn[0].x) + (R.a * vn[1].x)) + (R.b * vn[2].x), ((c * vn[0].y) + (R.a * vn[1].y)) + (R.b * vn[2].y),
                        ((c * vn[0].z) + (R.a * vn[1].z)) + (R.b * vn[2].z)};
    const float l2 = m[0] * m[0] + m[1] * m[1] + m[2] * m[2];
    const bool fallback = !(l2 > ptmesh::kSmoothMinLen2);
    S.fallback += fallback;
    if (fallback) CHECK(!memcmp(ns, ng, 12), "fallback: the shading normal is not the geometric normal");
    const bool same_as_ng = !memcmp(ns, ng, 12);
    if (!fallback && same_as_ng) S.dropped += 1;
    // unit length within 4 ulp
    const double len = std::sqrt((double)ns[0] * ns[0] + (double)ns[1] * ns[1] + (double)ns[2] * ns[2]);
    CHECK(std::fabs(len - 1.0) <= 4.0 * 1.1920928955078125e-07, "|n| = %.9g", len);
    // normals given negated; the stored normal negated (reversed winding): the same normal once it faces the ray
    ptmesh::F4 neg[3];
    for (int k = 0; k < 3; ++k) neg[k] = ptmesh::F4{-vn[k].x, -vn[k].y, -vn[k].z, 0.f};
    const float nng[3] = {-ng[0], -ng[1], -ng[2]};
    float n_neg[3], n_rev[3];
    ptmesh::blend_normal(R.a, R.b, d, ng, neg, n_neg);
    ptmesh::blend_normal(R.a, R.b, d, nng, vn, n_rev);
    const float inv_len = 1.0f / sqrtf(fallback ? 1.0f : l2);
    const float unit[3] = {m[0] * inv_len, m[1] * inv_len, m[2] * inv_len};   // the interpolated normal before rules 3 and 4
    const bool tie = fallback || ptmesh::dot3(unit, ng) == 0.0f || ptmesh::dot3(unit, d) == 0.0f || ptmesh::dot3(ng, d) == 0.0f;
    if (tie) S.ties += 1;
    else {
      CHECK(same(n_neg, ns), "negated corner normals give another normal");
      float f_rev[3] = {n_rev[0], n_rev[1], n_rev[2]}, f_ns[3] = {ns[0], ns[1], ns[2]};
      if (ptmesh::dot3(f_rev, d) > 0.0f) for (int k = 0; k < 3; ++k) f_rev[k] = -f_rev[k];
      if (ptmesh::dot3(f_ns, d) > 0.0f) for (int k = 0; k < 3; ++k) f_ns[k] = -f_ns[k];
      CHECK(same(f_rev, f_ns), "a reversed stored normal gives another normal");
    }
  }
  // the two-sided flip (rule 5: diffuse and specular), then the mirror direction with rule 6
  if (ptmesh::dot3(ns, d) > 0.0f) for (int k = 0; k < 3; ++k) ns[k] = -ns[k];
  CHECK(ptmesh::dot3(ns, d) <= 0.0f, "dot(n, d) = %.9g > 0", (double)ptmesh::dot3(ns, d));
  if (!M.corner.empty()) {
    const float cost = ptmesh::dot3(d, ns);
    float v[3] = {d[0] - ns[0] * (cost * 2.0f), d[1] - ns[1] * (cost * 2.0f), d[2] - ns[2] * (cost * 2.0f)};
    const float before[3] = {v[0], v[1], v[2]};
    ptmesh::mirror_guard(d, ng, v);
    S.guarded += memcmp(before, v, 12) != 0;
    float ngf[3] = {ng[0], ng[1], ng[2]};
    if (ptmesh::dot3(ngf, d) > 0.0f) for (int k = 0; k < 3; ++k) ngf[k] = -ngf[k];
    if (ptmesh::dot3(ngf, d) != 0.0f) CHECK(ptmesh::dot3(v, ngf) > 0.0f, "mirror direction below the surface: dot(v, ng_f) = %.9g", (double)ptmesh::dot3(v, ngf));
  }
  for (int k = 0; k < 3; ++k) R.n[k] = ns[k];
  return R;
}

// ---- the validation's messages

int validate() {
  const uint32_t idx[6] = {0, 1, 2, 2, 1, 3};
  const float good[12] = {0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 2, 0};
  auto expect = [&](const char* what, const std::string& got, const char* needle) {
    CHECK(got.find(needle) != std::string::npos, "%s: message \"%s\" lacks \"%s\"", what, got.c_str(), needle);
  };
  CHECK(ptmesh::check_normals(1, 4, 2, idx, good, 4, nullptr).empty(), "valid per-vertex normals refused");
  const uint32_t nidx[6] = {0, 0, 0, 1, 1, 1};
  CHECK(ptmesh::check_normals(1, 4, 2, idx, good, 2, nidx).empty(), "valid per-corner normals refused");
  expect("null", ptmesh::check_normals(1, 4, 2, idx, nullptr, 4, nullptr), "mesh 1: null normals with n_normals = 4");
  expect("count", ptmesh::check_normals(1, 4, 2, idx, good, 3, nullptr), "mesh 1: n_normals must equal n_vertices = 4 when normal_indices is null (got 3)");
  const uint32_t bad_idx[6] = {0, 0, 0, 1, 2, 1};
  expect("index", ptmesh::check_normals(1, 4, 2, idx, good, 2, bad_idx), "mesh 1: triangle 1: normal_indices[1] must be < n_normals = 2 (got 2)");
  float nan_n[12];
  memcpy(nan_n, good, sizeof good);
  nan_n[10] = NAN;
  expect("nan", ptmesh::check_normals(0, 4, 2, idx, nan_n, 4, nullptr), "mesh 0: triangle 1: normals[3] must be finite (got nan)");
  nan_n[10] = INFINITY;
  expect("inf", ptmesh::check_normals(0, 4, 2, idx, nan_n, 4, nullptr), "normals[3] must be finite (got inf)");
  float zero_n[12];
  memcpy(zero_n, good, sizeof good);
  zero_n[2] = 0.f;
  expect("zero", ptmesh::check_normals(0, 4, 2, idx, zero_n, 4, nullptr), "mesh 0: triangle 0: normals[0] must have a finite dot(n, n) > 0 (got 0)");
  zero_n[2] = 3e38f;
  expect("overflow", ptmesh::check_normals(0, 4, 2, idx, zero_n, 4, nullptr), "normals[0] must have a finite dot(n, n) > 0 (got inf)");
  zero_n[2] = 1e-30f;   // the square underflows to 0
  expect("underflow", ptmesh::check_normals(0, 4, 2, idx, zero_n, 4, nullptr), "normals[0] must have a finite dot(n, n) > 0 (got 0)");
  // an unreferenced normal is not examined
  float spare[15];
  memcpy(spare, good, sizeof good);
  spare[12] = NAN; spare[13] = 0.f; spare[14] = 0.f;
  CHECK(ptmesh::check_normals(0, 4, 2, idx, spare, 5, idx).empty(), "an unreferenced normal was examined");
  // preparation: unit length by a disc normal's expressions; slot order follows orig
  std::vector<float> corner;
  ptmesh::corner_normals(2, idx, good, nullptr, corner);
  CHECK(corner.size() == 18 && corner[3 * 5 + 1] == 1.0f && corner[2] == 1.0f, "corner_normals");
  const uint32_t orig[2] = {1, 0};
  ptmesh::F4 slots[6];
  ptmesh::slot_normals(corner.data(), orig, 2, nullptr, slots);
  CHECK(slots[0].x == corner[9] && slots[0].y == corner[10] && slots[3].z == corner[2] && slots[5].w == 0.f, "slot_normals");
  if (g_failures) { printf("MESH_NORMALS_FAILED %d\n", g_failures); return 1; }
  printf("MESH_NORMALS_VALIDATE_OK\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--validate")) return validate();
  if (argc < 2) { fprintf(stderr, "usage: %s --validate | FIXTURE [--dump FILE] [--sphere K CX CY CZ] [--fallback K]\n", argv[0]); return 2; }
  const char* dump = nullptr;
  int sphere = -1, fallback = -1;
  double centre[3] = {0, 0, 0};
  for (int i = 2; i < argc; ++i) {
    if (!strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
    else if (!strcmp(argv[i], "--sphere") && i + 4 < argc) { sphere = atoi(argv[i + 1]); for (int k = 0; k < 3; ++k) centre[k] = atof(argv[i + 2 + k]); i += 4; }
    else if (!strcmp(argv[i], "--fallback") && i + 1 < argc) fallback = atoi(argv[++i]);
    else { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
  }
  std::vector<Mesh> meshes;
  if (!load(argv[1], meshes) || !prepare(meshes)) return 2;
  if (sphere >= (int)meshes.size() || fallback >= (int)meshes.size()) { fprintf(stderr, "no such mesh\n"); return 2; }
  Rays R = make_rays(meshes, 0x6e6f726d616c73ull + meshes.size());
  if (fallback >= 0) {   // rays at the centroid of the zero-sum triangle, from both sides
    const Mesh& M = meshes[(size_t)fallback];
    const float* f = M.frames.data();
    float c[3];
    for (int k = 0; k < 3; ++k) c[k] = f[k] + (f[3 + k] + f[6 + k]) * (1.0f / 3.0f);
    Rng rng{0x66616c6cull};
    for (int i = 0; i < 256; ++i) {
      float o[3], d[3];
      do {   // from nearby and not grazing: the barycentrics must land within 1e-6 of (1/3, 1/3) for |m|^2 <= 1e-12
        for (int k = 0; k < 3; ++k) o[k] = c[k] + rng.range(-0.1f, 0.1f);
        for (int k = 0; k < 3; ++k) d[k] = c[k] - o[k];
        normalise(d);
      } while (std::fabs(ptmesh::dot3(d, f + 9)) < 0.5f);
      push(R, o, d);
    }
  }
  const size_t n = R.o.size() / 3;
  std::vector<Result> out(n);
  Stats S;
  size_t hits = 0, fallback_hits = 0, sphere_hits = 0, sphere_skipped = 0;
  double dev_smooth = 0.0, dev_flat = 0.0;
  for (size_t i = 0; i < n; ++i) {
    const float* o = &R.o[3 * i];
    const float* d = &R.d[3 * i];
    const size_t fb_before = S.fallback;
    out[i] = shade(meshes, o, d, S);
    hits += out[i].mesh >= 0;
    if (i >= kRays && out[i].mesh == fallback) {
      fallback_hits += 1;
      CHECK(S.fallback == fb_before + 1, "ray %zu at the centroid of the zero-sum triangle did not fall back", i);
    }
    if (out[i].mesh == sphere && sphere >= 0) {
      // closed form: normalise(hp - centre), hp = o + t d with the hit's binary32 t, in float64, facing the ray
      double ref[3], len = 0.0, facing = 0.0;
      for (int k = 0; k < 3; ++k) { ref[k] = ((double)o[k] + (double)out[i].t * (double)d[k]) - centre[k]; len += ref[k] * ref[k]; }
      len = std::sqrt(len);
      for (int k = 0; k < 3; ++k) { ref[k] /= len; facing += ref[k] * (double)d[k]; }
      if (facing > 0.0) for (int k = 0; k < 3; ++k) ref[k] = -ref[k];
      // the geometric normal facing the ray, for the flat figure and to tell a hit rule 4 decided
      const Mesh& M = meshes[(size_t)sphere];
      const float* fr = &M.frames[ptmesh::kFrameFloats * (size_t)out[i].tri];
      double g[3] = {fr[9], fr[10], fr[11]}, gd = 0.0;
      for (int k = 0; k < 3; ++k) gd += g[k] * (double)d[k];
      if (gd > 0.0) for (int k = 0; k < 3; ++k) g[k] = -g[k];
      const bool is_ng = out[i].n[0] == (float)g[0] && out[i].n[1] == (float)g[1] && out[i].n[2] == (float)g[2];
      if (is_ng) { sphere_skipped += 1; continue; }   // rule 4 (or 2) gave the geometric normal: not the interpolated one
      sphere_hits += 1;
      for (int k = 0; k < 3; ++k) {
        dev_smooth = std::max(dev_smooth, std::fabs((double)out[i].n[k] - ref[k]));
        dev_flat = std::max(dev_flat, std::fabs(g[k] - ref[k]));
      }
    }
  }
  CHECK(hits * 8 >= n, "%zu hits of %zu rays: too few", hits, n);
  CHECK(S.smooth >= 1000 && S.flat >= 1000, "%zu smooth and %zu flat hits: too few", S.smooth, S.flat);
  if (fallback >= 0) CHECK(fallback_hits >= 200, "%zu of 256 centroid rays hit the zero-sum triangle", fallback_hits);
  printf("rays %zu hits %zu smooth %zu flat %zu fallback %zu dropped-by-rule-4 %zu mirror-guarded %zu ties %zu\n", n, hits, S.smooth, S.flat,
         S.fallback, S.dropped, S.guarded, S.ties);
  if (sphere >= 0) {
    CHECK(sphere_hits >= 1000, "%zu closed-form hits: too few", sphere_hits);
    printf("closed-form hits %zu skipped %zu smooth %.9e flat %.9e\n", sphere_hits, sphere_skipped, dev_smooth, dev_flat);
  }
  if (dump) {
    FILE* f = fopen(dump, "wb");
    if (!f) { perror(dump); return 2; }
    const uint32_t head[2] = {0x4e524d4fu, (uint32_t)n};
    std::vector<float> t(n), ab(2 * n), nn(3 * n);
    std::vector<int32_t> mesh(n), tri(n);
    for (size_t i = 0; i < n; ++i) {
      t[i] = out[i].t; mesh[i] = out[i].mesh; tri[i] = out[i].tri; ab[2 * i] = out[i].a; ab[2 * i + 1] = out[i].b;
      for (int k = 0; k < 3; ++k) nn[3 * i + k] = out[i].n[k];
    }
    bool ok = fwrite(head, 4, 2, f) == 2 && fwrite(R.o.data(), 4, 3 * n, f) == 3 * n && fwrite(R.d.data(), 4, 3 * n, f) == 3 * n;
    ok = ok && fwrite(t.data(), 4, n, f) == n && fwrite(mesh.data(), 4, n, f) == n && fwrite(tri.data(), 4, n, f) == n;
    ok = ok && fwrite(ab.data(), 4, 2 * n, f) == 2 * n && fwrite(nn.data(), 4, 3 * n, f) == 3 * n;
    ok = fclose(f) == 0 && ok;
    if (!ok) return 2;
  }
  if (g_failures) { printf("MESH_NORMALS_FAILED %d\n", g_failures); return 1; }
  printf("MESH_NORMALS_OK\n");
  return 0;
}
