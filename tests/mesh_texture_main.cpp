// mesh_texture_main.cpp -- texture coordinates and image textures of meshes (pt_set_mesh_texture) on the CPU, a stand-alone program:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I include -I ipu_path_trace_amd/csrc tests/mesh_texture_main.cpp
// The host validation (ptmi_mesh.h: check_texture), the host preparation (corner_uvs, slot_uvs, texel_vectors) and the lookup the
// kernels run (pt_mesh.h: tri_bary, blend_uv, tex_wrap, texel), which g++ compiles from the same header.
//   --validate        every message of check_texture in the contract's order, that valid input passes, the preparation, and the
//                     index rules at s' == 1 and t' == 0 for both wraps and both filters on a 5 x 3 image of distinct values and on a
//                     1 x 1 image; prints MESH_TEXTURE_VALIDATE_OK.
//   FIXTURE [--dump FILE]
//                     a fixture written by tests/mesh_texture_fixtures.py (two or three meshes, the first without a texture): builds
//                     the trees, draws 2^14 rays of the families of tests/mesh_bvh_main.cpp around the meshes, takes the nearest hit
//                     over the meshes in order and looks the texel up as mesh_texel_kernel does; checks the properties below on
//                     every hit and prints MESH_TEXTURE_OK or MESH_TEXTURE_FAILED.  --dump: rays and results (t, mesh, triangle,
//                     uv, bgr) for tests/test_gpu_mesh_texture.py, which puts the same rays through pt_mesh_texel.
// Properties per hit on a textured mesh.  NEAREST: the result is a texel of the image, bit for bit, and it is THE texel a float64
// restatement of rules 3 and 4 names (column from s, row from 1 - t, rows top to bottom) unless the position lies within 1e-4 of a
// texel boundary without being on it (counted as ties).  BILINEAR: every channel lies within the range of its four taps, the taps found here by integer
// modulo / clamp arithmetic, and within 4e-6 of the taps' range + 4e-7 of the largest tap of the float64 bilinear value.  A constant image returns
// the constant exactly under both filters.  An untextured mesh returns uv 0 and bgr 1.
#include <algorithm>
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
  std::vector<float> v, uvs, bgr;
  std::vector<uint32_t> idx, uvidx;
  uint32_t width = 0, height = 0;
  int32_t filter = 0, wrap = 0;
  std::vector<float> frames, corner, slot_uvs;   // world frames; corner uvs (empty: no texture); uvs in slot order
  std::vector<ptmesh::F4> texels;
  ptmesh::Built B;
  bool constant = false;
  uint32_t triangles() const { return (uint32_t)(idx.size() / 3); }
  bool textured() const { return !corner.empty(); }
  ptmesh::TexDesc desc() const {
    ptmesh::TexDesc D{};
    D.texels = texels.data(); D.width = width; D.height = height; D.filter = filter; D.wrap = wrap;
    return D;
  }
};

bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

bool load(const char* path, std::vector<Mesh>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); return false; }
  uint32_t head[2];
  bool ok = read_exact(f, head, 8) && head[0] == 0x5458544cu && head[1] >= 1 && head[1] <= 8;
  for (uint32_t m = 0; ok && m < head[1]; ++m) {
    uint32_t h[8];   // vertices, triangles, uvs, has uv indices, width, height, filter, wrap
    ok = read_exact(f, h, 32) && h[0] >= 1 && h[0] < (1u << 20) && h[1] >= 1 && h[1] < (1u << 20) && h[2] < (1u << 20) && h[3] <= 1 &&
         h[4] <= 64 && h[5] <= 64 && h[6] <= 1 && h[7] <= 1 && (h[2] == 0 || (h[4] >= 1 && h[5] >= 1));
    if (!ok) break;
    Mesh M;
    M.v.resize(3 * (size_t)h[0]); M.idx.resize(3 * (size_t)h[1]); M.uvs.resize(2 * (size_t)h[2]);
    if (h[3]) M.uvidx.resize(3 * (size_t)h[1]);
    if (h[2]) M.bgr.resize(3 * (size_t)h[4] * h[5]);
    M.width = h[4]; M.height = h[5]; M.filter = (int32_t)h[6]; M.wrap = (int32_t)h[7];
    ok = read_exact(f, M.v.data(), 4 * M.v.size()) && read_exact(f, M.idx.data(), 4 * M.idx.size()) &&
         read_exact(f, M.uvs.data(), 4 * M.uvs.size()) && read_exact(f, M.uvidx.data(), 4 * M.uvidx.size()) &&
         read_exact(f, M.bgr.data(), 4 * M.bgr.size());
    out.push_back(std::move(M));
  }
  fclose(f);
  if (!ok) fprintf(stderr, "%s: not a fixture file\n", path);
  return ok;
}

pt_mesh_texture view_of(const Mesh& M) {
  pt_mesh_texture t{};
  t.struct_size = sizeof(t); t.width = M.width; t.height = M.height; t.filter = M.filter; t.wrap = M.wrap;
  t.bgr = M.bgr.data(); t.uvs = M.uvs.data(); t.n_uvs = (uint32_t)(M.uvs.size() / 2);
  t.uv_indices = M.uvidx.empty() ? nullptr : M.uvidx.data();
  return t;
}

// What pt_set_scene_meshes and pt_set_mesh_texture do on the host, in the world frame.
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
    if (M.uvs.empty()) continue;
    const pt_mesh_texture t = view_of(M);
    const std::string badt = ptmesh::check_texture((uint32_t)k, view.n_vertices, view.n_triangles, M.idx.data(), &t);
    if (!badt.empty()) { fprintf(stderr, "%s\n", badt.c_str()); return false; }
    ptmesh::corner_uvs(view.n_triangles, M.idx.data(), t.uvs, t.uv_indices, M.corner);
    M.slot_uvs.resize(6 * (size_t)view.n_triangles);
    ptmesh::slot_uvs(M.corner.data(), M.B.orig.data(), view.n_triangles, M.slot_uvs.data());
    ptmesh::texel_vectors(&t, M.texels);
    M.constant = true;
    for (size_t i = 3; i < M.bgr.size(); ++i) M.constant = M.constant && M.bgr[i] == M.bgr[i % 3];
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

// Rules 3 and 4 again, in float64 and by integer arithmetic, from the binary32 (s, t): where the lookup must land.
double wrap64(double x, int wrap) {
  double w = wrap == ptmesh::kTexClamp ? std::min(std::max(x, 0.0), 1.0) : x - std::floor(x);
  return w >= 0.0 ? w : 0.0;
}
long index64(long i, long size, int wrap) {
  if (wrap == ptmesh::kTexClamp) return std::min(std::max(i, 0l), size - 1);
  return ((i % size) + size) % size;
}

// Within 1e-4 of an integer but not ON it: binary32 may fall on the other side.  A position that IS an integer in float64 -- a
// clamped coordinate above all: 0 or the size -- is one in binary32 too (the same exact product) and is judged.
bool near_boundary(double x) { return x != std::round(x) && std::fabs(x - std::round(x)) < 1e-4; }

struct Result { float t; int32_t mesh, tri; float uv[2], bgr[3]; };
struct Stats { size_t textured = 0, plain = 0, nearest = 0, bilinear = 0, ties = 0, constant = 0, outside = 0; };

// The nearest hit over the meshes in order (the scene's rule: a later object wins only with a strictly smaller t, which the walk's
// carried tbest gives), then what mesh_texel_kernel does.
Result lookup(const std::vector<Mesh>& meshes, const float* o, const float* d, Stats& S) {
  Result R{0.f, -1, -1, {0.f, 0.f}, {0.f, 0.f, 0.f}};
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
  R.t = tbest;
  R.tri = (int32_t)M.B.orig[(size_t)slot];
  R.bgr[0] = R.bgr[1] = R.bgr[2] = 1.f;
  if (!M.textured()) { S.plain += 1; return R; }
  S.textured += 1;
  float a, b;
  ptmesh::tri_bary(o, d, ptmesh::load_tri(M.B.tris.data() + 3 * (size_t)slot), a, b);
  ptmesh::blend_uv(a, b, M.slot_uvs.data() + 6 * (size_t)slot, R.uv[0], R.uv[1]);
  const ptmesh::TexDesc D = M.desc();
  ptmesh::texel(D, R.uv[0], R.uv[1], R.bgr);
  // the slot order holds the triangle's own corners
  CHECK(!memcmp(M.slot_uvs.data() + 6 * (size_t)slot, M.corner.data() + 6 * (size_t)R.tri, 24), "slot_uvs: slot %d is not triangle %d", slot, R.tri);
  if (R.uv[0] < 0.f || R.uv[0] > 1.f || R.uv[1] < 0.f || R.uv[1] > 1.f) S.outside += 1;
  const long W = (long)M.width, H = (long)M.height;
  const double sw = wrap64((double)R.uv[0], M.wrap), tw = wrap64((double)R.uv[1], M.wrap);
  if (M.constant) {
    S.constant += 1;
    CHECK(!memcmp(R.bgr, M.bgr.data(), 12), "a constant image returned (%.9g, %.9g, %.9g)", (double)R.bgr[0], (double)R.bgr[1], (double)R.bgr[2]);
  }
  if (M.filter == ptmesh::kTexNearest) {
    S.nearest += 1;
    bool found = false;
    for (size_t i = 0; i < M.texels.size() && !found; ++i) found = !memcmp(R.bgr, &M.texels[i], 12);
    CHECK(found, "nearest: (%.9g, %.9g, %.9g) is no texel of the image", (double)R.bgr[0], (double)R.bgr[1], (double)R.bgr[2]);
    const double X = sw * (double)W, Y = (1.0 - tw) * (double)H;
    const bool tie = near_boundary(X) || near_boundary(Y);
    if (tie) S.ties += 1;
    else {
      const long c = index64((long)std::floor(X), W, M.wrap), r = index64((long)std::floor(Y), H, M.wrap);
      CHECK(!memcmp(R.bgr, &M.texels[(size_t)(r * W + c)], 12), "nearest: uv (%.9g, %.9g) did not return texel (row %ld, column %ld)",
            (double)R.uv[0], (double)R.uv[1], r, c);
    }
  } else {
    S.bilinear += 1;
    const double X = sw * (double)W - 0.5, Y = (1.0 - tw) * (double)H - 0.5;
    const bool tie = near_boundary(X) || near_boundary(Y);
    if (tie) S.ties += 1;
    else {
      const long c0 = (long)std::floor(X), r0 = (long)std::floor(Y);
      const double fx = X - (double)c0, fy = Y - (double)r0;
      const ptmesh::F4 t00 = M.texels[(size_t)(index64(r0, H, M.wrap) * W + index64(c0, W, M.wrap))];
      const ptmesh::F4 t01 = M.texels[(size_t)(index64(r0, H, M.wrap) * W + index64(c0 + 1, W, M.wrap))];
      const ptmesh::F4 t10 = M.texels[(size_t)(index64(r0 + 1, H, M.wrap) * W + index64(c0, W, M.wrap))];
      const ptmesh::F4 t11 = M.texels[(size_t)(index64(r0 + 1, H, M.wrap) * W + index64(c0 + 1, W, M.wrap))];
      const float tap[3][4] = {{t00.x, t01.x, t10.x, t11.x}, {t00.y, t01.y, t10.y, t11.y}, {t00.z, t01.z, t10.z, t11.z}};
      for (int ch = 0; ch < 3; ++ch) {
        const float lo = *std::min_element(tap[ch], tap[ch] + 4), hi = *std::max_element(tap[ch], tap[ch] + 4);
        // one rounding of each of the three fmaf may leave the range by an ulp of the largest tap
        const float slack = hi * 2.4e-7f;
        CHECK(R.bgr[ch] >= lo - slack && R.bgr[ch] <= hi + slack, "bilinear: channel %d = %.9g outside its taps [%.9g, %.9g]", ch, (double)R.bgr[ch], (double)lo, (double)hi);
        const double top = tap[ch][0] + fx * ((double)tap[ch][1] - tap[ch][0]), bot = tap[ch][2] + fx * ((double)tap[ch][3] - tap[ch][2]);
        const double ref = top + fy * (bot - top);
        // binary32 against float64 from the same (s, t): s' and the product s' width round by 2^-24 each, relative to at most
        // width <= 8, so fx and fy are off by at most 1e-6 each -- 2e-6 of the taps' range --, and the three fmaf round by 2^-24 of
        // the largest tap each, 1.8e-7; twice that sum is allowed
        CHECK(std::fabs((double)R.bgr[ch] - ref) <= 4e-6 * ((double)hi - lo) + 4e-7 * (double)hi,
              "bilinear: channel %d = %.9g, float64 %.9g at uv (%.9g, %.9g)", ch, (double)R.bgr[ch], ref, (double)R.uv[0], (double)R.uv[1]);
      }
    }
  }
  return R;
}

// ---- the validation's messages, the preparation and the index rules

int validate() {
  const uint32_t idx[6] = {0, 1, 2, 2, 1, 3};
  const float uvs[8] = {0.f, 0.f, 1.f, 0.f, 0.f, 1.f, 1.5f, -2.f};
  float img[5 * 3 * 3];
  for (int i = 0; i < 45; ++i) img[i] = (float)(i + 1);
  auto expect = [&](const char* what, const std::string& got, const char* needle) {
    CHECK(got.find(needle) != std::string::npos, "%s: message \"%s\" lacks \"%s\"", what, got.c_str(), needle);
  };
  pt_mesh_texture good{};
  good.struct_size = sizeof(good); good.width = 5; good.height = 3; good.filter = PT_TEX_FILTER_BILINEAR; good.wrap = PT_TEX_WRAP_REPEAT;
  good.bgr = img; good.uvs = uvs; good.n_uvs = 4; good.uv_indices = nullptr;
  CHECK(ptmesh::check_texture(1, 4, 2, idx, &good).empty(), "a valid per-vertex texture refused");
  const uint32_t cidx[6] = {0, 0, 0, 1, 1, 1};
  pt_mesh_texture t = good;
  t.n_uvs = 2; t.uv_indices = cidx;
  CHECK(ptmesh::check_texture(1, 4, 2, idx, &t).empty(), "a valid per-corner texture refused");
  // every failure at once: the FIRST of the contract's order is the one reported, then it is mended and the next one shows
  float bad_img[45];
  memcpy(bad_img, img, sizeof img);
  bad_img[3 * (1 * 5 + 2) + 1] = -1.f;
  const uint32_t bad_cidx[6] = {0, 0, 0, 1, 7, 1};
  t = good;
  t.struct_size = 8; t.width = 0; t.filter = 2; t.wrap = -1; t.bgr = nullptr; t.uvs = nullptr; t.n_uvs = 3;
  expect("struct_size", ptmesh::check_texture(1, 4, 2, idx, &t), "mesh 1: texture: struct_size must be 56 (got 8)");
  t.struct_size = sizeof(t);
  expect("size", ptmesh::check_texture(1, 4, 2, idx, &t), "mesh 1: texture: width and height must be in 1..8192 (got 0 x 3)");
  t.width = 5; t.height = 8193;
  expect("size", ptmesh::check_texture(1, 4, 2, idx, &t), "width and height must be in 1..8192 (got 5 x 8193)");
  t.height = 3;
  expect("filter", ptmesh::check_texture(1, 4, 2, idx, &t), "mesh 1: texture: filter must be 0 (nearest) or 1 (bilinear) (got 2)");
  t.filter = 0;
  expect("wrap", ptmesh::check_texture(1, 4, 2, idx, &t), "mesh 1: texture: wrap must be 0 (repeat) or 1 (clamp) (got -1)");
  t.wrap = 1;
  expect("bgr", ptmesh::check_texture(1, 4, 2, idx, &t), "mesh 1: texture: null bgr");
  t.bgr = bad_img;
  expect("uvs", ptmesh::check_texture(1, 4, 2, idx, &t), "mesh 1: texture: null uvs with n_uvs = 3");
  t.uvs = uvs;
  expect("count", ptmesh::check_texture(1, 4, 2, idx, &t), "mesh 1: texture: n_uvs must equal n_vertices = 4 when uv_indices is null (got 3)");
  t.n_uvs = 2; t.uv_indices = bad_cidx;
  expect("texel", ptmesh::check_texture(1, 4, 2, idx, &t), "mesh 1: texture: texel (row 1, column 2) channel 1 must be finite and >= 0 (got -1)");
  bad_img[3 * (1 * 5 + 2) + 1] = NAN;
  expect("texel nan", ptmesh::check_texture(1, 4, 2, idx, &t), "texel (row 1, column 2) channel 1 must be finite and >= 0 (got nan)");
  bad_img[3 * (1 * 5 + 2) + 1] = INFINITY;
  expect("texel inf", ptmesh::check_texture(1, 4, 2, idx, &t), "texel (row 1, column 2) channel 1 must be finite and >= 0 (got inf)");
  t.bgr = img;
  expect("index", ptmesh::check_texture(1, 4, 2, idx, &t), "mesh 1: triangle 1: uv_indices[1] must be < n_uvs = 2 (got 7)");
  float nan_uv[8];
  memcpy(nan_uv, uvs, sizeof uvs);
  nan_uv[7] = NAN;
  t = good; t.uvs = nan_uv;
  expect("uv nan", ptmesh::check_texture(0, 4, 2, idx, &t), "mesh 0: triangle 1: uvs[3] must be finite (got nan)");
  nan_uv[7] = -INFINITY;
  expect("uv inf", ptmesh::check_texture(0, 4, 2, idx, &t), "mesh 0: triangle 1: uvs[3] must be finite (got -inf)");
  t.n_uvs = 3;
  expect("per-vertex index", ptmesh::check_texture(0, 3, 2, idx, &t), "mesh 0: triangle 1: indices[2] must be < n_uvs = 3 (got 3)");
  // an unreferenced uv is not examined
  float spare[10];
  memcpy(spare, uvs, sizeof uvs);
  spare[8] = NAN; spare[9] = 0.f;
  t = good; t.uvs = spare; t.n_uvs = 5; t.uv_indices = idx;
  CHECK(ptmesh::check_texture(0, 4, 2, idx, &t).empty(), "an unreferenced uv was examined");
  // preparation: corner order, slot order, one vector per texel
  std::vector<float> corner;
  ptmesh::corner_uvs(2, idx, uvs, nullptr, corner);
  CHECK(corner.size() == 12 && corner[2] == 1.f && corner[5] == 1.f && corner[10] == 1.5f && corner[11] == -2.f, "corner_uvs");
  const uint32_t orig[2] = {1, 0};
  float slots[12];
  ptmesh::slot_uvs(corner.data(), orig, 2, slots);
  CHECK(!memcmp(slots, corner.data() + 6, 24) && !memcmp(slots + 6, corner.data(), 24), "slot_uvs");
  std::vector<ptmesh::F4> tex;
  ptmesh::texel_vectors(&good, tex);
  CHECK(tex.size() == 15 && tex[7].x == img[21] && tex[7].y == img[22] && tex[7].z == img[23] && tex[7].w == 0.f, "texel_vectors");
  // interpolation at the corners: a = b = 0 is corner 0, a = 1 corner 1, b = 1 corner 2
  {
    const float uv6[6] = {0.25f, 0.5f, 2.f, -1.f, 8.f, 3.f};
    float s, tt;
    ptmesh::blend_uv(0.f, 0.f, uv6, s, tt); CHECK(s == 0.25f && tt == 0.5f, "blend_uv corner 0");
    ptmesh::blend_uv(1.f, 0.f, uv6, s, tt); CHECK(s == 2.f && tt == -1.f, "blend_uv corner 1");
    ptmesh::blend_uv(0.f, 1.f, uv6, s, tt); CHECK(s == 8.f && tt == 3.f, "blend_uv corner 2");
    ptmesh::blend_uv(0.25f, 0.5f, uv6, s, tt); CHECK(s == ((0.25f * 0.25f) + (0.25f * 2.f)) + (0.5f * 8.f), "blend_uv inside");
  }
  // the index rules on the 5 x 3 image: B of texel (r, c) is 3 (5 r + c) + 1
  auto B = [&](int r, int c) { return (float)(3 * (5 * r + c) + 1); };
  auto at = [&](int filter, int wrap, float s, float tt) {
    ptmesh::TexDesc D{};
    D.texels = tex.data(); D.width = 5; D.height = 3; D.filter = filter; D.wrap = wrap;
    float out[3];
    ptmesh::texel(D, s, tt, out);
    CHECK(out[1] == out[0] + 1.f && out[2] == out[0] + 2.f, "channels out of step: (%.9g, %.9g, %.9g)", (double)out[0], (double)out[1], (double)out[2]);
    return out[0];
  };
  const int N = ptmesh::kTexNearest, L = ptmesh::kTexBilinear, RP = ptmesh::kTexRepeat, CL = ptmesh::kTexClamp;
  // (0, 0) is the bottom-left corner: the LAST row, column 0; (just below 1, just below 1): the first row, the last column
  CHECK(at(N, CL, 0.01f, 0.01f) == B(2, 0), "nearest: (0, 0) is not the bottom-left texel");
  CHECK(at(N, CL, 0.99f, 0.99f) == B(0, 4), "nearest: (1, 1) is not the top-right texel");
  CHECK(at(N, RP, 0.3f, 0.5f) == B(1, 1), "nearest: (0.3, 0.5) is not texel (1, 1)");
  // s' == 1: CLAMP of any s >= 1; REPEAT of a tiny negative s, whose s - floorf(s) rounds to 1
  CHECK(ptmesh::tex_wrap(-1e-9f, RP) == 1.0f && ptmesh::tex_wrap(3.f, CL) == 1.0f, "s' == 1 is not reached");
  CHECK(at(N, CL, 3.f, 0.5f) == B(1, 4), "nearest, clamp, s' == 1: the column is not size - 1");
  CHECK(at(N, RP, -1e-9f, 0.5f) == B(1, 0), "nearest, repeat, s' == 1: the column does not wrap to 0");
  // t' == 0: the row coordinate is (1 - 0) height == height
  CHECK(at(N, CL, 0.5f, -2.f) == B(2, 2), "nearest, clamp, t' == 0: the row is not size - 1");
  CHECK(at(N, RP, 0.5f, 0.f) == B(0, 2), "nearest, repeat, t' == 0: the row does not wrap to 0");
  CHECK(at(N, RP, 0.5f, 4.f) == B(0, 2), "nearest, repeat, t == 4: the row does not wrap to 0");
  // t' == 1 (row coordinate 0) and s' == 0
  CHECK(at(N, CL, -5.f, 7.f) == B(0, 0), "nearest, clamp, s' == 0, t' == 1");
  // bilinear at the seam.  s' == 1: X = 4.5, columns 4 and 5 -> 0 (repeat) or 4 (clamp), fx = 0.5; t = 0.5: Y = 1, fy = 0, row 1
  CHECK(at(L, RP, -1e-9f, 0.5f) == 0.5f * (B(1, 4) + B(1, 0)), "bilinear, repeat, s' == 1");
  CHECK(at(L, CL, 3.f, 0.5f) == B(1, 4), "bilinear, clamp, s' == 1");
  // s' == 0: X = -0.5, columns -1 -> 4 (repeat) or 0 (clamp) and 0
  CHECK(at(L, RP, 0.f, 0.5f) == 0.5f * (B(1, 4) + B(1, 0)), "bilinear, repeat, s' == 0");
  CHECK(at(L, CL, 0.f, 0.5f) == B(1, 0), "bilinear, clamp, s' == 0");
  // t' == 0: Y = 2.5, rows 2 and 3 -> 0 (repeat) or 2 (clamp); s = 0.5: X = 2, fx = 0, column 2
  CHECK(at(L, RP, 0.5f, 0.f) == 0.5f * (B(2, 2) + B(0, 2)), "bilinear, repeat, t' == 0");
  CHECK(at(L, CL, 0.5f, -1.f) == B(2, 2), "bilinear, clamp, t' == 0");
  // a texel centre returns the texel: s = 0.5 is the centre of column 2, t = 0.5 of row 1
  CHECK(at(L, CL, 0.5f, 0.5f) == B(1, 2), "bilinear: a texel centre does not return its texel");
  // non-finite coordinates (an overflowed interpolation) read inside the image
  for (int f = 0; f < 2; ++f)
    for (int w = 0; w < 2; ++w)
      for (float x : {INFINITY, -INFINITY, NAN, 3e38f, -3e38f}) { (void)at(f, w, x, 0.5f); (void)at(f, w, 0.5f, x); }
  // a 1 x 1 image returns its texel whatever the coordinates
  {
    const ptmesh::F4 one{0.25f, 0.5f, 0.75f, 0.f};
    for (int f = 0; f < 2; ++f)
      for (int w = 0; w < 2; ++w) {
        ptmesh::TexDesc D{};
        D.texels = &one; D.width = 1; D.height = 1; D.filter = f; D.wrap = w;
        for (float s : {-3.7f, -1e-9f, 0.f, 0.25f, 0.5f, 0.75f, 1.f, 9.3f}) {
          float out[3];
          ptmesh::texel(D, s, 1.f - s, out);
          CHECK(out[0] == 0.25f && out[1] == 0.5f && out[2] == 0.75f, "1 x 1 image, filter %d wrap %d s %.9g", f, w, (double)s);
        }
      }
  }
  if (g_failures) { printf("MESH_TEXTURE_FAILED %d\n", g_failures); return 1; }
  printf("MESH_TEXTURE_VALIDATE_OK\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--validate")) return validate();
  if (argc < 2) { fprintf(stderr, "usage: %s --validate | FIXTURE [--dump FILE]\n", argv[0]); return 2; }
  const char* dump = nullptr;
  for (int i = 2; i < argc; ++i) {
    if (!strcmp(argv[i], "--dump") && i + 1 < argc) dump = argv[++i];
    else { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
  }
  std::vector<Mesh> meshes;
  if (!load(argv[1], meshes) || !prepare(meshes)) return 2;
  const Rays R = make_rays(meshes, 0x74657874757265ull + meshes.size());
  const size_t n = R.o.size() / 3;
  std::vector<Result> out(n);
  Stats S;
  size_t hits = 0;
  for (size_t i = 0; i < n; ++i) {
    out[i] = lookup(meshes, &R.o[3 * i], &R.d[3 * i], S);
    hits += out[i].mesh >= 0;
  }
  CHECK(hits * 8 >= n, "%zu hits of %zu rays: too few", hits, n);
  CHECK(S.textured >= 1000 && S.plain >= 1000, "%zu textured and %zu plain hits: too few", S.textured, S.plain);
  printf("rays %zu hits %zu textured %zu plain %zu nearest %zu bilinear %zu ties %zu constant %zu outside-unit-square %zu\n", n, hits,
         S.textured, S.plain, S.nearest, S.bilinear, S.ties, S.constant, S.outside);
  if (dump) {
    FILE* f = fopen(dump, "wb");
    if (!f) { perror(dump); return 2; }
    const uint32_t head[2] = {0x5458544fu, (uint32_t)n};
    std::vector<float> t(n), uv(2 * n), bgr(3 * n);
    std::vector<int32_t> mesh(n), tri(n);
    for (size_t i = 0; i < n; ++i) {
      t[i] = out[i].t; mesh[i] = out[i].mesh; tri[i] = out[i].tri; uv[2 * i] = out[i].uv[0]; uv[2 * i + 1] = out[i].uv[1];
      for (int k = 0; k < 3; ++k) bgr[3 * i + k] = out[i].bgr[k];
    }
    bool ok = fwrite(head, 4, 2, f) == 2 && fwrite(R.o.data(), 4, 3 * n, f) == 3 * n && fwrite(R.d.data(), 4, 3 * n, f) == 3 * n;
    ok = ok && fwrite(t.data(), 4, n, f) == n && fwrite(mesh.data(), 4, n, f) == n && fwrite(tri.data(), 4, n, f) == n;
    ok = ok && fwrite(uv.data(), 4, 2 * n, f) == 2 * n && fwrite(bgr.data(), 4, 3 * n, f) == 3 * n;
    ok = fclose(f) == 0 && ok;
    if (!ok) return 2;
  }
  if (g_failures) { printf("MESH_TEXTURE_FAILED %d\n", g_failures); return 1; }
  printf("MESH_TEXTURE_OK\n");
  return 0;
}
