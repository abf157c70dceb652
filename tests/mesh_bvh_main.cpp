// mesh_bvh_main.cpp -- the mesh builder (ptmi_mesh.h) and the stackless walk (pt_mesh.h) on the CPU, a stand-alone program:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I include -I ipu_path_trace_amd/csrc tests/mesh_bvh_main.cpp
// No argument: for every fixture, the tree's invariants, then walk == brute force bit for bit in (t, triangle) over kRays rays of
// the families below, and prints MESH_BVH_OK with the counts.  Any difference is a failure: this run is the calibration of the
// boxes' pad (ptmi_mesh.h).
//   --only FIXTURE: that fixture and the exact part alone.
//   --dump FIXTURE FILE: the fixture's mesh, the same rays and the walk's results into FILE, for tests/test_gpu_scene_meshes.py,
//   which puts the same rays through pt_mesh_intersect (the rays travel as this program's seed, not as a committed file).
// Built with -DPT_MESH_MUTATE_CULL (< for <= in the node cull) or -DPT_MESH_MUTATE_NAN (a NaN in the slab test rejects the
// node) the comparison must FAIL: tests/test_mesh_bvh.py checks that it does.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "ptmi_mesh.h"

namespace {

constexpr uint32_t kRays = 1u << 16;   // per fixture; split over the families in make_rays
constexpr float kInf = 3.402823466e+38f;

struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  float uniform() { return (float)(next() >> 40) * 5.9604644775390625e-08f; }   // [0, 1)
  float range(float a, float b) { return a + (b - a) * uniform(); }
  uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct Mesh {
  std::vector<float> v;
  std::vector<uint32_t> idx;
  uint32_t triangles() const { return (uint32_t)(idx.size() / 3); }
  pt_mesh view() const { return pt_mesh{sizeof(pt_mesh), (uint32_t)(v.size() / 3), triangles(), v.data(), idx.data()}; }
};

// ---- fixtures (world space, in front of the built-in camera)

const double kCentre[3] = {0.37, -0.21, -2.9};

Mesh icosphere(int k, double radius) {
  const double g = (1.0 + std::sqrt(5.0)) / 2.0;
  std::vector<double> p = {-1, g, 0, 1, g, 0, -1, -g, 0, 1, -g, 0, 0, -1, g, 0, 1, g, 0, -1, -g, 0, 1, -g, g, 0, -1, g, 0, 1, -g, 0, -1, -g, 0, 1};
  std::vector<uint32_t> f = {0, 11, 5, 0, 5, 1, 0, 1, 7, 0, 7, 10, 0, 10, 11, 1, 5, 9, 5, 11, 4, 11, 10, 2, 10, 7, 6, 7, 1, 8,
                             3, 9, 4, 3, 4, 2, 3, 2, 6, 3, 6, 8, 3, 8, 9, 4, 9, 5, 2, 4, 11, 6, 2, 10, 8, 6, 7, 9, 8, 1};
  for (int level = 0; level < k; ++level) {
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> mid;
    auto midpoint = [&](uint32_t a, uint32_t b) {
      const auto key = std::make_pair(std::min(a, b), std::max(a, b));
      auto it = mid.find(key);
      if (it != mid.end()) return it->second;
      const uint32_t m = (uint32_t)(p.size() / 3);
      for (int c = 0; c < 3; ++c) p.push_back(0.5 * (p[3 * a + c] + p[3 * b + c]));
      mid[key] = m;
      return m;
    };
    std::vector<uint32_t> nf;
    for (size_t t = 0; t < f.size(); t += 3) {
      const uint32_t a = f[t], b = f[t + 1], c = f[t + 2], ab = midpoint(a, b), bc = midpoint(b, c), ca = midpoint(c, a);
      const uint32_t four[12] = {a, ab, ca, b, bc, ab, c, ca, bc, ab, bc, ca};
      nf.insert(nf.end(), four, four + 12);
    }
    f.swap(nf);
  }
  Mesh M;
  for (size_t i = 0; i < p.size(); i += 3) {
    const double len = std::sqrt(p[i] * p[i] + p[i + 1] * p[i + 1] + p[i + 2] * p[i + 2]);
    for (int c = 0; c < 3; ++c) M.v.push_back((float)(kCentre[c] + radius * p[i + c] / len));
  }
  M.idx = f;
  return M;
}

// 32 x 32 cells of two triangles over x in [-0.5, 0.5], z in [-3.5, -2.5] (exact binary steps); the half x <= 0 is exactly flat.
// The cells are listed from the last to the first: the builder keeps lower coordinates to the left, so in ascending order the
// lowest index at a shared vertex would also be the first the walk meets, and the cull's <= would have nothing to do.
Mesh grid() {
  Mesh M;
  Rng rng{0x6772696473ull};
  const int n = 32;
  for (int j = 0; j <= n; ++j)
    for (int i = 0; i <= n; ++i) {
      const float x = (float)i / 32.0f - 0.5f, z = (float)j / 32.0f - 0.5f - 3.0f;
      const float y = i <= n / 2 ? -0.25f : -0.25f + 0.06f * rng.uniform();
      M.v.insert(M.v.end(), {x, y, z});
    }
  for (int j = n - 1; j >= 0; --j)
    for (int i = n - 1; i >= 0; --i) {
      const uint32_t a = (uint32_t)(j * (n + 1) + i), b = a + 1, c = a + (uint32_t)(n + 1), d = c + 1;
      M.idx.insert(M.idx.end(), {b, d, c, a, b, c});
    }
  return M;
}

Mesh doubled() {   // every triangle listed twice: the lower index must win everywhere
  const Mesh S = icosphere(2, 0.1);
  Mesh M;
  M.v = S.v;
  for (size_t t = 0; t < S.idx.size(); t += 3)
    for (int copy = 0; copy < 2; ++copy) M.idx.insert(M.idx.end(), {S.idx[t], S.idx[t + 1], S.idx[t + 2]});
  return M;
}

Mesh sliver() {   // long thin triangles, 1 : 1000
  Mesh M;
  Rng rng{0x736c6976ull};
  for (uint32_t t = 0; t < 256; ++t) {
    float p[3], u[3], w[3];
    for (int c = 0; c < 3; ++c) { p[c] = rng.range(-0.3f, 0.3f) + (c == 2 ? -3.0f : 0.0f); u[c] = rng.range(-1.f, 1.f); w[c] = rng.range(-1.f, 1.f); }
    const float ul = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) + 1e-6f;
    const float cr[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    const float cl = std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]) + 1e-6f;
    for (int c = 0; c < 3; ++c) M.v.push_back(p[c]);
    for (int c = 0; c < 3; ++c) M.v.push_back(p[c] + 0.5f * u[c] / ul);
    for (int c = 0; c < 3; ++c) M.v.push_back(p[c] + 0.0005f * cr[c] / cl);
    M.idx.insert(M.idx.end(), {3 * t, 3 * t + 1, 3 * t + 2});
  }
  return M;
}

Mesh single() {
  Mesh M;
  M.v = {0.1f, -0.2f, -3.0f, 0.45f, -0.1f, -3.2f, 0.2f, 0.3f, -2.9f};
  M.idx = {0, 1, 2};
  return M;
}

const char* const kFixtures[] = {"icosphere2", "icosphere4", "grid", "doubled", "sliver", "single"};
Mesh fixture(const std::string& name) {
  if (name == "icosphere2") return icosphere(2, 0.1);
  if (name == "icosphere4") return icosphere(4, 0.1);
  if (name == "grid") return grid();
  if (name == "doubled") return doubled();
  if (name == "sliver") return sliver();
  if (name == "single") return single();
  fprintf(stderr, "unknown fixture %s\n", name.c_str());
  exit(2);
}
uint64_t fixture_seed(const std::string& name) {
  uint64_t s = 0x6d657368ull;
  for (char c : name) s = s * 131 + (unsigned char)c;
  return s;
}

// ---- the tree's invariants

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failures++ < 20) { fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

bool inside(const ptmesh::Node& c, const ptmesh::Node& p) {
  for (int k = 0; k < 3; ++k) if (c.lo[k] < p.lo[k] || c.hi[k] > p.hi[k]) return false;
  return true;
}

// Checks the subtree at `node`, whose depth-first successor must be `after`; returns the number of its nodes.
uint32_t check_subtree(const ptmesh::Built& B, const std::vector<float>& frames, uint32_t node, uint32_t after, std::vector<uint32_t>& seen,
                       const char* name) {
  const ptmesh::Node& N = B.nodes[node];
  CHECK(N.skip == after, "%s: node %u skip %u, depth-first successor %u", name, node, N.skip, after);
  if (N.leaf != 0u) {
    const uint32_t first = N.leaf >> ptmesh::kLeafCountBits, count = N.leaf & 7u;
    CHECK(count >= 1 && count <= ptmesh::kMaxLeaf, "%s: leaf %u holds %u triangles", name, node, count);
    for (uint32_t s = first; s < first + count; ++s) {
      CHECK(s < B.orig.size(), "%s: slot %u out of range", name, s);
      if (s >= B.orig.size()) continue;
      seen[B.orig[s]] += 1;
      const float* f = &frames[ptmesh::kFrameFloats * (size_t)B.orig[s]];
      CHECK(!memcmp(&B.tris[3 * (size_t)s], f, 48), "%s: slot %u does not hold triangle %u", name, s, B.orig[s]);
      const ptmesh::Box tb = ptmesh::tri_box(f);
      for (int k = 0; k < 3; ++k) CHECK(tb.lo[k] >= N.lo[k] && tb.hi[k] <= N.hi[k], "%s: triangle %u leaves its leaf's box", name, B.orig[s]);
    }
    return 1;
  }
  const uint32_t left = node + 1;
  CHECK(left < B.nodes.size(), "%s: inner node %u without a left child", name, node);
  const uint32_t right = B.nodes[left].skip;
  CHECK(right > left && right < after, "%s: inner node %u: right child %u outside (%u, %u)", name, node, right, left, after);
  if (!(right > left && right < after)) return 1;
  CHECK(inside(B.nodes[left], N) && inside(B.nodes[right], N), "%s: a child of node %u leaves its parent's box", name, node);
  return 1 + check_subtree(B, frames, left, right, seen, name) + check_subtree(B, frames, right, after, seen, name);
}

// ---- rays

struct Rays { std::vector<float> o, d; };

void push(Rays& R, const float* o, const float* d) { R.o.insert(R.o.end(), o, o + 3); R.d.insert(R.d.end(), d, d + 3); }

void normalise(float* d) {
  const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (len > 0.f) for (int k = 0; k < 3; ++k) d[k] /= len;
  else { d[0] = 0.f; d[1] = 0.f; d[2] = -1.f; }
}

// kRays rays against a built mesh: (a) half of them from random points near the mesh towards random points of its box; (b) a
// quarter axis-parallel -- one or two direction components exactly 0 -- with origins off and ON slab planes of the tree (the
// root's and inner nodes'); (c) a quarter aimed exactly at vertices, where neighbouring triangles tie, from nearby.  flat_far
// (the grid): half of (c) instead falls straight down on vertices of the exactly flat half from 4096 units above.  There every
// operation of the triangle test and of the slab test is exact, the pad is absorbed by the rounding of hi - o, and so tnear equals
// the t of the triangles that share the vertex: the lower index lies in a node that only <= in the cull still visits.  (Far rays
// at curved geometry are no part of the contract: the rounding of a, b and t then exceeds any pad set by the mesh's size.)
Rays make_rays(const Mesh& M, const ptmesh::Built& B, uint64_t seed, bool flat_far) {
  Rays R;
  Rng rng{seed};
  const ptmesh::Node root = B.nodes[0];
  float ext = 0.f, mid[3];
  for (int k = 0; k < 3; ++k) { ext = std::max(ext, root.hi[k] - root.lo[k]); mid[k] = 0.5f * (root.lo[k] + root.hi[k]); }
  auto near_point = [&](float* p) { for (int k = 0; k < 3; ++k) p[k] = mid[k] + ext * rng.range(-1.5f, 1.5f); };
  auto box_point = [&](float* p) { for (int k = 0; k < 3; ++k) p[k] = rng.range(root.lo[k], root.hi[k]); };
  auto plane = [&](int k) {   // a slab plane of the tree along axis k
    const ptmesh::Node& N = B.nodes[rng.below(4) == 0 ? 0u : rng.below((uint32_t)B.nodes.size())];
    return rng.below(2) ? N.lo[k] : N.hi[k];
  };
  auto vertex = [&](float* p) { const uint32_t i = M.idx[rng.below((uint32_t)M.idx.size())]; for (int k = 0; k < 3; ++k) p[k] = M.v[3 * (size_t)i + k]; };
  for (uint32_t i = 0; i < kRays / 2; ++i) {
    float o[3], t[3], d[3];
    near_point(o); box_point(t);
    for (int k = 0; k < 3; ++k) d[k] = t[k] - o[k];
    normalise(d);
    push(R, o, d);
  }
  for (uint32_t i = 0; i < kRays / 4; ++i) {
    float o[3], d[3] = {0.f, 0.f, 0.f};
    const int axis = (int)rng.below(3);
    if (rng.below(2)) {   // two zero components: along +-axis, from outside the box
      d[axis] = rng.below(2) ? 1.f : -1.f;
      box_point(o);
      o[axis] = mid[axis] - d[axis] * ext * rng.range(0.6f, 2.0f);
      for (int k = 0; k < 3; ++k) if (k != axis && rng.below(2)) o[k] = plane(k);
    } else {              // one zero component: in the plane perpendicular to the axis
      float t[3];
      near_point(o); box_point(t);
      o[axis] = rng.below(2) ? plane(axis) : rng.range(root.lo[axis], root.hi[axis]);
      for (int k = 0; k < 3; ++k) d[k] = k == axis ? 0.f : t[k] - o[k];
      normalise(d);
    }
    push(R, o, d);
  }
  for (uint32_t i = 0; i < kRays / 4; ++i) {
    float o[3], t[3], d[3] = {0.f, 0.f, 0.f};
    vertex(t);
    if (flat_far && rng.below(2)) {
      while (t[0] > 0.f) vertex(t);
      o[0] = t[0]; o[1] = t[1] + 4096.f; o[2] = t[2];
      d[1] = -1.f;
    } else {
      near_point(o);
      for (int k = 0; k < 3; ++k) d[k] = t[k] - o[k];
      normalise(d);
    }
    push(R, o, d);
  }
  return R;
}

struct Hits { std::vector<float> t; std::vector<int32_t> tri; };

Hits trace(const ptmesh::Built& B, const Rays& R, bool tree) {
  Hits H;
  const size_t n = R.o.size() / 3;
  for (size_t i = 0; i < n; ++i) {
    const float* o = &R.o[3 * i];
    const float* d = &R.d[3 * i];
    float inv[3], tbest = kInf;
    ptmesh::ray_inverse(d, inv);
    const int slot = tree ? ptmesh::walk(B.nodes.data(), (uint32_t)B.nodes.size(), B.tris.data(), B.orig.data(), o, d, inv, tbest)
                          : ptmesh::brute(B.tris.data(), B.orig.data(), (uint32_t)B.orig.size(), o, d, tbest);
    H.t.push_back(slot < 0 ? 0.f : tbest);
    H.tri.push_back(slot < 0 ? -1 : (int32_t)B.orig[(size_t)slot]);
  }
  return H;
}

void build_fixture(const Mesh& M, std::vector<float>& frames, ptmesh::Built& B, float pad_scale = ptmesh::kPadScale) {
  const pt_mesh view = M.view();
  frames.clear();
  ptmesh::world_frames(view, frames);
  ptmesh::build(frames.data(), view.n_triangles, B, pad_scale);
}

size_t differences(const char* name, const Hits& W, const Hits& Y) {
  size_t diff = 0;
  for (size_t i = 0; i < W.t.size(); ++i)
    if (memcmp(&W.t[i], &Y.t[i], 4) || W.tri[i] != Y.tri[i]) {
      if (diff++ < 5)
        fprintf(stderr, "%s: ray %zu: walk (%.9g, %d), brute force (%.9g, %d)\n", name, i, (double)W.t[i], W.tri[i], (double)Y.t[i], Y.tri[i]);
    }
  return diff;
}

// With a positive pad no ray in a node's slab plane can meet a triangle of that node, and tnear stays below every t inside the
// box: neither the NaN rule nor the <= of the cull can then show.  They show where boxes have NO margin, so this part builds the
// grid with pad 0 -- its flat half gives zero-thickness boxes whose x and z planes are the grid lines -- and drops rays straight
// down on the flat half's vertices.  Every operation of both tests is exact there (binary fractions throughout), so pad 0 is
// safe; the ray lies IN the x and z slab planes of the nodes around the vertex (0 x inf), and tnear equals the triangles' t.
void exact_part() {
  const Mesh M = grid();
  std::vector<float> frames;
  ptmesh::Built B;
  build_fixture(M, frames, B, 0.f);
  CHECK(B.pad == 0.f, "exact: pad %g", (double)B.pad);
  Rays R;
  for (int j = 0; j <= 32; ++j)
    for (int i = 0; i <= 16; ++i)
      for (float height : {1.f, 64.f, 4096.f}) {
        const float* v = &M.v[3 * (size_t)(j * 33 + i)];
        const float o[3] = {v[0], v[1] + height, v[2]}, d[3] = {0.f, -1.f, 0.f};
        push(R, o, d);
      }
  const Hits W = trace(B, R, true), Y = trace(B, R, false);
  const size_t diff = differences("exact", W, Y);
  size_t hits = 0;
  for (int32_t t : Y.tri) hits += t >= 0;
  CHECK(diff == 0, "exact: %zu of %zu rays differ between the walk and brute force", diff, W.t.size());
  CHECK(hits == Y.tri.size(), "exact: %zu hits of %zu rays", hits, Y.tri.size());
  printf("exact      grid with pad 0: %zu rays on the flat half's vertices, %zu hits, %zu differences\n", W.t.size(), hits, diff);
}

int dump(const std::string& name, const char* path) {
  const Mesh M = fixture(name);
  std::vector<float> frames;
  ptmesh::Built B;
  build_fixture(M, frames, B);
  const Rays R = make_rays(M, B, fixture_seed(name), name == "grid");
  const Hits H = trace(B, R, true);
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); return 2; }
  const uint32_t head[4] = {0x4d455348u, (uint32_t)(M.v.size() / 3), M.triangles(), (uint32_t)H.t.size()};
  bool ok = fwrite(head, 4, 4, f) == 4;
  ok = ok && fwrite(M.v.data(), 4, M.v.size(), f) == M.v.size() && fwrite(M.idx.data(), 4, M.idx.size(), f) == M.idx.size();
  ok = ok && fwrite(R.o.data(), 4, R.o.size(), f) == R.o.size() && fwrite(R.d.data(), 4, R.d.size(), f) == R.d.size();
  ok = ok && fwrite(H.t.data(), 4, H.t.size(), f) == H.t.size() && fwrite(H.tri.data(), 4, H.tri.size(), f) == H.tri.size();
  ok = fclose(f) == 0 && ok;
  return ok ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "--dump")) return dump(argv[2], argv[3]);
  const char* only = argc == 3 && !strcmp(argv[1], "--only") ? argv[2] : nullptr;   // one fixture and the exact part (the mutation runs)
  if (argc != 1 && !only) { fprintf(stderr, "usage: %s [--dump FIXTURE FILE | --only FIXTURE]\n", argv[0]); return 2; }
  for (const char* name : kFixtures) {
    if (only && strcmp(only, name)) continue;
    const Mesh M = fixture(name);
    std::vector<float> frames;
    ptmesh::Built B, again;
    build_fixture(M, frames, B);
    build_fixture(M, frames, again);
    const uint32_t T = M.triangles();
    // invariants
    CHECK(B.nodes.size() == again.nodes.size() && !memcmp(B.nodes.data(), again.nodes.data(), B.nodes.size() * sizeof(ptmesh::Node)) &&
              B.orig == again.orig && !memcmp(B.tris.data(), again.tris.data(), B.tris.size() * sizeof(ptmesh::F4)),
          "%s: two builds differ", name);
    CHECK(B.nodes.size() <= 2 * (size_t)T - 1 && B.orig.size() == T && B.tris.size() == 3 * (size_t)T, "%s: sizes", name);
    CHECK(B.max_leaf <= ptmesh::kMaxLeaf, "%s: max_leaf %u", name, B.max_leaf);
    std::vector<uint32_t> seen(T, 0);
    const uint32_t counted = check_subtree(B, frames, 0, (uint32_t)B.nodes.size(), seen, name);
    CHECK(counted == B.nodes.size(), "%s: %u nodes reached of %zu", name, counted, B.nodes.size());
    for (uint32_t j = 0; j < T; ++j) CHECK(seen[j] == 1, "%s: triangle %u is in %u leaves", name, j, seen[j]);
    // walk == brute force, bit for bit
    const Rays R = make_rays(M, B, fixture_seed(name), !strcmp(name, "grid"));
    const Hits W = trace(B, R, true), Y = trace(B, R, false);
    const size_t diff = differences(name, W, Y);
    size_t hits = 0, odd = 0;
    for (size_t i = 0; i < W.t.size(); ++i) {
      hits += Y.tri[i] >= 0;
      odd += Y.tri[i] >= 0 && (Y.tri[i] & 1);
    }
    CHECK(diff == 0, "%s: %zu of %zu rays differ between the walk and brute force", name, diff, W.t.size());
    CHECK(W.t.size() >= kRays && hits * 16 >= W.t.size(), "%s: %zu rays, %zu hits: too few", name, W.t.size(), hits);
    if (!strcmp(name, "doubled")) CHECK(odd == 0, "doubled: %zu hits on the second copy of a triangle", odd);
    printf("%-10s %5u triangles %5zu nodes depth %2u max leaf %u pad %.3g: %zu rays, %zu hits, %zu differences\n", name, T, B.nodes.size(),
           B.depth, B.max_leaf, (double)B.pad, W.t.size(), hits, diff);
  }
  exact_part();
  if (g_failures) { printf("MESH_BVH_FAILED %d\n", g_failures); return 1; }
  printf("MESH_BVH_OK\n");
  return 0;
}
