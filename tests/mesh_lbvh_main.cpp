// mesh_lbvh_main.cpp -- the linear BVH builder and the refit (ipu_path_trace_amd/csrc/pt_mesh_build.h) on the CPU, a stand-alone
// program:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I include -I ipu_path_trace_amd/csrc tests/mesh_lbvh_main.cpp
// The fixtures, rays, invariants and comparisons are those of tests/mesh_bvh_main.cpp, by that program's own code (it is included
// below with its main renamed), plus small fixtures of this program's own.
// No argument: for every fixture
//   * the reference builder: the tree's invariants, its boxes against the triangles' boxes and the pad, two builds identical, the
//     parallel form (the kernels' functions run thread by thread) identical to it, walk == brute force bit for bit in (t, triangle)
//     over kRays rays in the world frame, and the walk over the SAH tree's own rays == the SAH walk;
//   * under three poses (moved, rolled, from behind): the SAH tree and the linear tree REFITTED from the world frame, and the
//     host's rebuild, each with the invariants and walk == brute force in the posed frame (the grid's far family belongs to the
//     world frame alone: far rays at inexact geometry are outside the contract); the refit's thread form identical to it; a refit
//     under the identity gives back the world tree's bytes.
// Any difference is a failure.  Prints MESH_LBVH_OK.
//   --only FIXTURE: that fixture alone.
//   --dump FIXTURE FILE: the fixture's mesh, its world-frame rays with the walk's results, the cameras of two poses, and the trees
//   tests/test_gpu_mesh_device_build.py holds the device against: the linear tree in the world frame and under each pose, and the
//   world-frame linear and SAH trees refitted to each pose.
// Built with -DPT_LBVH_MUTATE_NO_PAD (boxes fitted without the pad) or -DPT_LBVH_MUTATE_KEEP_PAD (a refit that keeps the old
// root's pad) the program must FAIL: tests/test_mesh_lbvh.py checks that it does.
#define main mesh_bvh_program_main
#include "mesh_bvh_main.cpp"
#undef main

#include "pt_mesh_build.h"

namespace {

#if defined(PT_LBVH_MUTATE_KEEP_PAD)
constexpr bool kKeepPad = true;
#else
constexpr bool kKeepPad = false;
#endif

const char* const kSmall[] = {"tri2", "tri3", "tri4", "tri5", "tri8", "tri9", "copies9", "planar"};

Mesh lbvh_fixture(const std::string& name) {
  if (name.rfind("tri", 0) == 0) {   // the first T triangles of the icosahedron
    Mesh M = icosphere(0, 0.1);
    M.idx.resize(3 * (size_t)std::stoi(name.substr(3)));
    return M;
  }
  if (name == "copies9") {   // nine copies of one triangle: all codes equal
    Mesh M = single();
    for (int c = 1; c < 9; ++c) M.idx.insert(M.idx.end(), {0, 1, 2});
    return M;
  }
  if (name == "planar") {   // 5 x 3 cells in the plane y = -0.25: the centroids' extent along y is exactly 0
    Mesh M;
    for (int j = 0; j <= 3; ++j)
      for (int i = 0; i <= 5; ++i) M.v.insert(M.v.end(), {(float)i / 8.0f - 0.25f, -0.25f, (float)j / 8.0f - 3.0f});
    for (int j = 0; j < 3; ++j)
      for (int i = 0; i < 5; ++i) {
        const uint32_t a = (uint32_t)(j * 6 + i), b = a + 1, c = a + 6, d = c + 1;
        M.idx.insert(M.idx.end(), {b, d, c, a, b, c});
      }
    return M;
  }
  if (name.rfind("icosphere", 0) == 0) return icosphere(std::stoi(name.substr(9)), 0.1);   // (any level: scripts/mesh_build_bench.py --verify)
  return fixture(name);
}
bool is_small(const std::string& name) {
  for (const char* s : kSmall) if (name == s) return true;
  return false;
}

pt_camera pose_camera(int p) {
  pt_camera c = ptcamera::default_camera();
  const float cams[3][9] = {{0.5f, 0.3f, 0.4f, 0.2f, -0.2f, -3.0f, 0.f, 1.f, 0.f},      // moved
                            {-0.4f, 0.1f, 0.2f, 0.3f, -0.2f, -3.0f, 0.3f, 1.f, 0.1f},   // rolled
                            {0.3f, 0.2f, -6.5f, 0.3f, -0.2f, -3.0f, 0.f, 1.f, 0.f}};    // from behind
  for (int k = 0; k < 3; ++k) { c.position[k] = cams[p][k]; c.look_at[k] = cams[p][3 + k]; c.up[k] = cams[p][6 + k]; }
  return c;
}
const char* const kPoseName[3] = {"moved", "rolled", "behind"};

bool same_tree(const ptmesh::Built& A, const ptmesh::Built& B) {
  return A.nodes.size() == B.nodes.size() && !memcmp(A.nodes.data(), B.nodes.data(), A.nodes.size() * sizeof(ptmesh::Node)) && A.orig == B.orig &&
         A.tris.size() == B.tris.size() && !memcmp(A.tris.data(), B.tris.data(), A.tris.size() * sizeof(ptmesh::F4)) && A.depth == B.depth &&
         A.max_leaf == B.max_leaf && !memcmp(&A.pad, &B.pad, 4);
}

// check_subtree's invariants, then the boxes against the triangles' own (ptmesh::tri_box) and the pad of the builder's rule
void check_tree(const ptmesh::Built& B, const std::vector<float>& frames, uint32_t T, const std::string& tag) {
  const char* name = tag.c_str();
  CHECK(B.nodes.size() <= 2 * (size_t)T - 1 && B.orig.size() == T && B.tris.size() == 3 * (size_t)T, "%s: sizes", name);
  CHECK(B.max_leaf <= ptmesh::kMaxLeaf, "%s: max_leaf %u", name, B.max_leaf);
  if (B.orig.size() != T || B.nodes.empty()) return;
  std::vector<uint32_t> seen(T, 0);
  const uint32_t counted = check_subtree(B, frames, 0, (uint32_t)B.nodes.size(), seen, name);
  CHECK(counted == B.nodes.size(), "%s: %u nodes reached of %zu", name, counted, B.nodes.size());
  for (uint32_t j = 0; j < T; ++j) CHECK(seen[j] == 1, "%s: triangle %u is in %u leaves", name, j, seen[j]);
  ptmesh::Box all;
  all.clear();
  for (uint32_t j = 0; j < T; ++j) all.grow(ptmesh::tri_box(&frames[ptmesh::kFrameFloats * (size_t)j]));
  float big = 0.f;
  for (int k = 0; k < 3; ++k) big = std::max(big, std::max(std::fabs(all.lo[k]), std::fabs(all.hi[k])));
  const float pad = ptmesh::kPadScale * big;
  CHECK(!memcmp(&pad, &B.pad, 4), "%s: pad %.9g, the rule gives %.9g", name, (double)B.pad, (double)pad);
  for (size_t i = 0; i < B.nodes.size(); ++i) {
    const ptmesh::Node& N = B.nodes[i];
    ptmesh::Box box = all;
    if (i != 0) {
      if (N.leaf == 0u) continue;
      box.clear();
      for (uint32_t s = N.leaf >> ptmesh::kLeafCountBits; s < (N.leaf >> ptmesh::kLeafCountBits) + (N.leaf & 7u); ++s)
        box.grow(ptmesh::tri_box(&frames[ptmesh::kFrameFloats * (size_t)B.orig[s]]));
    }
    for (int k = 0; k < 3; ++k) {
      volatile float lo = box.lo[k] - pad, hi = box.hi[k] + pad;
      CHECK(N.lo[k] == lo && N.hi[k] == hi, "%s: node %zu axis %d: box [%.9g, %.9g], its triangles' padded box [%.9g, %.9g]", name, i, k,
            (double)N.lo[k], (double)N.hi[k], (double)lo, (double)hi);
    }
  }
}

// walk == brute force over R; returns the differences.  brute: computed once per frame (it does not depend on the tree).
size_t compare(const std::string& tag, const ptmesh::Built& B, const Rays& R, const Hits* brute, size_t* hits_out = nullptr) {
  const Hits W = trace(B, R, true);
  const Hits Y = brute ? *brute : trace(B, R, false);
  const size_t diff = differences(tag.c_str(), W, Y);
  size_t hits = 0;
  for (int32_t t : Y.tri) hits += t >= 0;
  CHECK(diff == 0, "%s: %zu of %zu rays differ between the walk and brute force", tag.c_str(), diff, W.t.size());
  if (hits_out) *hits_out = hits;
  return diff;
}

struct Posed {
  ptcamera::Basis basis;
  std::vector<float> frames;   // triangle order, in the camera's frame
  Mesh mesh;                   // the vertices as points through the transform (what the rays aim at)
};
Posed posed(const Mesh& M, const std::vector<float>& world, int p) {
  Posed P;
  const pt_camera cam = pose_camera(p);
  P.basis = ptcamera::basis(cam);
  P.frames.resize(world.size());
  ptmesh::kernel_frames(world.data(), M.triangles(), &P.basis, P.frames.data());
  P.mesh = M;
  for (size_t i = 0; i < M.v.size(); i += 3) ptcamera::to_camera_point(P.basis, &M.v[i], &P.mesh.v[i]);
  return P;
}

void run_fixture(const std::string& name) {
  const Mesh M = lbvh_fixture(name);
  const uint32_t T = M.triangles();
  const pt_mesh view = M.view();
  std::vector<float> world;
  ptmesh::world_frames(view, world);
  ptmesh::Built sah, lin, again, threads;
  ptmesh::build(world.data(), T, sah);
  ptlbvh::build(world.data(), T, lin);
  ptlbvh::build(world.data(), T, again);
  ptlbvh::build_threads(world.data(), T, threads);
  CHECK(same_tree(lin, again), "%s: two builds differ", name.c_str());
  CHECK(same_tree(lin, threads), "%s: the parallel form's tree differs from the reference builder's", name.c_str());
  check_tree(lin, world, T, name);
  // the world frame: the tree's own rays, and the SAH program's rays against the SAH walk
  const bool far = name == "grid";
  const Rays R = make_rays(M, lin, fixture_seed(name), far);
  const Hits Y = trace(lin, R, false);
  size_t hits = 0;
  const size_t diff = compare(name, lin, R, &Y, &hits);
  if (!is_small(name)) CHECK(R.o.size() / 3 >= kRays && hits * 16 >= R.o.size() / 3, "%s: %zu rays, %zu hits: too few", name.c_str(), R.o.size() / 3, hits);
  if (name == "doubled") {
    size_t odd = 0;
    for (int32_t t : Y.tri) odd += t >= 0 && (t & 1);
    CHECK(odd == 0, "doubled: %zu hits on the second copy of a triangle", odd);
  }
  const Rays Rs = make_rays(M, sah, fixture_seed(name), far);
  const size_t cross = differences((name + " (SAH rays)").c_str(), trace(lin, Rs, true), trace(sah, Rs, true));
  CHECK(cross == 0, "%s: %zu rays of the SAH tree's own differ between the two walks", name.c_str(), cross);
  printf("%-10s world  %5u triangles %5zu nodes depth %2u max leaf %u pad %.3g: %zu rays, %zu hits, %zu differences, %zu against the SAH walk\n",
         name.c_str(), T, lin.nodes.size(), lin.depth, lin.max_leaf, (double)lin.pad, R.o.size() / 3, hits, diff, cross);
  // a refit under the identity: the world tree's bytes
  for (const ptmesh::Built* src : {&sah, &lin}) {
    ptmesh::Built b = *src, bt = *src;
    ptlbvh::refit(b, world.data(), ptlbvh::pose_of(nullptr), ptlbvh::kPadScale, kKeepPad);
    ptlbvh::refit_threads(bt, world.data(), ptlbvh::pose_of(nullptr));
    CHECK(same_tree(b, *src) && same_tree(bt, *src), "%s: a refit of the %s tree under the identity changes it", name.c_str(), src == &sah ? "SAH" : "linear");
  }
  for (int p = 0; p < 3; ++p) {
    const Posed P = posed(M, world, p);
    const ptlbvh::Pose pose = ptlbvh::pose_of(&P.basis);
    for (uint32_t j = 0; j < T; ++j) {   // one transform for the host and the device
      float fr[12];
      ptlbvh::kernel_frame(pose, &world[12 * (size_t)j], fr);
      CHECK(!memcmp(fr, &P.frames[12 * (size_t)j], 48), "%s %s: triangle %u: kernel_frame differs from ptmesh::kernel_frames", name.c_str(), kPoseName[p], j);
    }
    ptmesh::Built rs = sah, rl = lin, rst = sah, rlt = lin, rebuilt, direct;
    ptlbvh::refit(rs, world.data(), pose, ptlbvh::kPadScale, kKeepPad);
    ptlbvh::refit(rl, world.data(), pose, ptlbvh::kPadScale, kKeepPad);
    ptlbvh::refit_threads(rst, world.data(), pose);
    ptlbvh::refit_threads(rlt, world.data(), pose);
    ptmesh::build(P.frames.data(), T, rebuilt);
    ptlbvh::build(P.frames.data(), T, direct);
    CHECK(same_tree(rs, rst) && same_tree(rl, rlt), "%s %s: the refit's thread form differs from the reference refit", name.c_str(), kPoseName[p]);
    const std::string tag = name + " " + kPoseName[p];
    check_tree(rs, P.frames, T, tag + " SAH refit");
    check_tree(rl, P.frames, T, tag + " linear refit");
    check_tree(direct, P.frames, T, tag + " linear build");
    CHECK(rs.nodes.size() == sah.nodes.size() && rs.orig == sah.orig && rl.nodes.size() == lin.nodes.size() && rl.orig == lin.orig,
          "%s: a refit changed the topology", tag.c_str());
    const Rays Rp = make_rays(P.mesh, rl, fixture_seed(name) + 17u * (uint64_t)(p + 1), false);
    const Hits Yp = trace(rl, Rp, false);
    size_t hp = 0;
    const size_t d0 = compare(tag + " SAH refit", rs, Rp, &Yp, &hp), d1 = compare(tag + " linear refit", rl, Rp, &Yp), d2 = compare(tag + " host rebuild", rebuilt, Rp, &Yp),
                 d3 = compare(tag + " linear build", direct, Rp, &Yp);
    printf("%-10s %-6s %zu rays, %zu hits: SAH refit %zu, linear refit %zu, host rebuild %zu, linear build %zu differences\n", name.c_str(), kPoseName[p],
           Rp.o.size() / 3, hp, d0, d1, d2, d3);
  }
}

bool put(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }
bool put_tree(FILE* f, const ptmesh::Built& B) {
  const uint32_t head[4] = {(uint32_t)B.nodes.size(), B.depth, B.max_leaf, 0u};
  return put(f, head, 16) && put(f, &B.pad, 4) && put(f, B.nodes.data(), B.nodes.size() * sizeof(ptmesh::Node)) && put(f, B.orig.data(), B.orig.size() * 4);
}
// The file: magic, n_vertices, n_triangles, n_rays; vertices; indices; ray origins; directions; t; triangle; two cameras (position,
// look_at, up: nine floats each); then seven trees (n_nodes, depth, max_leaf, 0, pad, nodes, orig): the linear tree in the world
// frame, under pose 0, under pose 1; the world linear tree refitted to pose 0, to pose 1; the world SAH tree refitted to pose 0,
// to pose 1; last, the world SAH tree itself.
int lbvh_dump(const std::string& name, const char* path) {
  const Mesh M = lbvh_fixture(name);
  const uint32_t T = M.triangles();
  const pt_mesh view = M.view();
  std::vector<float> world;
  ptmesh::world_frames(view, world);
  ptmesh::Built sah, lin;
  ptmesh::build(world.data(), T, sah);
  ptlbvh::build(world.data(), T, lin);
  const Rays R = make_rays(M, lin, fixture_seed(name), name == "grid");
  const Hits H = trace(lin, R, true);
  FILE* f = fopen(path, "wb");
  if (!f) { perror(path); return 2; }
  const uint32_t head[4] = {0x4c425648u, (uint32_t)(M.v.size() / 3), T, (uint32_t)H.t.size()};
  bool ok = put(f, head, 16) && put(f, M.v.data(), 4 * M.v.size()) && put(f, M.idx.data(), 4 * M.idx.size()) && put(f, R.o.data(), 4 * R.o.size()) &&
            put(f, R.d.data(), 4 * R.d.size()) && put(f, H.t.data(), 4 * H.t.size()) && put(f, H.tri.data(), 4 * H.tri.size());
  for (int p = 0; p < 2; ++p) {
    const pt_camera c = pose_camera(p);
    ok = ok && put(f, c.position, 12) && put(f, c.look_at, 12) && put(f, c.up, 12);
  }
  ok = ok && put_tree(f, lin);
  Posed P[2] = {posed(M, world, 0), posed(M, world, 1)};
  for (int p = 0; p < 2; ++p) {
    ptmesh::Built direct;
    ptlbvh::build(P[p].frames.data(), T, direct);
    ok = ok && put_tree(f, direct);
  }
  for (const ptmesh::Built* src : {&lin, &sah})
    for (int p = 0; p < 2; ++p) {
      ptmesh::Built r = *src;
      ptlbvh::refit(r, world.data(), ptlbvh::pose_of(&P[p].basis));
      ok = ok && put_tree(f, r);
    }
  ok = ok && put_tree(f, sah);
  ok = fclose(f) == 0 && ok;
  return ok ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "--dump")) return lbvh_dump(argv[2], argv[3]);
  const char* only = argc == 3 && !strcmp(argv[1], "--only") ? argv[2] : nullptr;
  if (argc != 1 && !only) { fprintf(stderr, "usage: %s [--dump FIXTURE FILE | --only FIXTURE]\n", argv[0]); return 2; }
  std::vector<std::string> names(kFixtures, kFixtures + sizeof(kFixtures) / sizeof(kFixtures[0]));
  names.insert(names.end(), kSmall, kSmall + sizeof(kSmall) / sizeof(kSmall[0]));
  for (const std::string& name : names)
    if (!only || name == only) run_fixture(name);
  if (g_failures) { printf("MESH_LBVH_FAILED %d\n", g_failures); return 1; }
  printf("MESH_LBVH_OK\n");
  return 0;
}
