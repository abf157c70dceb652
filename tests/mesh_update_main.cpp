// mesh_update_main.cpp -- the rule of pt_update_mesh_vertices (ipu_path_trace_amd/csrc/pt_mesh_update.h) on the CPU, a stand-alone
// program:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -ffp-contract=off -I include -I ipu_path_trace_amd/csrc -I tests tests/mesh_update_main.cpp
// The yardstick is never the new code: it is ptmesh::world_frames, ptmesh::check, ptmesh::check_normals, ptmesh::corner_normals
// and ptlbvh::refit.  Fixtures, rays, tree invariants and the walk / brute-force comparison are those of tests/mesh_lbvh_main.cpp,
// by that program's own code (it is included below inside a namespace, so that its main is not this program's).
// For every fixture (an icosphere of 320 triangles, a grid, 1, 4, 5 and 9 triangles, slivers), in its original and deformed state:
//   * frames: frame_thread over all triangles == ptmesh::world_frames, byte for byte, and no fault is reported;
//   * tree: a SAH tree and a linear tree built on the ORIGINAL, refitted (ptlbvh::refit) to the deformed frames in the world frame
//     and under one pose: the tree invariants, and walk == brute force with 0 differences on 2^14 rays;
//   * normals: corner_normals_thread == ptmesh::corner_normals byte for byte, per vertex and per corner.
// Seeded bad inputs on the icosphere: the pass reports the triangle and the kind of fault that ptmesh::check / check_normals name in
// their message -- a NaN vertex, an inf vertex, vertices of 1e30 whose cross product overflows, an exactly collinear triangle, two
// bad triangles of which the later one is seeded first; a NaN normal, a zero normal, a normal whose dot overflows.
// Prints MESH_UPDATE_OK.  Built with -DPT_MESH_UPDATE_MUTATE_EDGE (e2 = v2 - v1) or -DPT_MESH_UPDATE_MUTATE_ANY (any offending
// triangle for the lowest) the program must FAIL: tests/test_mesh_update.py checks that it does.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "pt_mesh_build.h"
#include "pt_mesh_update.h"
#include "ptmi_mesh.h"

namespace programs {
#include "mesh_lbvh_main.cpp"
}
using namespace programs;

namespace {

constexpr uint32_t kUpdateRays = 1u << 14;

// v' = v * (1, 1.5, 0.75) + 0.1 * sin(3 * v[(1, 2, 0)]) + (0.2, 0, 0), in binary32
Mesh deformed(const Mesh& M) {
  Mesh D = M;
  const float scale[3] = {1.0f, 1.5f, 0.75f}, shift[3] = {0.2f, 0.0f, 0.0f};
  for (size_t i = 0; i < M.v.size(); i += 3)
    for (int k = 0; k < 3; ++k) D.v[i + k] = M.v[i + k] * scale[k] + 0.1f * sinf(3.0f * M.v[i + (k + 1) % 3]) + shift[k];
  return D;
}

Rays every_nth(const Rays& R, size_t want) {
  const size_t n = R.o.size() / 3, step = std::max<size_t>(1, n / want);
  Rays out;
  for (size_t i = 0; i < n && out.o.size() / 3 < want; i += step) push(out, &R.o[3 * i], &R.d[3 * i]);
  return out;
}

void check_frames(const std::string& tag, const Mesh& M) {
  const uint32_t T = M.triangles();
  std::vector<float> want, got(ptupdate::kFrameFloats * (size_t)T);
  ptmesh::world_frames(M.view(), want);
  const uint64_t word = ptupdate::frames_pass(T, M.idx.data(), M.v.data(), got.data());
  CHECK(word == ptupdate::kNoFault, "%s: a fault (triangle %u, status %u) on a valid mesh", tag.c_str(), ptupdate::fault_triangle(word), ptupdate::fault_status(word));
  CHECK(want.size() == got.size(), "%s: frame counts", tag.c_str());
  for (uint32_t j = 0; j < T && want.size() == got.size(); ++j)
    CHECK(!memcmp(&want[12 * (size_t)j], &got[12 * (size_t)j], 48), "%s: triangle %u: frame_thread differs from ptmesh::world_frames", tag.c_str(), j);
}

void check_normals_bytes(const std::string& tag, const Mesh& M) {
  const uint32_t T = M.triangles(), V = (uint32_t)(M.v.size() / 3);
  std::vector<float> nv(M.v.size());   // per vertex: v - centre, NOT of unit length
  for (size_t i = 0; i < M.v.size(); ++i) nv[i] = (M.v[i] - (float)kCentre[i % 3]) * 3.0f + 0.01f;
  std::vector<uint32_t> nidx(M.idx.size());   // per corner: another lookup into the same array
  for (size_t e = 0; e < nidx.size(); ++e) nidx[e] = (M.idx[e] * 7u + (uint32_t)e) % V;
  for (const uint32_t* ix : {(const uint32_t*)nullptr, (const uint32_t*)nidx.data()}) {
    CHECK(ptmesh::check_normals(0, V, T, M.idx.data(), nv.data(), V, ix).empty(), "%s: the normals are not valid", tag.c_str());
    std::vector<float> want, got(9 * (size_t)T);
    ptmesh::corner_normals(T, M.idx.data(), nv.data(), ix, want);
    const uint64_t word = ptupdate::corner_normals_pass(T, ix ? ix : M.idx.data(), nv.data(), got.data());
    CHECK(word == ptupdate::kNoFault, "%s: a normal fault on valid normals", tag.c_str());
    CHECK(want.size() == got.size() && !memcmp(want.data(), got.data(), 4 * want.size()), "%s: corner_normals_thread differs from ptmesh::corner_normals (%s)",
          tag.c_str(), ix ? "per corner" : "per vertex");
  }
}

void check_refit(const std::string& name, const Mesh& M0, const Mesh& M1) {
  const uint32_t T = M0.triangles();
  std::vector<float> world0, world1;
  ptmesh::world_frames(M0.view(), world0);
  ptmesh::world_frames(M1.view(), world1);
  ptmesh::Built sah, lin;
  ptmesh::build(world0.data(), T, sah);
  ptlbvh::build(world0.data(), T, lin);
  for (int frame = 0; frame < 2; ++frame) {   // the world frame, then pose 0
    const Posed P = posed(M1, world1, 0);
    const ptlbvh::Pose pose = frame ? ptlbvh::pose_of(&P.basis) : ptlbvh::pose_of(nullptr);
    const std::vector<float>& frames = frame ? P.frames : world1;
    const Mesh& aim = frame ? P.mesh : M1;
    Rays R;
    Hits Y;
    for (const ptmesh::Built* src : {&sah, &lin}) {
      const std::string tag = name + (frame ? " posed" : " world") + (src == &sah ? " SAH refit" : " linear refit");
      ptmesh::Built B = *src;
      ptlbvh::refit(B, world1.data(), pose);
      check_tree(B, frames, T, tag);
      CHECK(B.nodes.size() == src->nodes.size() && B.orig == src->orig, "%s: the refit changed the topology", tag.c_str());
      if (R.o.empty()) {
        R = every_nth(make_rays(aim, B, fixture_seed(name) + 101u * (uint64_t)(frame + 1), false), kUpdateRays);
        Y = trace(B, R, false);
      }
      size_t hits = 0;
      const size_t diff = compare(tag, B, R, &Y, &hits);
      printf("%-28s %5u triangles: %zu rays, %zu hits, %zu differences\n", tag.c_str(), T, R.o.size() / 3, hits, diff);
      if (T >= 100) CHECK(R.o.size() / 3 == kUpdateRays && hits * 16 >= kUpdateRays, "%s: %zu rays, %zu hits: too few", tag.c_str(), R.o.size() / 3, hits);
    }
  }
}

// ---- seeded faults: what the messages of ptmesh::check / check_normals name

bool named(const std::string& message, uint32_t& triangle, uint32_t& status) {
  const size_t at = message.find("triangle ");
  if (at == std::string::npos) return false;
  triangle = (uint32_t)std::stoul(message.substr(at + 9));
  if (message.find("dot(n, n)") != std::string::npos) status = ptupdate::kNormalNoLength;
  else if (message.find("normals[") != std::string::npos) status = ptupdate::kNormalNotFinite;
  else if (message.find("vertices[") != std::string::npos) status = ptupdate::kVertexNotFinite;
  else if (message.find("vertex differences") != std::string::npos) status = ptupdate::kFrameNotFinite;
  else if (message.find("collinear") != std::string::npos) status = ptupdate::kCollinear;
  else return false;
  return true;
}

void expect_vertex_fault(const char* what, const Mesh& M, uint32_t status_wanted, bool several) {
  pt_scene_object_ex row{};
  row.shape = PT_SHAPE_MESH;
  row.material = PT_MATERIAL_DIFFUSE;
  row.colour[0] = row.colour[1] = row.colour[2] = 0.5f;
  const pt_mesh view = M.view();
  const std::string message = ptmesh::check(&row, 1, sizeof(row), &view, 1);
  uint32_t tri = 0, status = 0;
  CHECK(named(message, tri, status), "%s: ptmesh::check names no triangle: '%s'", what, message.c_str());
  CHECK(status == status_wanted, "%s: the fixture seeds another fault: '%s'", what, message.c_str());
  std::vector<float> frames(12 * (size_t)M.triangles());
  const uint64_t word = ptupdate::frames_pass(M.triangles(), M.idx.data(), M.v.data(), frames.data());
  CHECK(word != ptupdate::kNoFault && ptupdate::fault_triangle(word) == tri && ptupdate::fault_status(word) == status,
        "%s: the pass reports (triangle %u, status %u), ptmesh::check says '%s'", what, ptupdate::fault_triangle(word), ptupdate::fault_status(word), message.c_str());
  uint32_t bad = 0;
  for (uint32_t j = 0; j < M.triangles(); ++j) bad += ptupdate::frame_thread(j, M.idx.data(), M.v.data(), frames.data()) != ptupdate::kStatusOk;
  if (several) CHECK(bad >= 2 && tri + 1 < M.triangles(), "%s: %u offending triangle(s): the lowest-index rule is not exercised", what, bad);
  printf("%-34s triangle %3u status %u (%u offending): %s\n", what, tri, status, bad, message.c_str());
}

void set_vertex(Mesh& M, uint32_t vertex, float x, float y, float z) { M.v[3 * (size_t)vertex] = x; M.v[3 * (size_t)vertex + 1] = y; M.v[3 * (size_t)vertex + 2] = z; }

void vertex_faults(const Mesh& good) {
  const uint32_t T = good.triangles();
  const uint32_t* late = &good.idx[3 * (size_t)(T - 20)];   // a triangle near the end ...
  const uint32_t* early = &good.idx[3 * 40];                // ... and one before it
  {
    Mesh M = good;
    M.v[3 * (size_t)late[1] + 2] = NAN;
    expect_vertex_fault("a NaN vertex", M, ptupdate::kVertexNotFinite, true);   // (a vertex of the icosphere lies in five or six triangles)
  }
  {
    Mesh M = good;
    M.v[3 * (size_t)late[2]] = -INFINITY;
    expect_vertex_fault("an inf vertex", M, ptupdate::kVertexNotFinite, true);
  }
  {
    Mesh M = good;   // every vertex about 1e30: finite vertices and differences, every cross product overflows
    for (float& x : M.v) x *= 1e31f;
    expect_vertex_fault("a cross product that overflows", M, ptupdate::kFrameNotFinite, true);
  }
  {
    Mesh M = good;
    set_vertex(M, late[0], 0.25f, 0.5f, -3.0f); set_vertex(M, late[1], 0.5f, 0.5f, -3.0f); set_vertex(M, late[2], 1.0f, 0.5f, -3.0f);
    expect_vertex_fault("an exactly collinear triangle", M, ptupdate::kCollinear, false);
  }
  {
    Mesh M = good;   // the later triangle's fault is of the kind a loop would meet first in a triangle; the earlier triangle must still win
    M.v[3 * (size_t)late[0] + 1] = NAN;
    set_vertex(M, early[0], 0.25f, 0.5f, -3.0f); set_vertex(M, early[1], 0.5f, 0.5f, -3.0f); set_vertex(M, early[2], 1.0f, 0.5f, -3.0f);
    expect_vertex_fault("two bad triangles", M, ptupdate::kCollinear, true);
  }
}

void expect_normal_fault(const char* what, const Mesh& M, const std::vector<float>& normals, const uint32_t* nidx, uint32_t status_wanted) {
  const uint32_t T = M.triangles(), N = (uint32_t)(normals.size() / 3);
  const std::string message = ptmesh::check_normals(1, (uint32_t)(M.v.size() / 3), T, M.idx.data(), normals.data(), N, nidx);
  uint32_t tri = 0, status = 0;
  CHECK(named(message, tri, status), "%s: check_normals names no triangle: '%s'", what, message.c_str());
  CHECK(status_wanted == 0u || status == status_wanted, "%s: the fixture seeds another fault: '%s'", what, message.c_str());
  std::vector<float> corner(9 * (size_t)T);
  const uint64_t word = ptupdate::corner_normals_pass(T, nidx ? nidx : M.idx.data(), normals.data(), corner.data());
  CHECK(word != ptupdate::kNoFault && ptupdate::fault_triangle(word) == tri && ptupdate::fault_status(word) == status,
        "%s: the pass reports (triangle %u, status %u), check_normals says '%s'", what, ptupdate::fault_triangle(word), ptupdate::fault_status(word), message.c_str());
  printf("%-34s triangle %3u status %u: %s\n", what, tri, status, message.c_str());
}

void normal_faults(const Mesh& M) {
  const uint32_t T = M.triangles(), V = (uint32_t)(M.v.size() / 3);
  std::vector<float> good(M.v.size());
  for (size_t i = 0; i < M.v.size(); ++i) good[i] = (M.v[i] - (float)kCentre[i % 3]) * 3.0f + 0.01f;
  std::vector<uint32_t> nidx(M.idx.size());
  for (size_t e = 0; e < nidx.size(); ++e) nidx[e] = (M.idx[e] * 7u + (uint32_t)e) % V;
  const uint32_t late = M.idx[3 * (size_t)(T - 20) + 1], early = M.idx[3 * 40 + 2];
  for (const uint32_t* ix : {(const uint32_t*)nullptr, (const uint32_t*)nidx.data()}) {
    const uint32_t a = ix ? ix[3 * (size_t)(T - 20) + 1] : late, b = ix ? ix[3 * 40 + 2] : early;
    std::vector<float> n = good;
    n[3 * (size_t)a + 1] = NAN;
    expect_normal_fault(ix ? "a NaN normal (per corner)" : "a NaN normal", M, n, ix, ptupdate::kNormalNotFinite);
    n = good;
    n[3 * (size_t)a] = n[3 * (size_t)a + 1] = n[3 * (size_t)a + 2] = 0.f;
    expect_normal_fault(ix ? "a zero normal (per corner)" : "a zero normal", M, n, ix, ptupdate::kNormalNoLength);
    n = good;
    n[3 * (size_t)a + 2] = 1e30f;
    expect_normal_fault(ix ? "dot(n, n) overflows (per corner)" : "dot(n, n) overflows", M, n, ix, ptupdate::kNormalNoLength);
    n = good;
    n[3 * (size_t)a + 2] = NAN;
    n[3 * (size_t)b] = n[3 * (size_t)b + 1] = n[3 * (size_t)b + 2] = 0.f;
    expect_normal_fault(ix ? "two bad normals (per corner)" : "two bad normals", M, n, ix, 0u);   // (whichever check_normals meets first)
  }
}

}  // namespace

int main() {
  const char* const names[] = {"icosphere2", "grid", "single", "tri4", "tri5", "tri9", "sliver"};
  for (const char* name : names) {
    const Mesh M0 = lbvh_fixture(name), M1 = deformed(M0);
    check_frames(std::string(name) + " original", M0);
    check_frames(std::string(name) + " deformed", M1);
    check_normals_bytes(std::string(name) + " original", M0);
    check_normals_bytes(std::string(name) + " deformed", M1);
    check_refit(name, M0, M1);
  }
  const Mesh ball = deformed(lbvh_fixture("icosphere2"));
  vertex_faults(ball);
  normal_faults(ball);
  if (g_failures) { printf("MESH_UPDATE_FAILED %d\n", g_failures); return 1; }
  printf("MESH_UPDATE_OK\n");
  return 0;
}
