// obj_uvs_main.cpp -- the OBJ reader's path with texture coordinates (ipu_path_trace_amd/host/ObjReader.hpp: parse_with_uvs) as a
// stand-alone program:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ipu_path_trace_amd/host tests/obj_uvs_main.cpp
// The forms it must read -- v/vt, v/vt/vn, `vt u`, `vt u v w`, negative indices, fans -- the errors it must report, that parse() and
// parse_with_normals() return on the same texts what they returned before the entry existed (the geometry of the seed with every vt
// taken out; no uv field filled), and a fuzz pass: every truncation of the seed and 20000 corruptions of it, each of which parses to
// in-range indices or throws std::runtime_error, under all three entries.  Prints OBJ_UVS_OK.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "ObjReader.hpp"

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; fprintf(stderr, "FAIL line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

const char kSeed[] =
    "# a quad, a pentagon and a triangle, every face with texture coordinates and normals\r\n"
    "o thing\n"
    "v 0 0 0\n"
    "vt 0 0\n"
    "vn 0 0 1\n"
    "v 1 0 0 1.0\r\n"
    "v 1 1 0\n"
    "  vt   1 0.5 0.25\n"
    "v 0 1 0\n"
    "vn 0 1 0\n"
    "v -0.5 0.5 1e-1\n"
    "f 1/1/1 2/2/2 3/1/1 4/-1/-1\r\n"
    "vt -0.75\n"
    "f 1/3/2 2/1/1 3/2/2 4/-3/1 5/3/-2\n"
    "f -1/-1/-1 -2/-2/-2 -3/-3/-1\n";
// the same geometry without a texture coordinate anywhere: what parse_with_normals() must make of the seed
const char kNoUvs[] =
    "v 0 0 0\nvn 0 0 1\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 1 0\nv -0.5 0.5 1e-1\n"
    "f 1//1 2//2 3//1 4//-1\nf 1//2 2//1 3//2 4//1 5//-2\nf -1//-1 -2//-2 -3//-1\n";
const char kPlain[] =
    "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv -0.5 0.5 1e-1\nf 1 2 3 4\nf 1 2 3 4 5\nf -1 -2 -3\n";

bool throws(const std::string& text, const char* part) {
  try { (void)objreader::parse_with_uvs(text); } catch (const std::runtime_error& e) { return std::string(e.what()).find(part) != std::string::npos; }
  return false;
}

void plain() {
  const objreader::Mesh m = objreader::parse_with_uvs(kSeed);
  const std::vector<float> uv = {0, 0, 1, 0.5f, -0.75f, 0};
  const std::vector<std::uint32_t> t = {0, 1, 2, 0, 2, 3,  0, 1, 2, 0, 2, 3, 0, 3, 4,  4, 3, 2};
  const std::vector<std::uint32_t> tt = {0, 1, 0, 0, 0, 1,  2, 0, 1, 2, 1, 0, 2, 0, 2,  2, 1, 0};
  CHECK(m.uvs == uv, "uvs: %zu floats", m.uvs.size());
  CHECK(m.indices == t, "indices: %zu", m.indices.size());
  CHECK(m.uv_indices == tt, "uv indices: %zu", m.uv_indices.size());
  CHECK(m.normals.empty() && m.normal_indices.empty(), "parse_with_uvs() fills no normals");
  // v/vt corners without a normal field read the same
  const objreader::Mesh two = objreader::parse_with_uvs("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0.25 0.5\nvt 1 1\nf 1/1 2/2 3/-2\n");
  CHECK(two.uv_indices == (std::vector<std::uint32_t>{0, 1, 0}) && two.uvs == (std::vector<float>{0.25f, 0.5f, 1, 1}), "v/vt corners");
  // the older entries are untouched: they never look at a texture coordinate, and fill neither new field
  const objreader::Mesh a = objreader::parse(kSeed), b = objreader::parse(kPlain);
  CHECK(a.vertices == b.vertices && a.indices == b.indices && a.indices == t && m.vertices == a.vertices, "parse() on the seed");
  CHECK(a.uvs.empty() && a.uv_indices.empty() && a.normals.empty(), "parse() fills no uvs");
  const objreader::Mesh c = objreader::parse_with_normals(kSeed), d = objreader::parse_with_normals(kNoUvs);
  CHECK(c.vertices == d.vertices && c.indices == d.indices && c.normals == d.normals && c.normal_indices == d.normal_indices && c.indices == t,
        "parse_with_normals() on the seed");
  CHECK(c.uvs.empty() && c.uv_indices.empty() && c.normals.size() == 6, "parse_with_normals() fills no uvs");
  CHECK(throws("v 0 0 0\nvt \nf 1/1 1/1 1/1\n", "line 2: a texture coordinate needs at least one number"), "an empty vt");
  CHECK(throws("v 0 0 0\nvt x 1\nf 1/1 1/1 1/1\n", "a texture coordinate needs at least one number"), "a vt that is no number");
  CHECK(throws("v 0 0 0\nvt 0 0\nf 1/1 1 1/1\n", "line 3: a face corner without a texture index"), "a corner without a texture index");
  CHECK(throws("v 0 0 0\nvt 0 0\nf 1//1 1//1 1//1\n", "without a texture index"), "v//vn corners");
  CHECK(throws("v 0 0 0\nvt 0 0\nf 1/ 1/1 1/1\n", "without a texture index"), "an empty texture field");
  CHECK(throws("v 0 0 0\nvt 0 0\nf 1/0 1/1 1/1\n", "texture index 0"), "texture index 0");
  CHECK(throws("v 0 0 0\nvt 0 0\nf 1/2 1/1 1/1\n", "texture index 2 with 1 texture coordinates read so far"), "a texture index beyond the coordinates");
  CHECK(throws("v 0 0 0\nvt 0 0\nf 1/-2 1/1 1/1\n", "texture index -2 with 1 texture coordinates"), "a negative texture index beyond the coordinates");
  CHECK(throws("v 0 0 0\nf 1/1 1/1 1/1\nvt 0 0\n", "texture index 1 with 0 texture coordinates"), "a forward reference");
  CHECK(throws("v 0 0 0\nvt 0 0\nf 1/x 1/1 1/1\n", "v/vt or v/vt/vn with integer indices"), "a texture index with letters");
  CHECK(throws("v 0 0 0\nvt 0 0\nf 1/1x 1/1 1/1\n", "a face corner must be v, v/vt, v//vn or v/vt/vn"), "a corner with letters");
  CHECK(throws("v 0 0 0\nvt 0 0\nf 1/1 1/1\n", "a face needs at least three corners"), "a short face");
  CHECK(throws("v 0 0 0\nvt 0 0\nf 2/1 1/1 1/1\n", "vertex index 2 with 1 vertices"), "a vertex index beyond the vertices");
  CHECK(throws("v 0 0 0\nvt 0 0\n", "no face"), "a file without a face");
}

void fuzz() {
  const std::string seed(kSeed);
  std::size_t parsed = 0, refused = 0;
  auto attempt = [&](const std::string& text) {
    try {
      const objreader::Mesh m = objreader::parse_with_uvs(text);
      for (std::uint32_t ix : m.indices) CHECK(ix < m.vertices.size() / 3, "an index %u beyond %zu vertices", ix, m.vertices.size() / 3);
      for (std::uint32_t ix : m.uv_indices) CHECK(ix < m.uvs.size() / 2, "a uv index %u beyond %zu uvs", ix, m.uvs.size() / 2);
      CHECK(m.indices.size() % 3 == 0 && m.vertices.size() % 3 == 0 && m.uvs.size() % 2 == 0 && !m.indices.empty() &&
                m.uv_indices.size() == m.indices.size(), "sizes");
      ++parsed;
    } catch (const std::runtime_error&) { ++refused; }
    // the older entries on the same text: in-range or refused, and never a uv
    try {
      const objreader::Mesh m = objreader::parse(text);
      for (std::uint32_t ix : m.indices) CHECK(ix < m.vertices.size() / 3, "parse(): an index %u beyond %zu vertices", ix, m.vertices.size() / 3);
      CHECK(m.uvs.empty() && m.uv_indices.empty() && m.normals.empty() && m.normal_indices.empty(), "parse() filled a side table");
    } catch (const std::runtime_error&) {}
    try {
      const objreader::Mesh m = objreader::parse_with_normals(text);
      for (std::uint32_t ix : m.indices) CHECK(ix < m.vertices.size() / 3, "parse_with_normals(): an index %u beyond %zu vertices", ix, m.vertices.size() / 3);
      for (std::uint32_t ix : m.normal_indices) CHECK(ix < m.normals.size() / 3, "a normal index %u beyond %zu normals", ix, m.normals.size() / 3);
      CHECK(m.uvs.empty() && m.uv_indices.empty(), "parse_with_normals() filled a uv");
    } catch (const std::runtime_error&) {}
  };
  for (std::size_t n = 0; n <= seed.size(); ++n) attempt(seed.substr(0, n));            // every truncation
  std::uint64_t s = 0x6f626a74ull;
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  const char alphabet[] = "vtnf/ -0123456789.e\r\n\t#x\0\xff";
  for (int k = 0; k < 20000; ++k) {                                                      // corruptions: 1 to 4 bytes replaced, or a span cut
    std::string text = seed;
    const int edits = 1 + (int)(next() % 4);
    for (int e = 0; e < edits; ++e) text[next() % text.size()] = alphabet[next() % (sizeof alphabet - 1)];
    if (next() % 4 == 0) { const std::size_t a = next() % text.size(); text.erase(a, next() % 16); }
    attempt(text);
  }
  attempt(std::string(1 << 16, 'f'));
  attempt("f " + std::string(1 << 16, '1'));
  attempt("v 0 0 0\nvt 0 0\nf 1/" + std::string(1 << 16, '1') + " 1/1 1/1\n");
  attempt("vt " + std::string(1 << 16, '9') + " 0 0\nv 0 0 0\nf 1/1 1/1 1/1\n");
  attempt("vt 1\nv 0 0 0\nf 1/1" + std::string(1 << 16, '/') + " 1/1 1/1\n");
  CHECK(parsed > 1000 && refused > 1000, "fuzz: %zu parsed, %zu refused", parsed, refused);
  printf("fuzz: %zu texts parsed, %zu refused\n", parsed, refused);
}

}  // namespace

int main() {
  plain();
  fuzz();
  if (g_failures) { printf("OBJ_UVS_FAILED %d\n", g_failures); return 1; }
  printf("OBJ_UVS_OK\n");
  return 0;
}
