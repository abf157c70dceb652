// obj_normals_main.cpp -- the OBJ reader's path with normals (ipu_path_trace_amd/host/ObjReader.hpp: parse_with_normals) as a
// stand-alone program:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ipu_path_trace_amd/host tests/obj_normals_main.cpp
// The forms it must read -- v//vn, v/vt/vn, negative indices, fans -- the errors it must report, that parse() without normals
// returns on the seed what it returns on the seed with every normal taken out, and a fuzz pass: every truncation of the seed and
// 20000 corruptions of it, each of which parses to in-range indices or throws std::runtime_error.  Prints OBJ_NORMALS_OK.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "ObjReader.hpp"

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; fprintf(stderr, "FAIL line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

const char kSeed[] =
    "# a quad, a pentagon and a triangle, every face with normals\r\n"
    "o thing\n"
    "v 0 0 0\n"
    "vn 0 0 1\n"
    "v 1 0 0 1.0\r\n"
    "v 1 1 0\n"
    "  vn   0 1 0\n"
    "v 0 1 0\n"
    "vt 0.5 0.5\n"
    "v -0.5 0.5 1e-1\n"
    "f 1//1 2//2 3//1 4//-1\r\n"
    "vn 1 0 0\n"
    "f 1/1/3 2/1/1 3/1/2 4/1/-3 5/1/3\n"
    "f -1//-1 -2//-2 -3//-3\n";
// the same geometry without a normal anywhere: what parse() must make of the seed
const char kPlain[] =
    "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv -0.5 0.5 1e-1\nf 1 2 3 4\nf 1 2 3 4 5\nf -1 -2 -3\n";

bool throws(const std::string& text, const char* part) {
  try { (void)objreader::parse_with_normals(text); } catch (const std::runtime_error& e) { return std::string(e.what()).find(part) != std::string::npos; }
  return false;
}

void plain() {
  const objreader::Mesh m = objreader::parse_with_normals(kSeed);
  const std::vector<float> n = {0, 0, 1, 0, 1, 0, 1, 0, 0};
  const std::vector<std::uint32_t> t = {0, 1, 2, 0, 2, 3,  0, 1, 2, 0, 2, 3, 0, 3, 4,  4, 3, 2};
  const std::vector<std::uint32_t> tn = {0, 1, 0, 0, 0, 1,  2, 0, 1, 2, 1, 0, 2, 0, 2,  2, 1, 0};
  CHECK(m.normals == n, "normals: %zu floats", m.normals.size());
  CHECK(m.indices == t, "indices: %zu", m.indices.size());
  CHECK(m.normal_indices == tn, "normal indices: %zu", m.normal_indices.size());
  // the default path is untouched: it never looks at a normal, and fills neither new field
  const objreader::Mesh a = objreader::parse(kSeed), b = objreader::parse(kPlain);
  CHECK(a.vertices == b.vertices && a.indices == b.indices && a.indices == t, "parse() on the seed");
  CHECK(a.normals.empty() && a.normal_indices.empty() && m.vertices == a.vertices, "parse() fills no normals");
  CHECK(throws("v 0 0 0\nvn 0 0\nf 1//1 1//1 1//1\n", "line 2: a normal needs three numbers"), "a short normal");
  CHECK(throws("v 0 0 0\nvn 0 0 1\nf 1//1 1 1//1\n", "line 3: a face corner without a normal index"), "a corner without a normal");
  CHECK(throws("v 0 0 0\nvn 0 0 1\nf 1/1 1/1 1/1\n", "without a normal index"), "v/vt corners");
  CHECK(throws("v 0 0 0\nvn 0 0 1\nf 1// 1//1 1//1\n", "without a normal index"), "an empty normal field");
  CHECK(throws("v 0 0 0\nvn 0 0 1\nf 1//0 1//1 1//1\n", "normal index 0"), "normal index 0");
  CHECK(throws("v 0 0 0\nvn 0 0 1\nf 1//2 1//1 1//1\n", "normal index 2 with 1 normals read so far"), "a normal index beyond the normals");
  CHECK(throws("v 0 0 0\nvn 0 0 1\nf 1//-2 1//1 1//1\n", "normal index -2 with 1 normals"), "a negative normal index beyond the normals");
  CHECK(throws("v 0 0 0\nf 1//1 1//1 1//1\nvn 0 0 1\n", "normal index 1 with 0 normals"), "a forward reference");
  CHECK(throws("v 0 0 0\nvn 0 0 1\nf 1//1x 1//1 1//1\n", "integer indices"), "a corner with letters");
  CHECK(throws("v 0 0 0\nvn 0 0 1\nf 1//1 1//1\n", "a face needs at least three corners"), "a short face");
  CHECK(throws("v 0 0 0\nvn 0 0 1\nf 2//1 1//1 1//1\n", "vertex index 2 with 1 vertices"), "a vertex index beyond the vertices");
  CHECK(throws("v 0 0 0\nvn 0 0 1\n", "no face"), "a file without a face");
}

void fuzz() {
  const std::string seed(kSeed);
  std::size_t parsed = 0, refused = 0;
  auto attempt = [&](const std::string& text) {
    try {
      const objreader::Mesh m = objreader::parse_with_normals(text);
      for (std::uint32_t ix : m.indices) CHECK(ix < m.vertices.size() / 3, "an index %u beyond %zu vertices", ix, m.vertices.size() / 3);
      for (std::uint32_t ix : m.normal_indices) CHECK(ix < m.normals.size() / 3, "a normal index %u beyond %zu normals", ix, m.normals.size() / 3);
      CHECK(m.indices.size() % 3 == 0 && m.vertices.size() % 3 == 0 && m.normals.size() % 3 == 0 && !m.indices.empty() &&
                m.normal_indices.size() == m.indices.size(), "sizes");
      ++parsed;
    } catch (const std::runtime_error&) { ++refused; }
  };
  for (std::size_t n = 0; n <= seed.size(); ++n) attempt(seed.substr(0, n));            // every truncation
  std::uint64_t s = 0x6f626a6eull;
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  const char alphabet[] = "vnf/ -0123456789.e\r\n\t#x\0\xff";
  for (int k = 0; k < 20000; ++k) {                                                      // corruptions: 1 to 4 bytes replaced, or a span cut
    std::string text = seed;
    const int edits = 1 + (int)(next() % 4);
    for (int e = 0; e < edits; ++e) text[next() % text.size()] = alphabet[next() % (sizeof alphabet - 1)];
    if (next() % 4 == 0) { const std::size_t a = next() % text.size(); text.erase(a, next() % 16); }
    attempt(text);
  }
  attempt(std::string(1 << 16, 'f'));
  attempt("f " + std::string(1 << 16, '1'));
  attempt("v 0 0 0\nvn 0 0 1\nf 1//" + std::string(1 << 16, '1') + " 1//1 1//1\n");
  attempt("vn " + std::string(1 << 16, '9') + " 0 0\nv 0 0 0\nf 1//1 1//1 1//1\n");
  CHECK(parsed > 1000 && refused > 1000, "fuzz: %zu parsed, %zu refused", parsed, refused);
  printf("fuzz: %zu texts parsed, %zu refused\n", parsed, refused);
}

}  // namespace

int main() {
  plain();
  fuzz();
  if (g_failures) { printf("OBJ_NORMALS_FAILED %d\n", g_failures); return 1; }
  printf("OBJ_NORMALS_OK\n");
  return 0;
}
