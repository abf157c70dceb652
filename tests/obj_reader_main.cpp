// obj_reader_main.cpp -- the OBJ reader of --scene meshes (ipu_path_trace_amd/host/ObjReader.hpp) as a stand-alone program:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I ipu_path_trace_amd/host tests/obj_reader_main.cpp
// First the face forms it must read -- v, v/vt, v//vn, v/vt/vn, negative indices, quads and n-gons as fans, CR LF -- and the errors
// it must report; then a fuzz pass in the style of envmap_fuzz_main.cpp: every truncation of a seed file and thousands of byte
// corruptions of it, each of which must either parse or throw std::runtime_error, never crash or read outside the text.
// Prints OBJ_READER_OK.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "ObjReader.hpp"

namespace {

int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failures; fprintf(stderr, "FAIL line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

const char kSeed[] =
    "# a cube corner and a pentagon\r\n"
    "mtllib none.mtl\n"
    "o thing\n"
    "v 0 0 0\n"
    "v 1 0 0 1.0\r\n"
    "v 1 1 0\n"
    "  v   0 1 0\n"
    "vt 0.5 0.5\n"
    "vn 0 0 1\n"
    "v -0.5 0.5 1e-1\n"
    "s off\n"
    "f 1 2 3\n"
    "f 1/1 3/1 4/1\n"
    "f 1//1 2//1 3//1 4//1\r\n"
    "f 1/1/1 2/1/1 3/1/1 4/1/1 5/1/1\n"
    "f -1 -2 -3\n"
    "v 2 2 2\n"
    "f -1 1 2\n";

bool throws(const std::string& text, const char* part) {
  try { (void)objreader::parse(text); } catch (const std::runtime_error& e) { return std::string(e.what()).find(part) != std::string::npos; }
  return false;
}

void plain() {
  const objreader::Mesh m = objreader::parse(kSeed);
  const std::vector<float> v = {0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, -0.5f, 0.5f, 0.1f, 2, 2, 2};
  const std::vector<std::uint32_t> t = {0, 1, 2,  0, 2, 3,  0, 1, 2, 0, 2, 3,  0, 1, 2, 0, 2, 3, 0, 3, 4,  4, 3, 2,  5, 0, 1};
  CHECK(m.vertices == v, "vertices: %zu floats", m.vertices.size());
  CHECK(m.indices == t, "indices: %zu", m.indices.size());
  CHECK(throws("v 0 0 0\nv 1 0 0\nv 0 1 0\n", "no face"), "a file without a face");
  CHECK(throws("v 0 0\nf 1 1 1\n", "line 1: a vertex needs three numbers"), "a short vertex");
  CHECK(throws("v 0 0 x\nf 1 1 1\n", "a vertex needs three numbers"), "a vertex that is no number");
  CHECK(throws("v 0 0 0\nv 1 0 0\nf 1 2\n", "line 3: a face needs at least three corners"), "a short face");
  CHECK(throws("v 0 0 0\nf 1 1 0\n", "vertex index 0"), "index 0");
  CHECK(throws("v 0 0 0\nf 1 1 2\n", "vertex index 2 with 1 vertices read so far"), "an index beyond the vertices");
  CHECK(throws("v 0 0 0\nf 1 1 -2\n", "vertex index -2 with 1 vertices"), "a negative index beyond the vertices");
  CHECK(throws("v 0 0 0\nf 1 1 1\nf a b c\n", "line 3: a face corner must start with an integer"), "a corner that is no integer");
  CHECK(throws("v 0 0 0\nf 1/x 1 1\n", "must be v, v/vt, v//vn or v/vt/vn"), "a corner with letters");
  CHECK(throws("v 0 0 0\nf 1 1 99999999999999999999\n", "integer"), "an index out of range of long");
  // a later vertex is not yet there for an earlier face; an index counts the vertices read SO FAR
  CHECK(throws("v 0 0 0\nv 1 0 0\nf 1 2 3\nv 0 1 0\n", "vertex index 3 with 2 vertices"), "a forward reference");
}

void fuzz() {
  const std::string seed(kSeed);
  std::size_t parsed = 0, refused = 0;
  auto attempt = [&](const std::string& text) {
    try {
      const objreader::Mesh m = objreader::parse(text);
      for (std::uint32_t ix : m.indices) CHECK(ix < m.vertices.size() / 3, "an index %u beyond %zu vertices", ix, m.vertices.size() / 3);
      CHECK(m.indices.size() % 3 == 0 && m.vertices.size() % 3 == 0 && !m.indices.empty(), "sizes");
      ++parsed;
    } catch (const std::runtime_error&) { ++refused; }
  };
  for (std::size_t n = 0; n <= seed.size(); ++n) attempt(seed.substr(0, n));            // every truncation
  std::uint64_t s = 0x6f626a72ull;
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  const char alphabet[] = "vf/ -0123456789.e\r\n\t#x\0\xff";
  for (int k = 0; k < 20000; ++k) {                                                      // corruptions: 1 to 4 bytes replaced, or a span cut
    std::string text = seed;
    const int edits = 1 + (int)(next() % 4);
    for (int e = 0; e < edits; ++e) text[next() % text.size()] = alphabet[next() % (sizeof alphabet - 1)];
    if (next() % 4 == 0) { const std::size_t a = next() % text.size(); text.erase(a, next() % 16); }
    attempt(text);
  }
  attempt(std::string(1 << 16, 'f'));                                                   // long lines without an end
  attempt("f " + std::string(1 << 16, '1'));
  attempt("v " + std::string(1 << 16, '9') + " 0 0\nf 1 1 1\n");
  CHECK(parsed > 1000 && refused > 1000, "fuzz: %zu parsed, %zu refused", parsed, refused);
  printf("fuzz: %zu texts parsed, %zu refused\n", parsed, refused);
}

}  // namespace

int main() {
  plain();
  fuzz();
  if (g_failures) { printf("OBJ_READER_FAILED %d\n", g_failures); return 1; }
  printf("OBJ_READER_OK\n");
  return 0;
}
