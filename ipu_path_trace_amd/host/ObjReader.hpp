// ObjReader.hpp -- a dependency-free reader of Wavefront OBJ geometry for --scene's {"shape": "mesh", "file": "x.obj"}.
//
// It reads `v x y z [w]` and `f a b c ...` lines and NOTHING else: every other line (vt, vn, o, g, s, usemtl, mtllib, comments,
// blank lines) is skipped.  A face index is `v`, `v/vt`, `v//vn` or `v/vt/vn`; only the vertex index is used (shading is flat and a
// mesh has one material: include/ptmi.h).  Indices count from 1; a negative index counts back from the vertices read SO FAR
// (-1 is the last one).  A face of more than three corners is triangulated as a fan about its first corner: (0, 1, 2), (0, 2, 3),
// ...  Lines end in LF or CR LF.  All vertices and all faces of the file make ONE mesh: objects and groups are not kept apart.
//
// Errors (a thrown std::runtime_error naming the line): a `v` with fewer than three numbers or one that is no number, an `f` with
// fewer than three corners, a corner that is no integer, index 0, an index beyond the vertices read so far, more than 2^22
// triangles, a file without a face.  Numbers are read with strtof / strtol on a bounded copy of the line: no line, however long or
// truncated, reads outside itself.
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace objreader {

struct Mesh {
  std::vector<float> vertices;          // [V][3]
  std::vector<std::uint32_t> indices;   // [T][3]
};

constexpr std::size_t kMaxTriangles = std::size_t(1) << 22;   // = PT_MAX_MESH_TRIANGLES

inline bool blank(char c) { return c == ' ' || c == '\t' || c == '\r'; }

// The text of an OBJ file -> a mesh.  `what` names the file in messages.
inline Mesh parse(const std::string& text, const std::string& what = "obj") {
  Mesh m;
  std::size_t pos = 0, line_no = 0;
  while (pos < text.size()) {
    std::size_t end = text.find('\n', pos);
    if (end == std::string::npos) end = text.size();
    const std::string line = text.substr(pos, end - pos);   // (a copy: c_str() ends it for strtof / strtol)
    pos = end + 1;
    line_no += 1;
    const std::string at = what + ": line " + std::to_string(line_no) + ": ";
    const char* p = line.c_str();
    while (blank(*p)) ++p;
    if ((p[0] != 'v' && p[0] != 'f') || !blank(p[1])) continue;   // vt, vn, comments, everything else
    const char kind = p[0];
    p += 1;
    if (kind == 'v') {
      float xyz[3];
      for (int k = 0; k < 3; ++k) {
        while (blank(*p)) ++p;
        char* stop = nullptr;
        xyz[k] = std::strtof(p, &stop);
        if (stop == p) throw std::runtime_error(at + "a vertex needs three numbers");
        p = stop;
      }
      m.vertices.insert(m.vertices.end(), xyz, xyz + 3);
      continue;
    }
    std::vector<std::uint32_t> corner;
    const long have = (long)(m.vertices.size() / 3);
    for (;;) {
      while (blank(*p)) ++p;
      if (*p == '\0') break;
      char* stop = nullptr;
      errno = 0;
      const long ix = std::strtol(p, &stop, 10);
      if (stop == p || errno == ERANGE) throw std::runtime_error(at + "a face corner must start with an integer vertex index");
      if (ix == 0) throw std::runtime_error(at + "vertex index 0 (indices count from 1)");
      const long v = ix > 0 ? ix - 1 : have + ix;
      if (v < 0 || v >= have)
        throw std::runtime_error(at + "vertex index " + std::to_string(ix) + " with " + std::to_string(have) + " vertices read so far");
      corner.push_back((std::uint32_t)v);
      p = stop;
      while (*p != '\0' && !blank(*p)) {   // the rest of the corner: /vt, //vn, /vt/vn -- digits, '-' and '/' only
        if (*p != '/' && *p != '-' && (*p < '0' || *p > '9')) throw std::runtime_error(at + "a face corner must be v, v/vt, v//vn or v/vt/vn");
        ++p;
      }
    }
    if (corner.size() < 3) throw std::runtime_error(at + "a face needs at least three corners");
    for (std::size_t k = 1; k + 1 < corner.size(); ++k) {
      if (m.indices.size() / 3 >= kMaxTriangles) throw std::runtime_error(at + "more than " + std::to_string(kMaxTriangles) + " triangles");
      m.indices.insert(m.indices.end(), {corner[0], corner[k], corner[k + 1]});
    }
  }
  if (m.indices.empty()) throw std::runtime_error(what + ": no face in the file");
  return m;
}

inline Mesh read(const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  if (!in) throw std::runtime_error(path + ": cannot open the file");
  std::stringstream text;
  text << in.rdbuf();
  return parse(text.str(), path);
}

}  // namespace objreader
