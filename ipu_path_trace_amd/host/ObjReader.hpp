// ObjReader.hpp -- a dependency-free reader of Wavefront OBJ geometry for --scene's {"shape": "mesh", "file": "x.obj"}.
//
// It reads `v x y z [w]` and `f a b c ...` lines and NOTHING else: every other line (vt, vn, o, g, s, usemtl, mtllib, comments,
// blank lines) is skipped.  A face index is `v`, `v/vt`, `v//vn` or `v/vt/vn`; only the vertex index is used (shading is flat unless
// normals are asked for, below, and a mesh has one material: include/ptmi.h).  Indices count from 1; a negative index counts back from the vertices read SO FAR
// (-1 is the last one).  A face of more than three corners is triangulated as a fan about its first corner: (0, 1, 2), (0, 2, 3),
// ...  Lines end in LF or CR LF.  All vertices and all faces of the file make ONE mesh: objects and groups are not kept apart.
//
// Errors (a thrown std::runtime_error naming the line): a `v` with fewer than three numbers or one that is no number, an `f` with
// fewer than three corners, a corner that is no integer, index 0, an index beyond the vertices read so far, more than 2^22
// triangles, a file without a face.  Numbers are read with strtof / strtol on a bounded copy of the line: no line, however long or
// truncated, reads outside itself.
//
// Normals (parse_with_normals, read(path, true): --scene's "normals": "file").  `vn x y z` lines are read too, and the third field
// of every corner, `v//vn` or `v/vt/vn`, by the vertex rules: from 1, a negative index counts back from the normals read so far,
// fans are kept (corner k of a fan's triangle carries corner k's normal).  Mesh::normals and Mesh::normal_indices come back
// filled, one index triple per triangle, for pt_set_mesh_normals.  More errors: a `vn` with fewer than three numbers, a corner
// without a normal index (EVERY face must carry one), normal index 0 or beyond the normals read so far.
//
// Texture coordinates (parse_with_uvs: --scene's "uvs": "file").  `vt u [v [w]]` lines are read too -- v defaults to 0, w is
// ignored -- and the second field of every corner, `v/vt` or `v/vt/vn`, by the vertex rules: from 1, a negative index counts back
// from the texture coordinates read so far, fans are kept.  Mesh::uvs and Mesh::uv_indices come back filled, one index triple per
// triangle, for pt_set_mesh_texture; vertices and indices are parse()'s.  More errors: a `vt` without a number, a corner without a
// texture index (EVERY face must carry one), texture index 0 or beyond the texture coordinates read so far.
//
// All entries are one body, parse_lines<NORMALS, UVS>: the line loop, the numbers, the fan and the limits are written once, and what
// normals or texture coordinates add is compiled into their instance alone, so parse() never looks at either and behaves as it
// always has, and parse_with_normals() never looks at a texture coordinate.
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
  std::vector<float> normals;                  // [N][3]   (parse_with_normals alone fills these two)
  std::vector<std::uint32_t> normal_indices;   // [T][3]
  std::vector<float> uvs;                      // [N][2]   (parse_with_uvs alone fills these two)
  std::vector<std::uint32_t> uv_indices;       // [T][3]
};

constexpr std::size_t kMaxTriangles = std::size_t(1) << 22;   // = PT_MAX_MESH_TRIANGLES

inline bool blank(char c) { return c == ' ' || c == '\t' || c == '\r'; }

// The text of an OBJ file -> a mesh; NORMALS: with `vn` lines and the corners' normal indices, UVS: with `vt` lines and the corners'
// texture indices (see the head of this file).
template <bool NORMALS, bool UVS = false>
inline Mesh parse_lines(const std::string& text, const std::string& what) {
  static_assert(!(NORMALS && UVS), "one side table per pass");
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
    const bool vn = NORMALS && p[0] == 'v' && p[1] == 'n' && blank(p[2]);
    const bool vt = UVS && p[0] == 'v' && p[1] == 't' && blank(p[2]);
    if (!vn && !vt && ((p[0] != 'v' && p[0] != 'f') || !blank(p[1]))) continue;   // comments, everything else (and vn, vt unless asked for)
    const char kind = p[0];
    p += (vn || vt) ? 2 : 1;
    if (vt) {
      float st[2] = {0.f, 0.f};
      for (int k = 0; k < 2; ++k) {
        while (blank(*p)) ++p;
        char* stop = nullptr;
        const float x = std::strtof(p, &stop);
        if (stop == p) {
          if (k == 0) throw std::runtime_error(at + "a texture coordinate needs at least one number");
          break;   // `vt u`: v is 0
        }
        st[k] = x;
        p = stop;
      }
      m.uvs.insert(m.uvs.end(), st, st + 2);
      continue;
    }
    if (kind == 'v') {
      float xyz[3];
      for (int k = 0; k < 3; ++k) {
        while (blank(*p)) ++p;
        char* stop = nullptr;
        xyz[k] = std::strtof(p, &stop);
        if (stop == p) throw std::runtime_error(at + (vn ? "a normal needs three numbers" : "a vertex needs three numbers"));
        p = stop;
      }
      std::vector<float>& into = vn ? m.normals : m.vertices;
      into.insert(into.end(), xyz, xyz + 3);
      continue;
    }
    std::vector<std::uint32_t> corner, corner_n, corner_t;
    const long have = (long)(m.vertices.size() / 3), have_n = (long)(m.normals.size() / 3), have_t = (long)(m.uvs.size() / 2);
    // one integer of a corner against `count` items read so far; `what_ix` names it in messages
    auto index = [&](const char*& q, long count, const char* what_ix, const char* plural) {
      char* stop = nullptr;
      errno = 0;
      const long ix = std::strtol(q, &stop, 10);
      if (stop == q || errno == ERANGE)
        throw std::runtime_error(at + (NORMALS ? "a face corner must be v//vn or v/vt/vn with integer indices"
                                       : (UVS && q[-1] == '/') ? "a face corner must be v/vt or v/vt/vn with integer indices"
                                               : "a face corner must start with an integer vertex index"));
      if (ix == 0) throw std::runtime_error(at + what_ix + " index 0 (indices count from 1)");
      const long v = ix > 0 ? ix - 1 : count + ix;
      if (v < 0 || v >= count)
        throw std::runtime_error(at + what_ix + " index " + std::to_string(ix) + " with " + std::to_string(count) + " " + plural + " read so far");
      q = stop;
      return (std::uint32_t)v;
    };
    for (;;) {
      while (blank(*p)) ++p;
      if (*p == '\0') break;
      corner.push_back(index(p, have, "vertex", "vertices"));
      if constexpr (NORMALS) {
        // /vt/vn or //vn: the texture index is skipped, the normal index is needed
        const char* const none = "a face corner without a normal index (normals were asked for: every face needs v//vn or v/vt/vn)";
        if (*p != '/') throw std::runtime_error(at + none);
        ++p;
        while (*p == '-' || (*p >= '0' && *p <= '9')) ++p;   // vt, unused
        if (*p != '/') throw std::runtime_error(at + none);
        ++p;
        if (*p == '\0' || blank(*p)) throw std::runtime_error(at + none);
        corner_n.push_back(index(p, have_n, "normal", "normals"));
        if (*p != '\0' && !blank(*p)) throw std::runtime_error(at + "a face corner must be v//vn or v/vt/vn with integer indices");
      } else {
        if constexpr (UVS) {
          // /vt or /vt/vn: the texture index is needed, the normal index is skipped below
          const char* const none = "a face corner without a texture index (texture coordinates were asked for: every face needs v/vt or v/vt/vn)";
          if (*p != '/') throw std::runtime_error(at + none);
          ++p;
          if (*p == '\0' || blank(*p) || *p == '/') throw std::runtime_error(at + none);
          corner_t.push_back(index(p, have_t, "texture", "texture coordinates"));
        }
        while (*p != '\0' && !blank(*p)) {   // the rest of the corner: /vt, //vn, /vt/vn -- digits, '-' and '/' only
          if (*p != '/' && *p != '-' && (*p < '0' || *p > '9')) throw std::runtime_error(at + "a face corner must be v, v/vt, v//vn or v/vt/vn");
          ++p;
        }
      }
    }
    if (corner.size() < 3) throw std::runtime_error(at + "a face needs at least three corners");
    for (std::size_t k = 1; k + 1 < corner.size(); ++k) {
      if (m.indices.size() / 3 >= kMaxTriangles) throw std::runtime_error(at + "more than " + std::to_string(kMaxTriangles) + " triangles");
      m.indices.insert(m.indices.end(), {corner[0], corner[k], corner[k + 1]});
      if constexpr (NORMALS) m.normal_indices.insert(m.normal_indices.end(), {corner_n[0], corner_n[k], corner_n[k + 1]});
      if constexpr (UVS) m.uv_indices.insert(m.uv_indices.end(), {corner_t[0], corner_t[k], corner_t[k + 1]});
    }
  }
  if (m.indices.empty()) throw std::runtime_error(what + ": no face in the file");
  return m;
}

// `what` names the file in messages.
inline Mesh parse(const std::string& text, const std::string& what = "obj") { return parse_lines<false>(text, what); }
inline Mesh parse_with_normals(const std::string& text, const std::string& what = "obj") { return parse_lines<true>(text, what); }
inline Mesh parse_with_uvs(const std::string& text, const std::string& what = "obj") { return parse_lines<false, true>(text, what); }

inline Mesh read(const std::string& path, bool normals = false) {
  std::ifstream in(path, std::ios::binary);
  if (!in) throw std::runtime_error(path + ": cannot open the file");
  std::stringstream text;
  text << in.rdbuf();
  return normals ? parse_with_normals(text.str(), path) : parse(text.str(), path);
}
inline Mesh read_with_uvs(const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  if (!in) throw std::runtime_error(path + ": cannot open the file");
  std::stringstream text;
  text << in.rdbuf();
  return parse_with_uvs(text.str(), path);
}

}  // namespace objreader
