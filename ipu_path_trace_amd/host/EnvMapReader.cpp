#include "EnvMapReader.hpp"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>

namespace env_map {
namespace {

// The whole file in memory and a cursor over it: every read is checked against the end first.
struct Bytes {
  std::string file;
  std::vector<std::uint8_t> d;
  std::size_t p = 0;

  [[noreturn]] void bad(const std::string& what, std::size_t at) const {
    throw std::runtime_error("'" + file + "': " + what + " at offset " + std::to_string(at) + " (file size " + std::to_string(d.size()) + ")");
  }
  [[noreturn]] void bad(const std::string& what) const { bad(what, p); }
  std::size_t left() const { return d.size() - p; }
  void need(std::size_t n, const char* what) const {
    if (n > left()) bad(std::string("truncated ") + what);
  }
  std::uint8_t byte(const char* what) { need(1, what); return d[p++]; }
  template <typename T>
  T get(const char* what) {
    need(sizeof(T), what);
    T v;
    std::memcpy(&v, &d[p], sizeof(T));
    p += sizeof(T);
    return v;
  }
  // text up to (not including) `end`, which is consumed; at most `limit` characters
  std::string until(char end, std::size_t limit, const char* what) {
    const std::size_t start = p;
    while (p < d.size() && d[p] != (std::uint8_t)end) {
      if (p - start >= limit) bad(std::string("over-long ") + what, start);
      ++p;
    }
    if (p >= d.size()) bad(std::string("truncated ") + what, start);
    std::string s(reinterpret_cast<const char*>(&d[start]), p - start);
    ++p;
    return s;
  }
};

void checkSize(const Bytes& b, long long w, long long h, std::size_t at) {
  if (w < 1 || h < 1 || w > (long long)kMaxSize || h > (long long)kMaxSize)
    b.bad("image size " + std::to_string(w) + " x " + std::to_string(h) + " is outside 1.." + std::to_string(kMaxSize), at);
}

// ---- Radiance RGBE
void rgbeToBgr(const std::uint8_t* px, float* bgr) {
  if (px[3] == 0) { bgr[0] = bgr[1] = bgr[2] = 0.f; return; }
  const float f = std::ldexp(1.0f, (int)px[3] - 136);
  bgr[0] = (float)px[2] * f;
  bgr[1] = (float)px[1] * f;
  bgr[2] = (float)px[0] * f;
}

Image readHdr(Bytes& b) {
  const std::string magic = b.until('\n', 64, "signature line");
  if (magic != "#?RADIANCE" && magic != "#?RGBE") b.bad("not a Radiance picture (the first line must be #?RADIANCE or #?RGBE)", 0);
  bool format = false;
  for (;;) {
    const std::size_t at = b.p;
    const std::string line = b.until('\n', 4096, "header line");
    if (line.empty()) break;
    if (line.compare(0, 7, "FORMAT=") == 0) {
      if (line != "FORMAT=32-bit_rle_rgbe") b.bad("unsupported " + line + " (only FORMAT=32-bit_rle_rgbe is read)", at);
      format = true;
    }
  }
  if (!format) b.bad("the header has no FORMAT=32-bit_rle_rgbe line");
  const std::size_t resAt = b.p;
  const std::string res = b.until('\n', 128, "resolution line");
  char sy = 0, ay = 0, sx = 0, ax = 0, extra = 0;
  long long n1 = 0, n2 = 0;
  if (std::sscanf(res.c_str(), "%c%c %lld %c%c %lld%c", &sy, &ay, &n1, &sx, &ax, &n2, &extra) != 6 || (sy != '-' && sy != '+') ||
      (sx != '-' && sx != '+') || !((ay == 'Y' && ax == 'X') || (ay == 'X' && ax == 'Y')))
    b.bad("malformed resolution line '" + res + "'", resAt);
  if (!(sy == '-' && ay == 'Y' && sx == '+' && ax == 'X'))
    b.bad("orientation '" + res + "' is not supported (only -Y H +X W: rows top to bottom, columns left to right)", resAt);
  checkSize(b, n2, n1, resAt);
  Image img;
  img.width = (std::size_t)n2; img.height = (std::size_t)n1;
  const std::size_t W = img.width;
  std::vector<std::uint8_t> line(4 * W);
  for (std::size_t y = 0; y < img.height; ++y) {
    const std::size_t rowAt = b.p;
    bool rle = false;
    if (W >= 8 && W <= 32767 && b.left() >= 4 && b.d[b.p] == 2 && b.d[b.p + 1] == 2 && !(b.d[b.p + 2] & 0x80)) {
      if ((((std::size_t)b.d[b.p + 2] << 8) | b.d[b.p + 3]) != W) b.bad("RLE scanline " + std::to_string(y) + " has the wrong length", rowAt);
      rle = true;
      b.p += 4;
    }
    if (rle) {   // adaptive RLE: the four channels one after the other, runs of at most 127
      for (int c = 0; c < 4; ++c) {
        std::size_t x = 0;
        while (x < W) {
          const std::size_t at = b.p;
          std::size_t count = b.byte("RLE scanline");
          if (count > 128) {
            count -= 128;
            if (x + count > W) b.bad("RLE run past the end of scanline " + std::to_string(y), at);
            const std::uint8_t v = b.byte("RLE scanline");
            for (std::size_t i = 0; i < count; ++i) line[4 * (x + i) + c] = v;
          } else {
            if (count == 0) b.bad("empty RLE packet in scanline " + std::to_string(y), at);
            if (x + count > W) b.bad("RLE packet past the end of scanline " + std::to_string(y), at);
            b.need(count, "RLE scanline");
            for (std::size_t i = 0; i < count; ++i) line[4 * (x + i) + c] = b.d[b.p + i];
            b.p += count;
          }
          x += count;
        }
      }
    } else {   // flat: W pixels of four bytes
      b.need(4 * W, "flat scanline");
      std::memcpy(line.data(), &b.d[b.p], 4 * W);
      b.p += 4 * W;
    }
    img.bgr.resize(img.bgr.size() + 3 * W);   // grows with what has really been read: a lying header allocates nothing
    float* out = &img.bgr[3 * W * y];
    for (std::size_t x = 0; x < W; ++x) rgbeToBgr(&line[4 * x], out + 3 * x);
  }
  return img;
}

// ---- PFM
Image readPfm(Bytes& b) {
  auto token = [&](const char* what) {
    while (b.p < b.d.size() && std::isspace(b.d[b.p])) ++b.p;
    const std::size_t start = b.p;
    while (b.p < b.d.size() && !std::isspace(b.d[b.p])) {
      if (b.p - start >= 64) b.bad(std::string("over-long ") + what, start);
      ++b.p;
    }
    if (b.p >= b.d.size()) b.bad(std::string("truncated ") + what, start);   // a token ends with white space
    return std::string(reinterpret_cast<const char*>(&b.d[start]), b.p - start);
  };
  const std::string magic = token("signature");
  if (magic == "Pf") b.bad("a one-channel PFM ('Pf') is not an environment map: three channels ('PF') are needed", 0);
  if (magic != "PF") b.bad("not a PFM file (the signature must be PF)", 0);
  const std::size_t sizeAt = b.p;
  long long w = 0, h = 0;
  double scale = 0.0;
  try {
    std::size_t used = 0;
    const std::string ws = token("width"); w = std::stoll(ws, &used); if (used != ws.size()) throw std::invalid_argument(ws);
    const std::string hs = token("height"); h = std::stoll(hs, &used); if (used != hs.size()) throw std::invalid_argument(hs);
    const std::string ss = token("scale"); scale = std::stod(ss, &used); if (used != ss.size()) throw std::invalid_argument(ss);
  } catch (const std::logic_error&) {   // invalid_argument, out_of_range
    b.bad("malformed PFM header (expected: PF, width, height, scale)", sizeAt);
  }
  if (!(scale != 0.0) || !std::isfinite(scale)) b.bad("PFM scale must be a non-zero number (its sign gives the byte order)", sizeAt);
  checkSize(b, w, h, sizeAt);
  b.p += 1;   // the single white-space character after the scale
  Image img;
  img.width = (std::size_t)w; img.height = (std::size_t)h;
  const std::size_t W = img.width, H = img.height, rowBytes = 12 * W;
  if (b.left() < rowBytes * H) b.bad("truncated pixel data (" + std::to_string(rowBytes * H) + " bytes expected)");
  img.bgr.resize(3 * W * H);
  const bool little = scale < 0.0;
  for (std::size_t y = 0; y < H; ++y) {
    const std::uint8_t* src = &b.d[b.p + rowBytes * (H - 1 - y)];   // the file's first row is the bottom one
    float* out = &img.bgr[3 * W * y];
    for (std::size_t x = 0; x < W; ++x)
      for (int c = 0; c < 3; ++c) {
        std::uint8_t raw[4];
        std::memcpy(raw, src + 12 * x + 4 * c, 4);
        std::uint32_t bits = little ? ((std::uint32_t)raw[0] | ((std::uint32_t)raw[1] << 8) | ((std::uint32_t)raw[2] << 16) | ((std::uint32_t)raw[3] << 24))
                                    : ((std::uint32_t)raw[3] | ((std::uint32_t)raw[2] << 8) | ((std::uint32_t)raw[1] << 16) | ((std::uint32_t)raw[0] << 24));
        float v;
        std::memcpy(&v, &bits, 4);
        out[3 * x + (2 - c)] = v;   // R, G, B in the file
      }
  }
  return img;
}

// ---- OpenEXR, the subset image_io::writeExr writes (all values little-endian, as on every host this builds for)
Image readExrSubset(Bytes& b) {
  if (b.get<std::uint32_t>("magic number") != 20000630u) b.bad("not an OpenEXR file", 0);
  const std::uint32_t version = b.get<std::uint32_t>("version");
  if ((version & 0xffu) != 2u || (version & ~0xffu) != 0u)
    b.bad("unsupported OpenEXR version word " + std::to_string(version) + " (only plain version-2 scanline files are read)", 4);
  bool haveChannels = false, haveWindow = false, haveCompression = false;
  std::int32_t box[4] = {0, 0, 0, 0};
  for (;;) {
    const std::size_t at = b.p;
    const std::string name = b.until('\0', 255, "attribute name");
    if (name.empty()) break;
    const std::string type = b.until('\0', 255, "attribute type");
    const std::int32_t size = b.get<std::int32_t>("attribute size");
    if (size < 0) b.bad("negative size of attribute '" + name + "'", at);
    b.need((std::size_t)size, "attribute value");
    const std::size_t value = b.p, end = b.p + (std::size_t)size;
    if (name == "channels") {
      std::vector<std::string> found;
      while (b.p < end && b.d[b.p] != 0) {
        const std::size_t cAt = b.p;
        const std::string ch = b.until('\0', 255, "channel name");
        if (b.p + 16 > end) b.bad("truncated channel list", cAt);
        std::int32_t pixelType, xs, ys;
        std::memcpy(&pixelType, &b.d[b.p], 4); std::memcpy(&xs, &b.d[b.p + 8], 4); std::memcpy(&ys, &b.d[b.p + 12], 4);
        b.p += 16;
        if (pixelType != 2) b.bad("channel '" + ch + "' is not FLOAT (only 32-bit float channels are read)", cAt);
        if (xs != 1 || ys != 1) b.bad("channel '" + ch + "' is subsampled", cAt);
        found.push_back(ch);
      }
      if (found != std::vector<std::string>{"B", "G", "R"}) {
        std::string list;
        for (const auto& c : found) list += (list.empty() ? "" : ", ") + c;
        b.bad("channels [" + list + "] are not supported (exactly B, G, R are read)", value);
      }
      haveChannels = true;
    } else if (name == "compression") {
      if (size != 1) b.bad("malformed compression attribute", at);
      if (b.d[value] != 0) b.bad("compression method " + std::to_string((int)b.d[value]) + " is not supported (only uncompressed files are read)", value);
      haveCompression = true;
    } else if (name == "dataWindow") {
      if (size != 16) b.bad("malformed dataWindow attribute", at);
      std::memcpy(box, &b.d[value], 16);
      haveWindow = true;
    } else if (name == "lineOrder") {
      if (size != 1) b.bad("malformed lineOrder attribute", at);
      if (b.d[value] != 0) b.bad("line order " + std::to_string((int)b.d[value]) + " is not supported (only increasing Y is read)", value);
    }
    b.p = end;
  }
  if (!haveChannels || !haveWindow || !haveCompression) b.bad("the header lacks channels, compression or dataWindow");
  const long long w = (long long)box[2] - box[0] + 1, h = (long long)box[3] - box[1] + 1;
  checkSize(b, w, h, b.p);
  Image img;
  img.width = (std::size_t)w; img.height = (std::size_t)h;
  const std::size_t W = img.width, H = img.height, rowBytes = 12 * W;
  b.need(8 * H, "scanline offset table");
  const std::size_t table = b.p;
  for (std::size_t y = 0; y < H; ++y) {
    std::uint64_t off;
    std::memcpy(&off, &b.d[table + 8 * y], 8);
    if (off > b.d.size() || b.d.size() - off < 8 + rowBytes) b.bad("scanline " + std::to_string(y) + " lies outside the file (truncated?)", table + 8 * y);
    std::int32_t yy, bytes;
    std::memcpy(&yy, &b.d[off], 4); std::memcpy(&bytes, &b.d[off + 4], 4);
    if ((long long)yy != (long long)box[1] + (long long)y || bytes < 0 || (std::size_t)bytes != rowBytes)
      b.bad("scanline " + std::to_string(y) + " has an unexpected header", (std::size_t)off);
    img.bgr.resize(img.bgr.size() + 3 * W);
    float* out = &img.bgr[3 * W * y];
    const std::uint8_t* row = &b.d[off + 8];
    for (int c = 0; c < 3; ++c)   // planes in alphabetical order B, G, R
      for (std::size_t x = 0; x < W; ++x) std::memcpy(&out[3 * x + c], row + 4 * ((std::size_t)c * W + x), 4);
  }
  return img;
}

}  // namespace

Image read(const std::string& fileName) {
  std::string ext;
  const auto dot = fileName.find_last_of("./\\");
  if (dot != std::string::npos && fileName[dot] == '.') ext = fileName.substr(dot);
  std::transform(ext.begin(), ext.end(), ext.begin(), [](unsigned char c) { return (char)std::tolower(c); });
  const bool hdr = ext == ".hdr" || ext == ".pic", pfm = ext == ".pfm", exr = ext == ".exr";
  if (!hdr && !pfm && !exr)
    throw std::runtime_error("'" + fileName + "': unknown environment-map format (read: .hdr / .pic Radiance RGBE, .pfm, .exr)");
  Bytes b;
  b.file = fileName;
  std::ifstream f(fileName, std::ios::binary);
  if (!f) throw std::runtime_error("'" + fileName + "': could not open the file");
  b.d.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  Image img = hdr ? readHdr(b) : pfm ? readPfm(b) : readExrSubset(b);
  if (img.bgr.size() != 3 * img.width * img.height) b.bad("internal: decoded size mismatch");
  return img;
}

}  // namespace env_map
