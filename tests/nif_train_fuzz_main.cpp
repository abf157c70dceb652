// Test infrastructure (not product): the host-side pieces of the NIF trainer that take outside input -- the parameter
// validation (csrc/ptmi_nif_train_check.h) and the writers of nif_metadata.txt / converted.ptnif (host/NifTrainWriter.hpp) --
// driven with defaults, every boundary, seeded garbage and awkward strings.  Built with -fsanitize=address,undefined by
// tests/test_nif_train_abi.py: anything out of bounds or undefined aborts the process with a non-zero status.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "NifTrainWriter.hpp"
#include "ptmi_nif_train_check.h"

static std::uint64_t state = 0x9e3779b97f4a7c15ull;
static std::uint32_t next() {   // xorshift64*: seeded, the same run every time
  state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
  return (std::uint32_t)((state * 0x2545f4914f6cdd1dull) >> 32);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  int accepted = 0, rejected = 0, unnamed = 0, refused_writes = 0;
  const pt_nif_train_params d = ptniftrain::defaults();
  if (!ptniftrain::check(&d).empty() || ptniftrain::check(nullptr).empty()) return 3;
  // every boundary of every field: inside is accepted, outside is refused with the field's name
  struct Case { const char* field; pt_nif_train_params p; bool ok; };
  std::vector<Case> cases;
  auto with = [&](const char* field, auto set, bool ok) { Case c{field, d, ok}; set(c.p); cases.push_back(c); };
  for (std::uint32_t v : {0u, 1u, 15u, 16u, 17u}) with("embedding_dim", [v](pt_nif_train_params& p) { p.embedding_dim = v; }, v >= 1 && v <= 15);
  for (std::uint32_t v : {0u, 31u, 32u, 48u, 1024u, 1056u, 2048u, 0xffffffe0u}) with("hidden", [v](pt_nif_train_params& p) { p.hidden = v; }, v >= 32 && v <= 1024 && v % 32 == 0);
  for (std::uint32_t v : {0u, 1u, 15u, 16u}) with("layer_count", [v](pt_nif_train_params& p) { p.layer_count = v; }, v >= 1 && v <= 15);
  for (std::uint32_t v : {0u, 100u, 256u, 1u << 20, (1u << 20) + 256u, 0xffffff00u}) with("batch", [v](pt_nif_train_params& p) { p.batch = v; }, v >= 256 && v <= (1u << 20) && v % 256 == 0);
  const float inf = 1.0f / 0.0f, nan = inf - inf;
  for (float v : {nan, inf, -inf, 0.f, -1.f, 1e-3f}) {
    with("learning_rate", [v](pt_nif_train_params& p) { p.learning_rate = v; }, v == 1e-3f);
    with("adam_eps", [v](pt_nif_train_params& p) { p.adam_eps = v; }, v == 1e-3f);
    with("eps", [v](pt_nif_train_params& p) { p.eps = v; }, v == 1e-3f);
  }
  for (float v : {nan, inf, -0.5f, 1.0f, 0.f, 0.5f}) {
    with("beta1", [v](pt_nif_train_params& p) { p.beta1 = v; }, v == 0.f || v == 0.5f);
    with("beta2", [v](pt_nif_train_params& p) { p.beta2 = v; }, v == 0.f || v == 0.5f);
  }
  for (std::int32_t v : {-1, 0, 1, 2}) with("log_tone_map", [v](pt_nif_train_params& p) { p.log_tone_map = v; }, v == 0 || v == 1);
  with("struct_size", [](pt_nif_train_params& p) { p.struct_size -= 4; }, false);
  for (const Case& c : cases) {
    const std::string msg = ptniftrain::check(&c.p);
    if (msg.empty() != c.ok) { std::printf("wrong verdict for %s: '%s'\n", c.field, msg.c_str()); return 4; }
    if (!c.ok && msg.find(c.field) == std::string::npos) { unnamed += 1; std::printf("unnamed: %s: %s\n", c.field, msg.c_str()); }
  }
  // seeded garbage: whatever the bytes are, a verdict and -- for an accepted set -- a well-formed stack
  for (int i = 0; i < 20000; ++i) {
    pt_nif_train_params p = d;
    unsigned char* raw = reinterpret_cast<unsigned char*>(&p);
    const int edits = 1 + (int)(next() % 6);
    for (int e = 0; e < edits; ++e) raw[4 + next() % (sizeof(p) - 4)] = (unsigned char)next();
    if (!ptniftrain::check(&p).empty()) { rejected += 1; continue; }
    accepted += 1;
    const std::vector<ptniftrain::Shape> s = ptniftrain::shapes(p);
    if (s.size() != p.layer_count + 1 || s.front().rows != 4 * p.embedding_dim || s.back().cols != 3) return 5;
    for (std::size_t l = 1; l < s.size(); ++l)
      if (s[l].rows != s[l - 1].cols && s[l].rows != s[l - 1].cols + 4 * p.embedding_dim) return 6;
  }
  // the writers: awkward names, extreme values, and layers whose buffers do not match their shape
  nif_train::MetaData m;
  m.embeddingDimension = 12; m.hiddenSize = 320; m.layerCount = 6; m.imageHeight = 16384; m.imageWidth = 16384;
  m.eps = 1e-8f; m.max = 3.4e38f; m.mean[0] = -1e-38f; m.mean[1] = nan; m.mean[2] = inf;
  for (const std::string& name : {std::string("plain.hdr"), std::string("quo\"te\\back"), std::string("ctl\x01\x1f\n\ttab"), std::string(5000, 'x'), std::string()}) {
    m.name = name;
    nif_train::writeMetadata(dir + "/meta.txt", m);
    std::ifstream f(dir + "/meta.txt", std::ios::binary);
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (text != nif_train::metadataText(m) || text.find("\"train_command\"") == std::string::npos) return 7;
    for (const char c : text)
      if ((unsigned char)c < 0x20 && c != '\n') return 8;   // control characters are escaped
  }
  std::vector<nif_train::HalfLayer> layers;
  for (const ptniftrain::Shape& s : ptniftrain::shapes(d)) {
    nif_train::HalfLayer l;
    l.rows = s.rows; l.cols = s.cols; l.relu = s.relu;
    l.kernel.assign((std::size_t)s.rows * s.cols, (std::uint16_t)next());
    l.bias.assign(s.cols, (std::uint16_t)next());
    layers.push_back(l);
  }
  nif_train::writePtnif(dir + "/w.ptnif", layers, d.embedding_dim);
  std::size_t want = 16;
  for (const auto& l : layers) want += 20 + 2 * (l.kernel.size() + l.bias.size());
  std::ifstream w(dir + "/w.ptnif", std::ios::binary | std::ios::ate);
  if ((std::size_t)w.tellg() != want) return 9;
  for (int bad = 0; bad < 5; ++bad) {
    std::vector<nif_train::HalfLayer> broken = layers;
    if (bad == 0) broken[2].kernel.pop_back();
    if (bad == 1) broken[3].bias.push_back(0);
    if (bad == 2) broken[0].rows = 0;
    if (bad == 3) broken.clear();
    if (bad == 4) broken.resize(17, layers[1]);
    try { nif_train::writePtnif(dir + "/broken.ptnif", broken, d.embedding_dim); return 10; } catch (const std::exception&) { refused_writes += 1; }
  }
  try { nif_train::writePtnif(dir + "/no/such/dir/w.ptnif", layers, d.embedding_dim); return 11; } catch (const std::exception&) { refused_writes += 1; }
  std::printf("cases %zu accepted %d rejected %d unnamed %d refused_writes %d\n", cases.size(), accepted, rejected, unnamed, refused_writes);
  return 0;
}
