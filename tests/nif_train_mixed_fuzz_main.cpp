// Test infrastructure (not product): the validation of pt_nif_train_precision (csrc/ptmi_nif_train_check.h, check_precision)
// and the train_command the metadata writer records for a precision (host/NifTrainWriter.hpp), driven with the defaults, every
// boundary and seeded garbage.  Built with -fsanitize=address,undefined by tests/test_nif_train_mixed_abi.py: anything out of
// bounds or undefined aborts the process with a non-zero status.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "NifTrainWriter.hpp"
#include "ptmi_nif_train_check.h"

static std::uint64_t state = 0x9e3779b97f4a7c15ull;
static std::uint32_t next() {   // xorshift64*: seeded, the same run every time
  state ^= state >> 12; state ^= state << 25; state ^= state >> 27;
  return (std::uint32_t)((state * 0x2545f4914f6cdd1dull) >> 32);
}

int main() {
  int accepted = 0, rejected = 0, unnamed = 0;
  const pt_nif_train_precision d = ptniftrain::default_precision();
  if (!ptniftrain::check_precision(&d).empty() || ptniftrain::check_precision(nullptr).empty()) return 3;
  if (d.mode != PT_NIF_TRAIN_F32 || d.loss_scale != 65536.0f || d.dynamic != 1 || d.growth_interval != 2000u) return 3;
  struct Case { const char* field; pt_nif_train_precision p; bool ok; };
  std::vector<Case> cases;
  auto with = [&](const char* field, auto set, bool ok) { Case c{field, d, ok}; set(c.p); cases.push_back(c); };
  for (std::int32_t v : {-1, 0, 1, 2, INT32_MIN, INT32_MAX}) with("mode", [v](pt_nif_train_precision& p) { p.mode = v; }, v == 0 || v == 1);
  const float inf = 1.0f / 0.0f, nan = inf - inf;
  for (float v : {nan, inf, -inf, 0.f, -1.f, -65536.f, 0.5f, 1.f, 2.f, 3.f, 1000.f, 1024.f, 65536.f, 65537.f, 1073741824.f, 2147483648.f, 1e-45f, 3.4e38f})
    with("loss_scale", [v](pt_nif_train_precision& p) { p.loss_scale = v; }, v == 1.f || v == 2.f || v == 1024.f || v == 65536.f || v == 1073741824.f);
  for (std::int32_t v : {-1, 0, 1, 2, INT32_MIN}) with("dynamic", [v](pt_nif_train_precision& p) { p.dynamic = v; }, v == 0 || v == 1);
  for (std::uint32_t v : {0u, 1u, 2000u, 0x80000000u, 0x80000001u, 0xffffffffu})
    with("growth_interval", [v](pt_nif_train_precision& p) { p.growth_interval = v; }, v >= 1u && v <= 0x80000000u);
  with("struct_size", [](pt_nif_train_precision& p) { p.struct_size -= 4; }, false);
  with("struct_size", [](pt_nif_train_precision& p) { p.struct_size = 0; }, false);
  for (const Case& c : cases) {
    const std::string msg = ptniftrain::check_precision(&c.p);
    if (msg.empty() != c.ok) { std::printf("wrong verdict for %s: '%s'\n", c.field, msg.c_str()); return 4; }
    if (!c.ok && msg.find(c.field) == std::string::npos) { unnamed += 1; std::printf("unnamed: %s: %s\n", c.field, msg.c_str()); }
  }
  // field order: with every field wrong, the first one in the struct is named
  {
    pt_nif_train_precision p = d;
    p.mode = 7; p.loss_scale = 3.f; p.dynamic = 5; p.growth_interval = 0;
    if (ptniftrain::check_precision(&p).find("mode") == std::string::npos) return 5;
    p.mode = 1;
    if (ptniftrain::check_precision(&p).find("loss_scale") == std::string::npos) return 5;
    p.loss_scale = 2.f;
    if (ptniftrain::check_precision(&p).find("dynamic") == std::string::npos) return 5;
    p.dynamic = 0;
    if (ptniftrain::check_precision(&p).find("growth_interval") == std::string::npos) return 5;
  }
  // seeded garbage: whatever the bytes are, a verdict; an accepted set is inside every documented range
  for (int i = 0; i < 20000; ++i) {
    pt_nif_train_precision p = d;
    unsigned char* raw = reinterpret_cast<unsigned char*>(&p);
    const int edits = 1 + (int)(next() % 4);
    for (int e = 0; e < edits; ++e) raw[4 + next() % (sizeof(p) - 4)] = (unsigned char)next();
    if (!ptniftrain::check_precision(&p).empty()) { rejected += 1; continue; }
    accepted += 1;
    int exponent = 0;
    if ((p.mode != 0 && p.mode != 1) || (p.dynamic != 0 && p.dynamic != 1) || p.growth_interval < 1u || p.growth_interval > 0x80000000u) return 6;
    if (!(p.loss_scale >= 1.f && p.loss_scale <= 1073741824.f) || std::frexp(p.loss_scale, &exponent) != 0.5f) return 6;
  }
  // the recorded command names a precision other than the default, and nothing else moves
  nif_train::MetaData m;
  m.name = "map.hdr"; m.embeddingDimension = 12; m.hiddenSize = 320; m.layerCount = 6;
  const std::string plain = nif_train::metadataText(m);
  m.precision = "mixed";
  const std::string mixed = nif_train::metadataText(m);
  if (plain.find("--train-precision") != std::string::npos || mixed.find("\"--train-precision\", \"mixed\"]") == std::string::npos) return 7;
  m.precision = std::string(3000, '"');
  if (nif_train::metadataText(m).size() < 6000) return 7;
  std::printf("cases %zu accepted %d rejected %d unnamed %d\n", cases.size(), accepted, rejected, unnamed);
  return 0;
}
