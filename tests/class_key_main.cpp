// The key and the sizing rule of the NIF stage's class level (ipu_path_trace_amd/csrc/ptmi_share_plan.h) on the CPU:
// tests/test_class_key.py builds this twice and runs it -- plain (-O2, `--full`: every float of [0, 2]) and with
// -fsanitize=address,undefined (the boundaries and every 257th float).
//
// The NIF kernels read a coordinate as x = (coord - 1) * 2 and then only a_j = (float)(_Float16)(x * 2^j), j < 16.  The
// property: equal class_coord implies equal a_j for all j, as bits.  A class in range is named by the bits of (float)half(x),
// so it is enough that every x gives the a_j of its class's name and that the name is its own class; out of range the class
// is the bits of x itself.  The host compiler has no _Float16: the kernels' conversion is F16C's (round to nearest even) where
// the CPU has it, else the bit-exact software conversion below, which F16C pins on every value it is used on.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include <immintrin.h>

#include "ptmi_share_plan.h"

using namespace ptshare;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

// binary32 -> binary16 -> binary32, round to nearest even, the whole range (subnormal halves, overflow to infinity, NaN quieted)
static float soft_half(float f) {
  const uint32_t b = bits(f), sign = b & 0x80000000u, mag = b & 0x7fffffffu;
  if (mag > 0x7f800000u) return from_bits((b | 0x00400000u) & ~0x1fffu);
  if (mag >= 0x477ff000u) return from_bits(sign | 0x7f800000u);   // >= 65520 rounds to infinity
  if (mag < 0x38800000u) {                                        // below 2^-14: a multiple of 2^-24
    const float scaled = std::fabs(f) * 16777216.0f;              // exact
    const float r = std::nearbyintf(scaled);                      // to nearest even (default rounding mode)
    return from_bits(sign | bits(r * (1.0f / 16777216.0f)));
  }
  return from_bits((b + 0xfffu + ((b >> 13) & 1u)) & ~0x1fffu);
}

static bool g_f16c = false;
__attribute__((target("f16c"))) static float hw_half(float f) {
  return _mm_cvtss_f32(_mm_cvtph_ps(_mm_cvtps_ph(_mm_set_ss(f), _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC)));
}
static float to_half(float f) {
  const float s = soft_half(f);
  if (g_f16c && !std::isnan(f)) CHECK(bits(hw_half(f)) == bits(s));
  return s;
}

// a_j of the kernels, all sixteen, as bits
static void features(float x, uint32_t a[16]) {
  float scale = 1.0f;
  for (int j = 0; j < 16; ++j, scale *= 2.0f) a[j] = bits(to_half(x * scale));
}

static bool in_range(float x) {
  const float m = std::fabs(x);
  return m >= 0x1p-14f && m <= 2.0f;   // false for NaN
}

// one x: the class's name, and that x computes what its class's name computes
static void check_x(float x) {
  const uint32_t c = class_x(x);
  if (!in_range(x)) { CHECK(c == bits(x)); return; }
  const float name = from_bits(c);
  CHECK(c == bits(to_half(x)));            // the device expression (float)(_Float16)x
  CHECK(in_range(name) && class_x(name) == c && (c & 0x1fffu) == 0);   // a class of its own, and apart from every out-of-range key
  uint32_t ax[16], an[16];
  features(x, ax);
  features(name, an);
  for (int j = 0; j < 16; ++j) CHECK(ax[j] == an[j]);
}
static void check_coord(float coord) {
  const float x = (coord - 1.0f) * 2.0f;
  CHECK(class_coord(coord) == class_x(x));
  check_x(x);
}

// eight coordinates at a time with F16C: the same checks as check_coord for coordinates whose x is in range
__attribute__((target("avx2,f16c"))) static uint64_t sweep_avx(uint32_t first, uint32_t last, uint32_t stride) {
  uint64_t bad = 0;
  const __m256 one = _mm256_set1_ps(1.0f), two = _mm256_set1_ps(2.0f);
  for (uint64_t b0 = first; b0 <= last; b0 += 8ull * stride) {
    alignas(32) uint32_t cb[8];
    for (int i = 0; i < 8; ++i) { const uint64_t b = b0 + (uint64_t)i * stride; cb[i] = b <= last ? (uint32_t)b : last; }
    const __m256 coord = _mm256_castsi256_ps(_mm256_load_si256((const __m256i*)cb));
    const __m256 x = _mm256_mul_ps(_mm256_sub_ps(coord, one), two);
    const __m256 name = _mm256_cvtph_ps(_mm256_cvtps_ph(x, _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC));
    alignas(32) float xs[8], ns[8];
    _mm256_store_ps(xs, x); _mm256_store_ps(ns, name);
    int live = 0;
    for (int i = 0; i < 8; ++i) {
      if (!in_range(xs[i])) { bad += class_x(xs[i]) != bits(xs[i]); continue; }
      live |= 1 << i;
      bad += class_coord(from_bits(cb[i])) != bits(ns[i]);
    }
    __m256 sx = x, sn = name;
    int diff = 0;
    for (int j = 0; j < 16; ++j) {
      const __m128i hx = _mm256_cvtps_ph(sx, _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC);
      const __m128i hn = _mm256_cvtps_ph(sn, _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC);
      const int eq = _mm_movemask_epi8(_mm_cmpeq_epi16(hx, hn));   // two bits per half
      for (int i = 0; i < 8; ++i) diff |= ((eq >> (2 * i)) & 3) == 3 ? 0 : 1 << i;
      sx = _mm256_mul_ps(sx, two); sn = _mm256_mul_ps(sn, two);
    }
    bad += (uint64_t)__builtin_popcount(diff & live);
  }
  return bad;
}

static void sweep(uint32_t stride) {
  const uint32_t first = bits(0.0f), last = bits(2.0f);
  const unsigned hw = std::thread::hardware_concurrency();
  const unsigned T = hw == 0 ? 1 : hw > 8 ? 8 : hw;
  std::atomic<uint64_t> bad{0};
  std::vector<std::thread> pool;
  const uint64_t n = ((uint64_t)last - first) / stride + 1, per = (n + T - 1) / T;
  for (unsigned t = 0; t < T; ++t)
    pool.emplace_back([=, &bad] {
      const uint64_t i0 = (uint64_t)t * per, i1 = std::min<uint64_t>(n, i0 + per);
      if (i0 >= i1) return;
      const uint32_t a = (uint32_t)(first + i0 * stride), z = (uint32_t)(first + (i1 - 1) * stride);
      if (g_f16c && __builtin_cpu_supports("avx2")) bad += sweep_avx(a, z, stride);
      else for (uint64_t b = a; b <= z; b += stride) check_coord(from_bits((uint32_t)b));
    });
  for (auto& th : pool) th.join();
  CHECK(bad.load() == 0);
  std::printf("swept %llu coordinates of [0, 2] (stride %u, %u threads, %s)\n", (unsigned long long)n, stride, T,
              g_f16c ? "F16C" : "software half");
}

static bool pow2(uint64_t x) { return x && !(x & (x - 1)); }

static void sizing() {
  const uint64_t counts[] = {0, 1, 2, 511, 512, 513, 1024, 1025, 55296, 84000000ull, 331200000ull, kClassSpace - 1, kClassSpace,
                             kClassSpace + 1, (1ull << 29) - 1, 1ull << 29, 1ull << 30, (1ull << 31) - 1};
  uint64_t prev = 0;
  for (uint64_t e : counts) {
    const uint64_t w = class_slots(e, kFreeUnknown);
    CHECK(pow2(w) && w >= kMinSlots && w <= kClassMaxSlots && w >= prev);
    CHECK(w >= 2 * e || w == kClassMaxSlots);
    prev = w;
    uint64_t prev_m = 0;
    for (uint64_t free_b : {0ull, 1ull, 4096ull, 1ull << 20, 1ull << 30, 16ull << 30, 288ull << 30, ~0ull - 1}) {
      const uint64_t m = class_slots(e, free_b);
      CHECK(pow2(m) && m >= kMinSlots && m <= w && m >= prev_m);
      CHECK(m == kMinSlots || m * kSlotBytes <= free_b / kTableMemoryDivisor);
      prev_m = m;
    }
  }
  // slot indices fit an owner word, and the whole class space of [0, 1]^2 fills the largest table to a half (and 0.0001)
  CHECK(kClassMaxSlots <= kMaxSlots && kClassMaxSlots - 1 <= kOwnerSlotBits);
  CHECK(kClassSpace * 10000 <= kClassMaxSlots * 5001);
  // class_fits: nothing to run over; the class store must be indexable; held buffers cost nothing; a quarter of the memory
  const ClassHeld none;
  CHECK(!class_fits(1024, 0, 1000, none, 1ull << 40) && !class_fits(1024, 1, 0, none, 1ull << 40));
  CHECK(!class_fits(kClassMaxSlots * 2, 1, 1000, none, ~0ull - 1));
  CHECK(class_fits(1024, 2, (1ull << 30) - 1, none, ~0ull - 1) && !class_fits(1024, 2, 1ull << 30, none, ~0ull - 1));
  const uint64_t need = class_bytes(2048, 11, 33120000, none);
  CHECK(need == 2048 * kSlotBytes + 11ull * 33120000 * kStoreEntryBytes + 33120000ull * kOwnerEntryBytes);
  CHECK(class_fits(2048, 11, 33120000, none, 4 * need) && !class_fits(2048, 11, 33120000, none, 4 * need - 4));
  CHECK(!class_fits(2048, 11, 33120000, none, kFreeUnknown));
  ClassHeld all;
  all.table_slots = 2048; all.store_regions = 11; all.owner_maps = 1;
  CHECK(class_bytes(2048, 11, 33120000, all) == 0 && class_fits(2048, 11, 33120000, all, 0) && class_fits(2048, 11, 33120000, all, kFreeUnknown));
  all.store_regions = 10;
  CHECK(class_bytes(2048, 11, 33120000, all) == 11ull * 33120000 * kStoreEntryBytes);
}

int main(int argc, char** argv) {
  const bool full = argc > 1 && !std::strcmp(argv[1], "--full");
  g_f16c = __builtin_cpu_supports("f16c");

  // every half rounding boundary of the range, both signs: the midpoint between two neighbouring halves, +- 4 ulps
  for (uint32_t h = 0x38800000u; h < 0x40000000u; h += 0x2000u)
    for (int d = -4; d <= 4; ++d)
      for (uint32_t sign : {0u, 0x80000000u}) {
        check_x(from_bits(sign | (h + 0x1000u + (uint32_t)d)));
        check_x(from_bits(sign | (h + (uint32_t)d)));   // (and around the half itself; below 2^-14 at the first: out of range)
      }
  // neighbours on either side of a boundary are different classes, a tie goes to the even half
  CHECK(class_x(from_bits(0x3f800fffu)) == 0x3f800000u && class_x(from_bits(0x3f801001u)) == 0x3f802000u);
  CHECK(class_x(from_bits(0x3f801000u)) == 0x3f800000u && class_x(from_bits(0x3f803000u)) == 0x3f804000u);
  // the ends of the range and what lies outside: -2, +-0, +-2^-14 and its neighbours, subnormal x, |x| > 2, infinities, NaN
  for (uint32_t sign : {0u, 0x80000000u}) {
    for (uint32_t m : {0u, 1u, 0x007fffffu, 0x00800000u, 0x387fffffu, 0x38800000u, 0x38800001u, 0x38800fffu, 0x38801000u, 0x38801001u,
                       0x33800000u, 0x3fffffffu, 0x40000000u, 0x40000001u, 0x40001000u, 0x477fe000u, 0x477ff000u, 0x7f7fffffu, 0x7f800000u,
                       0x7fc00000u, 0x7f800001u, 0x7fffffffu})
      check_x(from_bits(sign | m));
    CHECK(class_x(from_bits(sign | 0x40000000u)) == (sign | 0x40000000u));
    CHECK(class_x(from_bits(sign | 0x387fffffu)) == (sign | 0x387fffffu));   // just below 2^-14: its own bits
    CHECK(class_x(from_bits(sign)) == sign);                                // +0 and -0 stay apart
  }
  // coordinates: 0 (x = -2; at E = 16 its last features overflow to infinity), 1 (x = 0), around 1, above 1, below 0, above 2, NaN
  for (float c : {0.0f, 1.0f, 2.0f, 0.5f, 1.5f, 0.25f, 0.999999f, 1.000001f, -0.0f, -0.25f, -3.0f, 2.5f, 1e30f, -1e30f, 1e-30f})
    for (int d = -4; d <= 4; ++d) check_coord(from_bits(bits(c) + (uint32_t)d));
  check_coord(std::nanf(""));
  check_coord(from_bits(0xffffffffu));   // the tables' empty marker, per coordinate
  CHECK(class_key(0.25f, 0.75f) == (((uint64_t)class_coord(0.25f) << 32) | class_coord(0.75f)));
  uint32_t a0[16];
  features(-2.0f, a0);
  CHECK(a0[15] == 0xff800000u && a0[14] == bits(-32768.0f));   // -2 x 2^15 = -65536 is past the largest half

  sweep(full ? 1u : 257u);
  sizing();
  std::printf("CLASS_KEY_OK\n");
  return 0;
}
