// ptmi_probe.h -- the one path of the query entry points (pt_nif_infer, pt_env_map_lookup, pt_trace_paths and the hooks of the
// guides and the meshes): n caller items go up into the scratch buffer, one small kernel runs over them, the answers come back.
// Part of the one translation unit ptmi.hip; included there after ptmi_context.h.
#pragma once

#include <tuple>
#include <type_traits>

namespace {

// One array of the caller's: `per_item` elements of T for each of the call's n items, or (once) that many for the whole call.
// in(p, k) travels to the device before the launch, out(p, k) back after it; `dev` is the span's place in the scratch buffer, as
// the kernel's own type of the same layout where that has another name (out_as).
template <class T, bool kOut, class Dev = T>
struct ProbeSpan {
  static_assert(sizeof(Dev) == sizeof(T), "a span's device type has the layout of the caller's");
  std::conditional_t<kOut, T*, const T*> host;
  size_t per_item;
  bool once;
  std::conditional_t<kOut, Dev*, const Dev*> dev;
  size_t bytes(size_t n) const { return (once ? 1 : n) * per_item * sizeof(T); }
  size_t room(size_t n) const { return (bytes(n) + 15) / 16 * 16; }
  int copy(pt_handle h, size_t n, bool down) const {
    if constexpr (kOut) { if (down) PT_HIP(hipMemcpyAsync(host, dev, bytes(n), hipMemcpyDeviceToHost, h->stream)); }
    else { if (!down) PT_HIP(hipMemcpyAsync(const_cast<Dev*>(dev), host, bytes(n), hipMemcpyHostToDevice, h->stream)); }
    return PT_OK;
  }
};
template <class T> ProbeSpan<T, false> in(const T* p, size_t per_item = 1) { return {p, per_item, false, nullptr}; }
template <class T> ProbeSpan<T, false> in_once(const T* p, size_t count = 1) { return {p, count, true, nullptr}; }
template <class T> ProbeSpan<T, true> out(T* p, size_t per_item = 1) { return {p, per_item, false, nullptr}; }
template <class Dev, class T> ProbeSpan<T, true, Dev> out_as(T* p, size_t per_item = 1) { return {p, per_item, false, nullptr}; }

// What a probe accepts: fewer than `n` items, and its words for more.
struct ProbeLimit { size_t n; const char* too_many; };
constexpr ProbeLimit kNoProbeLimit{SIZE_MAX, ""};

// The grid of the probes' kernels: a thread per item, 256 to a workgroup.
constexpr unsigned kProbeBlock = 256;
inline dim3 probe_grid(size_t n) { return dim3(((uint32_t)n + kProbeBlock - 1) / kProbeBlock); }

// n caller items through one kernel.  The head every probe shares: no item is no work, a null array and a count at or over the
// limit are refused.  Then the device is made current, the spans are packed into the scratch buffer at 16-byte boundaries, the
// inputs go up on the stream, `launch` -- it takes the spans' device pointers, typed and in order, and returns a status -- queues
// the kernel, the outputs come down, and the host waits once.
// Whatever fails, no copy from or to the caller's arrays is left pending when the call returns.
template <class... S, class Launch>
int probe(pt_handle h, size_t n, ProbeLimit limit, std::tuple<S...> spans, Launch launch) {
  if (n == 0) return PT_OK;
  if (std::apply([](const auto&... s) { return (... || !s.host); }, spans)) return fail(h, PT_ERR_INVALID_ARGUMENT, "null buffer");
  if (n >= limit.n) return fail(h, PT_ERR_INVALID_ARGUMENT, limit.too_many);
  PT_HIP(hipSetDevice(h->cfg.device));
  auto run = [&]() -> int {
    if (int rc = ensure_scratch(h, std::apply([n](const auto&... s) { return (size_t{0} + ... + s.room(n)); }, spans))) return rc;
    char* p = h->d_scratch;
    std::apply([&](auto&... s) { ((s.dev = reinterpret_cast<decltype(s.dev)>(p), p += s.room(n)), ...); }, spans);
    int rc = PT_OK;
    if (std::apply([&](const auto&... s) { return (... || (rc = s.copy(h, n, false))); }, spans)) return rc;
    if ((rc = std::apply([&](const auto&... s) { return launch(s.dev...); }, spans))) return rc;
    PT_HIP(hipGetLastError());
    if (std::apply([&](const auto&... s) { return (... || (rc = s.copy(h, n, true))); }, spans)) return rc;
    PT_HIP(hipStreamSynchronize(h->stream));
    return PT_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  return rc;
}

}  // namespace
