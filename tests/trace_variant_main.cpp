// tests/trace_variant_main.cpp -- ptvariant::select, the derived flags, the occupancy pin and the dense numbering
// (ipu_path_trace_amd/csrc/ptmi_trace_variant.h) against the three ladders of hand-written kernel names they replaced, over all
// 2^10 states.  The ladders below are those of stage_trace, pt_trace_paths and ensure_features as they stood before the kernels
// became templates, rung for rung and in their override order; in place of each kernel's name stand the template arguments of
// its trace_body<...>, trace_paths_body<...> or features_body<...> line and its amdgpu_waves_per_eu.  Stand-alone (g++, no HIP);
// tests/test_trace_variant.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer.
#include <cstdio>
#include <cstdlib>

#include "ptmi_trace_variant.h"

using namespace ptvariant;

namespace {

// What a hand-written kernel passed to its body: trace_body<kRefillThreshold, kTraceOpt, CAM, GUIDE, LIGHTS, POLY, PLAMPS, MESH,
// SMOOTH, TEX> and its pin (0: none); trace_paths_body<GUIDE, LIGHTS, POLY, PLAMPS, MESH, SMOOTH, TEX> (cam and waves unused);
// features_body<POLY, MESH, SMOOTH, TEX>.  Defaults are the bodies' own: every flag false.
struct Old {
  int cam;
  bool guide, lights, poly, plamps, mesh, smooth, tex;
  int waves;
  bool takes_tex_params;   // the kernel had the second argument
};
constexpr int CAM_BUILTIN = 0, CAM_POSE = 1, CAM_LENS = 2;
constexpr bool F = false, T = true;

// one rung of stage_trace: P.lens_a > 0.f ? trace_kernel_lens_X : (P.cam_pose ? trace_kernel_pose_X : trace_kernel_X), the three
// differing in CAM alone
Old by_camera(const State& s, bool guide, bool lights, bool poly, bool plamps, bool mesh, bool smooth, bool tex, int waves) {
  return {s.lens ? CAM_LENS : (s.posed ? CAM_POSE : CAM_BUILTIN), guide, lights, poly, plamps, mesh, smooth, tex, waves, tex};
}

Old old_stage_trace(const State& s) {
  Old kernel = by_camera(s, F, F, F, F, F, F, F, 0);                                  // trace_kernel[_pose|_lens]
  if (s.guide_set) kernel = by_camera(s, T, F, F, F, F, F, F, 0);                     // _guide
  if (s.lights) kernel = by_camera(s, F, T, F, F, F, F, F, 6);                        // _lights
  if (s.scene && s.scene_poly) {
    kernel = by_camera(s, F, F, T, F, F, F, F, 0);                                    // _poly
    if (s.guide_set) kernel = by_camera(s, T, F, T, F, F, F, F, 0);                   // _guide_poly
    if (s.lights) kernel = by_camera(s, F, T, T, F, F, F, F, 6);                      // _lights_poly
    if (s.lights && s.light_polygons) kernel = by_camera(s, F, T, T, T, F, F, F, 6);  // _lights_plamps
  }
  if (s.scene && s.scene_mesh) {
    kernel = by_camera(s, F, F, T, F, T, F, F, 0);                                    // _mesh
    if (s.guide_set) kernel = by_camera(s, T, F, T, F, T, F, F, 0);                   // _guide_mesh
    if (s.lights) kernel = by_camera(s, F, T, T, F, T, F, F, 6);                      // _lights_mesh
    if (s.lights && s.light_polygons) kernel = by_camera(s, F, T, T, T, T, F, F, 6);  // _lights_plamps_mesh
  }
  if (s.scene && s.scene_mesh && s.mesh_smooth) {
    kernel = by_camera(s, F, F, T, F, T, T, F, 5);                                    // _smooth
    if (s.guide_set) kernel = by_camera(s, T, F, T, F, T, T, F, 0);                   // _guide_smooth
    if (s.lights) kernel = by_camera(s, F, T, T, F, T, T, F, 6);                      // _lights_smooth
    if (s.lights && s.light_polygons) kernel = by_camera(s, F, T, T, T, T, T, F, 6);  // _lights_plamps_smooth
  }
  if (s.scene && s.scene_mesh && s.mesh_textured) {
    Old tex = by_camera(s, F, F, T, F, T, T, T, 0);                                   // _tex
    if (s.guide_set) tex = by_camera(s, T, F, T, F, T, T, T, 0);                      // _guide_tex
    if (s.lights) tex = by_camera(s, F, T, T, F, T, T, T, 6);                         // _lights_tex
    if (s.lights && s.light_polygons) tex = by_camera(s, F, T, T, T, T, T, T, 6);     // _lights_plamps_tex
    return tex;   // launched with tex_params(h)
  }
  return kernel;
}

Old paths(bool guide, bool lights, bool poly, bool plamps, bool mesh, bool smooth, bool tex) {
  return {0, guide, lights, poly, plamps, mesh, smooth, tex, 0, tex};
}

Old old_trace_paths(const State& s) {
  //                        trace_paths_lights_kernel            trace_paths_guide_kernel               trace_paths_kernel
  Old kernel = s.lights ? paths(F, T, F, F, F, F, F) : (s.guide_set ? paths(T, F, F, F, F, F, F) : paths(F, F, F, F, F, F, F));
  if (s.scene && s.scene_poly)   // _lights_plamps, _lights_poly, _guide_poly, _poly
    kernel = s.lights ? (s.light_polygons ? paths(F, T, T, T, F, F, F) : paths(F, T, T, F, F, F, F))
                      : (s.guide_set ? paths(T, F, T, F, F, F, F) : paths(F, F, T, F, F, F, F));
  if (s.scene && s.scene_mesh)   // _lights_plamps_mesh, _lights_mesh, _guide_mesh, _mesh
    kernel = s.lights ? (s.light_polygons ? paths(F, T, T, T, T, F, F) : paths(F, T, T, F, T, F, F))
                      : (s.guide_set ? paths(T, F, T, F, T, F, F) : paths(F, F, T, F, T, F, F));
  if (s.scene && s.scene_mesh && s.mesh_smooth)   // _lights_plamps_smooth, _lights_smooth, _guide_smooth, _smooth
    kernel = s.lights ? (s.light_polygons ? paths(F, T, T, T, T, T, F) : paths(F, T, T, F, T, T, F))
                      : (s.guide_set ? paths(T, F, T, F, T, T, F) : paths(F, F, T, F, T, T, F));
  if (s.scene && s.scene_mesh && s.mesh_textured)   // _lights_plamps_tex, _lights_tex, _guide_tex, _tex: launched with tex_params(h)
    return s.lights ? (s.light_polygons ? paths(F, T, T, T, T, T, T) : paths(F, T, T, F, T, T, T))
                    : (s.guide_set ? paths(T, F, T, F, T, T, T) : paths(F, F, T, F, T, T, T));
  return kernel;
}

Old features(bool poly, bool mesh, bool smooth, bool tex) { return {0, F, F, poly, F, mesh, smooth, tex, 0, tex}; }

Old old_features(const State& s) {
  Old kernel = s.scene && s.scene_poly ? features(T, F, F, F) : features(F, F, F, F);                // features_kernel_poly : features_kernel
  if (s.scene && s.scene_mesh) kernel = s.mesh_smooth ? features(T, T, T, F) : features(T, T, F, F);   // features_kernel_smooth : features_kernel_mesh
  if (s.scene && s.scene_mesh && s.mesh_textured) return features(T, T, T, T);                         // features_kernel_tex, with tex_params(h)
  return kernel;
}

int failures = 0;
void check(bool ok, const char* what, unsigned state, const char* family) {
  if (ok) return;
  if (++failures <= 20) std::printf("FAIL %s: state 0x%03x, %s\n", family, state, what);
}

// the flags and the pin derived from the variant against the transcribed ones; use_camera / use_bounce: what the family reads
void compare(const Variant& v, const Old& old, bool use_camera, bool use_bounce, unsigned state, const char* family) {
  check(valid(v.bounce, v.geometry), "select returned an invalid variant", state, family);
  if (use_camera) check((int)v.camera == old.cam, "camera", state, family);
  if (use_bounce) {
    check(guide(v.bounce) == old.guide, "GUIDE", state, family);
    check(lights(v.bounce) == old.lights, "LIGHTS", state, family);
    check(plamps(v.bounce) == old.plamps, "PLAMPS", state, family);
  }
  check(poly(v.geometry) == old.poly, "POLY", state, family);
  check(mesh(v.geometry) == old.mesh, "MESH", state, family);
  check(smooth(v.geometry) == old.smooth, "SMOOTH", state, family);
  check(tex(v.geometry) == old.tex, "TEX", state, family);
  check(tex(v.geometry) == old.takes_tex_params, "the second kernel argument", state, family);
  if (use_camera) check(waves_per_eu(v.bounce, v.geometry) == old.waves, "amdgpu_waves_per_eu", state, family);
}

}  // namespace

int main() {
  static_assert((int)Camera::BUILTIN == CAM_BUILTIN && (int)Camera::POSE == CAM_POSE && (int)Camera::LENS == CAM_LENS, "the CAM_* values of pt_trace.h");
  bool reached_trace[kTraceInstances] = {}, reached_paths[kPathsInstances] = {}, reached_features[kFeatureInstances] = {};
  for (unsigned bits = 0; bits < (1u << 10); ++bits) {
    const State s = {(bits & 1u) != 0,  (bits & 2u) != 0,  (bits & 4u) != 0,   (bits & 8u) != 0,   (bits & 16u) != 0,
                     (bits & 32u) != 0, (bits & 64u) != 0, (bits & 128u) != 0, (bits & 256u) != 0, (bits & 512u) != 0};
    const Variant v = select(s);
    compare(v, old_stage_trace(s), true, true, bits, "trace");
    compare(v, old_trace_paths(s), false, true, bits, "trace_paths");
    compare(v, old_features(s), false, false, bits, "features");
    const int i = index(v), p = paths_index(v.bounce, v.geometry), f = (int)v.geometry;
    check(i >= 0 && i < kTraceInstances && at(i) == v, "index / at round trip", bits, "trace");
    check(p >= 0 && p < kPathsInstances && p == i / kCameras && at(p * kCameras).bounce == v.bounce && at(p * kCameras).geometry == v.geometry,
          "paths_index round trip", bits, "trace_paths");
    check((i >= kTraceTexFirst) == tex(v.geometry) && (p >= kPathsTexFirst) == tex(v.geometry) && (f >= kFeatureTexFirst) == tex(v.geometry),
          "the TEX instances lie behind the *TexFirst marks", bits, "all");
    if (i >= 0 && i < kTraceInstances) reached_trace[i] = true;
    if (p >= 0 && p < kPathsInstances) reached_paths[p] = true;
    if (f >= 0 && f < kFeatureInstances) reached_features[f] = true;
  }
  int valid_variants = 0;
  for (int g = 0; g < kGeometries; ++g)
    for (int b = 0; b < kBounces; ++b)
      for (int c = 0; c < kCameras; ++c) {
        const Variant v = {(Camera)c, (Bounce)b, (Geometry)g};
        if (!valid(v.bounce, v.geometry)) continue;
        ++valid_variants;
        check(at(index(v)) == v, "at(index(v)) == v", (unsigned)index(v), "numbering");
      }
  check(valid_variants == kTraceInstances, "57 valid variants", 0, "numbering");
  for (int i = 0; i < kTraceInstances; ++i) {
    check(index(at(i)) == i && valid(at(i).bounce, at(i).geometry), "index(at(i)) == i", (unsigned)i, "numbering");
    check(reached_trace[i], "a trace instance no state selects", (unsigned)i, "trace");
  }
  for (int i = 0; i < kPathsInstances; ++i) check(reached_paths[i], "a trace-paths instance no state selects", (unsigned)i, "trace_paths");
  for (int i = 0; i < kFeatureInstances; ++i) check(reached_features[i], "a feature instance no state selects", (unsigned)i, "features");
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("TRACE_VARIANT_OK %d + %d + %d instances, 1024 states\n", kTraceInstances, kPathsInstances, kFeatureInstances);
  return 0;
}
