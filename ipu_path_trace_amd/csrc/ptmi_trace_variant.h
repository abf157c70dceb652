// ptmi_trace_variant.h -- which instance of the trace, trace-paths and feature kernels runs (pt_trace.h, pt_features.h): the three
// coordinates of an instance, the template flags and the occupancy pin they imply, and the one function that picks the
// coordinates from the state of a handle.  Plain C++ (nothing from HIP), so that tests/trace_variant_main.cpp checks the choice
// exhaustively on a CPU; pt_trace.h includes it for the kernels, ptmi.hip and ptmi_denoise.h for the launches.
//
// To add a level or a kind: one enumerator, one line in the flag functions, one rung in select, one in the test's ladder.
#pragma once

namespace ptvariant {

enum class Camera : int { BUILTIN = 0, POSE = 1, LENS = 2 };   // the values of CAM_BUILTIN, CAM_POSE, CAM_LENS (pt_trace.h)
enum class Bounce : int { PLAIN, ENV_GUIDE, LIGHT_GUIDE, LIGHT_GUIDE_PLAMPS };   // the diffuse bounce: cosine, pt_set_env_guide, pt_set_light_guide, ... with polygon lamps
enum class Geometry : int { SPHERES, POLY, MESH, SMOOTH, TEX };   // each level carries the code of the ones below it
constexpr int kCameras = 3, kBounces = 4, kGeometries = 5;

// The flags trace_body, trace_paths_body and features_body take.  The emitter-guided bounce handles an environment guide too,
// by a wave-uniform test at run time, so GUIDE is the environment guide alone.
constexpr bool guide(Bounce b) { return b == Bounce::ENV_GUIDE; }
constexpr bool lights(Bounce b) { return b >= Bounce::LIGHT_GUIDE; }
constexpr bool plamps(Bounce b) { return b == Bounce::LIGHT_GUIDE_PLAMPS; }
constexpr bool poly(Geometry g) { return g >= Geometry::POLY; }
constexpr bool mesh(Geometry g) { return g >= Geometry::MESH; }
constexpr bool smooth(Geometry g) { return g >= Geometry::SMOOTH; }
constexpr bool tex(Geometry g) { return g == Geometry::TEX; }

// amdgpu_waves_per_eu of a trace kernel instance, 0: left to the allocator (the reasons stand at trace_kernel, pt_trace.h)
constexpr int waves_per_eu(Bounce b, Geometry g) { return lights(b) ? 6 : (b == Bounce::PLAIN && g == Geometry::SMOOTH) ? 5 : 0; }

// A polygon lamp is a row of a scene with polygons: the spheres-and-discs level has no such instance.
constexpr bool valid(Bounce b, Geometry g) { return !(plamps(b) && !poly(g)); }

// The same under the names of the bodies' template parameters, for a kernel template to pass on by name.
template <Bounce B, Geometry G> struct Flags {
  static_assert(valid(B, G), "not an instance of the product");
  static constexpr bool GUIDE = guide(B), LIGHTS = lights(B), PLAMPS = plamps(B), POLY = poly(G), MESH = mesh(G), SMOOTH = smooth(G), TEX = tex(G);
  static constexpr int WAVES = waves_per_eu(B, G);
};

struct Variant {
  Camera camera;
  Bounce bounce;
  Geometry geometry;
};
constexpr bool operator==(const Variant& a, const Variant& b) { return a.camera == b.camera && a.bounce == b.bounce && a.geometry == b.geometry; }

// What the choice reads of a handle and of the launch parameters filled from it.
struct State {
  bool lens;             // P.lens_a > 0
  bool posed;            // P.cam_pose
  bool guide_set;        // pt_set_env_guide
  bool lights;           // P.lights.n != 0: an active light guide
  bool light_polygons;   // its table lists a polygon lamp
  bool scene;            // scene_n != 0: a runtime scene is in force
  bool scene_poly, scene_mesh, mesh_smooth, mesh_textured;   // of that scene; they mean nothing without one
};

// The lens wins over a pose, the emitter guide over the environment guide, a mesh over polygons, textured over smooth.
// trace_paths ignores the camera, the feature kernels the camera and the bounce.
constexpr Variant select(const State& s) {
  const bool m = s.scene && s.scene_mesh;
  const Geometry g = m && s.mesh_textured ? Geometry::TEX : m && s.mesh_smooth ? Geometry::SMOOTH : m ? Geometry::MESH
                   : s.scene && s.scene_poly ? Geometry::POLY : Geometry::SPHERES;
  const Bounce b = s.lights ? (s.light_polygons && poly(g) ? Bounce::LIGHT_GUIDE_PLAMPS : Bounce::LIGHT_GUIDE)
                 : s.guide_set ? Bounce::ENV_GUIDE : Bounce::PLAIN;
  return {s.lens ? Camera::LENS : s.posed ? Camera::POSE : Camera::BUILTIN, b, g};
}

// Dense numbering of the valid variants, geometry major and camera minor, so that the TEX instances -- the ones with a second
// kernel argument, in tables of their own -- come last in every family.  Trace kernels: index; trace-paths kernels: index / 3
// (kPathsInstances pairs of bounce and geometry); feature kernels: the geometry.
constexpr int kTraceInstances = kCameras * (kGeometries * kBounces - 1), kPathsInstances = kTraceInstances / kCameras, kFeatureInstances = kGeometries;
constexpr int kTraceTexFirst = kTraceInstances - kCameras * kBounces, kPathsTexFirst = kTraceTexFirst / kCameras, kFeatureTexFirst = kGeometries - 1;
constexpr int paths_index(Bounce b, Geometry g) { return (int)g * kBounces + (int)b - (g > Geometry::SPHERES ? 1 : 0); }   // the one hole: (LIGHT_GUIDE_PLAMPS, SPHERES)
constexpr int index(const Variant& v) { return paths_index(v.bounce, v.geometry) * kCameras + (int)v.camera; }
constexpr Variant at(int i) {
  const int pair = i / kCameras + (i / kCameras >= kBounces - 1 ? 1 : 0);
  return {(Camera)(i % kCameras), (Bounce)(pair % kBounces), (Geometry)(pair / kBounces)};
}

constexpr bool numbering_round_trips() {
  int n = 0;
  for (int g = 0; g < kGeometries; ++g)
    for (int b = 0; b < kBounces; ++b)
      for (int c = 0; c < kCameras; ++c) {
        const Variant v = {(Camera)c, (Bounce)b, (Geometry)g};
        if (!valid(v.bounce, v.geometry)) continue;
        if (index(v) != n || !(at(n) == v) || (index(v) >= kTraceTexFirst) != tex(v.geometry)) return false;
        ++n;
      }
  for (int i = 0; i < kTraceInstances; ++i)
    if (index(at(i)) != i || !valid(at(i).bounce, at(i).geometry)) return false;
  return n == kTraceInstances;
}
static_assert(numbering_round_trips(), "index and at are inverse over the valid variants, in order, the TEX ones last");
static_assert(kTraceInstances == 57 && kPathsInstances == 19 && kFeatureInstances == 5, "the three families");
static_assert(kTraceTexFirst == 45 && kPathsTexFirst == 15 && kFeatureTexFirst == 4, "twelve, four and one TEX instances");

}  // namespace ptvariant
