#include "PathTracerApp.hpp"
#include "image_io.hpp"

#include <sstream>

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <fstream>
#include <limits>
#include <memory>
#include <stdexcept>
#include <thread>

#include "AsyncTask.hpp"
#include "json.hpp"
#include "logging.hpp"
#include "../csrc/ptmi_scene.h"
#include "../csrc/ptmi_camera.h"
#include "../csrc/ptmi_env_guide.h"
#include "../csrc/ptmi_light_guide.h"
#include "../csrc/ptmi_mesh.h"
#include "ObjReader.hpp"
#include "trace_ranges.hpp"

/// Adjust samples per pixel to be a multiple of samples per step (PathTracerApp.cpp:19-27).
std::size_t roundSamplesPerPixel(std::size_t samplesPerPixel, std::size_t samplesPerIpuStep) {
  if (samplesPerPixel % samplesPerIpuStep) {
    samplesPerPixel += samplesPerIpuStep - (samplesPerPixel % samplesPerIpuStep);
    pt_log::info_("Rounding SPP to next multiple of {}  (Rounded SPP :=  {})", samplesPerIpuStep, samplesPerPixel);
  }
  return samplesPerPixel;
}

namespace {
void check(pt_handle h, int rc, const char* what) {
  if (rc) throw std::runtime_error(std::string(what) + ": " + pt_last_error(h));
}
int aaNoiseType(const std::string& s) {
  if (s == "normal") return PT_AA_NORMAL;
  if (s == "uniform") return PT_AA_UNIFORM;
  if (s == "truncated-normal") return PT_AA_TRUNCATED_NORMAL;
  throw std::runtime_error("Invalid AA noise type: " + s);  // PathTracerApp.cpp:43
}
}  // namespace

PathTracerApp::PathTracerApp() {}

PathTracerApp::~PathTracerApp() {
  for (auto h : devices) pt_destroy(h);
}

std::vector<OptionSpec> PathTracerApp::addToolOptions() {
  return {
      // main.cpp:8-37
      {"help", 0, "", false, true, "Show command help."},
      {"model", 0, "false", false, true, "IPU-only (simulator): accepted and ignored."},
      {"ipus", 0, "1", false, false, "Number of devices to use (MI355X GPUs here)."},
      {"save-exe", 0, "", false, false, "IPU-only (graph cache): accepted and ignored."},
      {"load-exe", 0, "", false, false, "IPU-only (graph cache): accepted and ignored."},
      {"compile-only", 0, "false", false, true, "Validate the options and the NIF assets, then stop without touching a device (the reference compiles its graph and stops)."},
      {"defer-attach", 0, "false", false, true, "IPU-only: accepted and ignored."},
      {"log-level", 0, "info", false, false, "One of 'trace', 'debug', 'info', 'warn', 'err', 'critical', 'off'."},
      // PathTracerApp.cpp:794-830
      {"outfile", 'o', "", true, false, "Set output file name."},
      {"save-interval", 0, "1", false, false, ""},
      {"width", 'w', "256", false, false, "Output image width (total pixels)."},
      {"height", 'h', "256", false, false, "Output image height (total pixels)."},
      {"samples", 's', "512", false, false, "Total samples to take per pixel."},
      {"samples-per-step", 0, "512", false, false, "Samples to take per device step."},
      {"interactive-samples", 0, "8", false, false, "Number of samples to take per step during user interaction."},
      {"refractive-index", 'n', "1.5", false, false, "Refractive index."},
      {"roulette-depth", 0, "3", false, false, "Number of bounces before rays are randomly stopped."},
      {"stop-prob", 0, "0.3", false, false, "Probability of a ray being stopped."},
      {"aa-noise-scale", 'a', "0.3", false, false, "Scale of anti-aliasing noise (pixels)."},
      {"fov", 0, "90", false, false, "Horizontal field of view (degrees)."},
      {"exposure", 0, "0", false, false, "Exposure compensation for tone-mapping."},
      {"gamma", 0, "2.2", false, false, "Gamma correction for tone-mapping."},
      {"env-map-rotation", 0, "0", false, false, "Azimuthal rotation for HDRI environment map (degrees)."},
      {"seed", 0, "1", false, false, "Seed for random number generation."},
      {"aa-noise-type", 0, "normal", false, false, "['uniform', 'normal', 'truncated-normal']."},
      {"codelet-path", 0, "./", false, false, "IPU-only: accepted and ignored."},
      {"enable-load-balancing", 0, "false", false, true, "Run dynamic load balancing algorithm for path tracing."},
      {"max-path-length", 0, "10", false, false, ""},
      {"assets", 0, "", true, false, "Path to the 'assets.extra' directory of the saved keras model."},
      {"partials-type", 0, "half", false, false, "IPU-only: accepted and ignored (MFMA accumulates in fp32)."},
      {"available-memory-proportion", 0, "0.6", false, false, "IPU-only: accepted and ignored."},
      {"max-nif-batch-size", 0, "44160", false, false, "IPU-only: accepted and ignored (the NIF runs on a compacted queue)."},
      {"ui-port", 0, "0", false, false, "Start a remote user-interface server on the specified port (text protocol, see InterfaceServer.hpp)."},
      // additions of this build
      {"synthetic-nif", 0, "false", false, true, "Use seeded stand-in NIF weights when <assets>/converted.ptnif is absent."},
      {"constant-env", 0, "", false, false, "r,g,b: constant-radiance environment instead of the NIF (BASELINE config C1)."},
      {"host-film", 0, "false", false, true, "Run the reference's step loop (worklist to the host every step, host film) even without load balancing."},
      {"devices", 0, "", false, false, "GPU ordinal of every logical device, e.g. 0,1,2,3 (default: 0 .. ipus-1). Several logical devices may share a GPU (0,0): HDR tiles are then gathered through the host."},
      {"host-gather", 0, "false", false, true, "Gather the HDR tiles of the devices through the host (one copy per device) instead of over an RCCL communicator."},
      {"share-nif-evaluations", 0, "off", false, false, "off | batch | step: escaped paths with bit-identical (u, v) share one NIF evaluation within a kernel batch or a whole step (exact: the image is bit-identical to off; the reference evaluates every escaped path)."},
      {"scene", 0, "", false, false, "FILE.json: render the scene of the file instead of the built-in one -- {\"objects\": [...]}, 1..32 objects, each {\"shape\": \"sphere\" | \"disc\", \"centre\": [x, y, z], \"radius\": r, \"normal\": [x, y, z] (disc), \"material\": \"diffuse\" | \"specular\" | \"refractive\" | \"emissive\", \"colour\": [r, g, b] (\"emission\" for an emitter; default 1, 1, 1)}; a \"triangle\" or \"parallelogram\" takes \"vertices\": [[x, y, z], [x, y, z], [x, y, z]] (v0, v1, v2; the parallelogram's fourth corner is v1 + v2 - v0) instead of centre, radius and normal; a \"mesh\" (one object of the table, one material, flat shading unless \"normals\" is given) takes either \"vertices\": [[x, y, z], ...] and \"triangles\": [[a, b, c], ...] (indices from 0) or \"file\": \"x.obj\" (relative to the scene file; v and f lines, faces triangulated as fans), and optionally \"scale\": s or [sx, sy, sz] and \"translate\": [x, y, z], applied in binary32 on the host as v * scale + translate before anything else; \"normals\": \"file\" (the OBJ's vn lines and v//vn or v/vt/vn corners) or \"normals\": [[x, y, z], ...] with an optional \"normal_indices\": [[a, b, c], ...] per triangle (else one normal per vertex) shades the mesh smooth; normals are not scaled, so a non-uniform \"scale\" is refused with them; \"texture\": \"x.hdr|.pfm|.exr\" (relative to the scene file; a LINEAR float image, no 8-bit formats and no sRGB decoding) with \"uvs\": \"file\" (the OBJ's vt lines and v/vt or v/vt/vn corners) or \"uvs\": [[s, t], ...] with an optional \"uv_indices\": [[a, b, c], ...] per triangle (else one per vertex), and optionally \"texture_filter\": \"nearest\" | \"bilinear\" (default) and \"texture_wrap\": \"repeat\" (default) | \"clamp\", multiplies the mesh's colour by the image.  Optional \"camera\": {\"position\": [x, y, z], \"look_at\": [x, y, z], \"up\": [x, y, z], \"lens_radius\": a, \"focus_distance\": F} (defaults: the built-in pinhole at the origin looking down -z; a lens needs a focus distance)."},
      {"env-map", 0, "", false, false, "FILE: an equirectangular HDR image as the environment light instead of the NIF -- Radiance .hdr / .pic (RGBE, orientation -Y H +X W), .pfm or .exr (uncompressed float B, G, R). No NIF is loaded; not together with --constant-env. --env-map-rotation applies as to the NIF."},
      {"env-map-filter", 0, "bilinear", false, false, "nearest | bilinear: how --env-map is looked up between texels."},
      {"env-guide", 0, "", false, false, "FILE | map | env: guide diffuse bounces by the luminance of an equirectangular HDR image (formats of --env-map; 'map' reuses the file of --env-map; 'env' needs no file: the guide is built on the device from the environment in force -- the NIF of --assets, the map or the constant -- and follows a NIF loaded later). Changes how directions are sampled, not the light: the image stays unbiased under any environment, e.g. a NIF guided by the image it was trained from."},
      {"env-guide-size", 0, "", false, false, "RxC: grid of the guide, rows x columns, powers of two, at most 1024x2048 and the image size (default: the largest that fit; 256x512 for 'env')."},
      {"env-guide-supersample", 0, "2", false, false, "S: 1, 2 or 4 lookups of the environment per cell edge of --env-guide env."},
      {"env-guide-alpha", 0, "0.5", false, false, "Probability in [0, 0.9] that a diffuse bounce draws its direction from the guide."},
      {"light-guide-beta", 0, "0", false, false, "Probability in [0, 0.9] that a diffuse bounce draws its direction towards an emitter of the scene (0 = off); with --env-guide, alpha + beta must not exceed 0.9. Changes how directions are sampled, not the light."},
      {"light-guide-polygons", 0, "false", false, true, "With --light-guide-beta > 0: guided bounces also draw from the emissive triangles and parallelograms of --scene, a uniform point of their area (without it an emissive polygon is reached by the hemisphere alone)."},
      {"denoise", 0, "false", false, true, "Also write <basename>_denoised.exr and _denoised.<ext> at every save: the film through the edge-avoiding A-trous filter (pt_denoise), guided by first-hit object id, normal, depth and albedo. The plain outputs are unchanged. One device with the film resident filters the resident film; --host-film, load balancing or several devices filter the host film on device 0."},
      {"denoise-iterations", 0, "5", false, false, "A-trous iterations, 1..6 (steps 1, 2, 4, ...)."},
      {"denoise-sigma-colour", 0, "4", false, false, "Colour stop of the denoiser (halved every iteration); <= 0 disables it."},
      {"denoise-sigma-normal", 0, "0.5", false, false, "Normal stop of the denoiser; <= 0 disables it."},
      {"denoise-sigma-depth", 0, "0.1", false, false, "Relative depth stop of the denoiser; <= 0 disables it."},
      {"save-features", 0, "false", false, true, "Also write the first-hit feature buffers at every save: <basename>_normal.exr (world x, y, z in the B, G, R channels), _albedo.exr (B, G, R) and _depth.exr (the hit distance in all three channels)."},
      {"mesh-builder", 0, "host", false, false, "host | device: who builds the trees of --scene's meshes -- binned SAH on one host thread, or a linear BVH built by kernels (pt_set_mesh_build; faster to build, somewhat slower to trace). The image is bit-identical either way."},
      {"mesh-device-tree", 0, "linear", false, false, "linear | sah: which tree --mesh-builder device builds -- a linear BVH, or the host builder's binned-SAH tree, byte for byte, built by kernels (pt_set_mesh_device_tree; slower to build than the linear tree, traces as the host's). Inert under --mesh-builder host. The image is bit-identical either way."},
      {"nif-memo-gib", 0, "0", false, false, "GiB of device memory for a memo of decoded NIF values kept across steps, per logical device (0 = off). Exact: the image is bit-identical to off. Escaped paths whose (u, v) an earlier step evaluated are served from it; the memo is forgotten when a new NIF is loaded."},
  };
}

// --mesh-builder (an extension: pt_set_mesh_build)
std::int32_t meshBuilderMode(const std::string& name) {
  if (name == "host") return PT_MESH_BUILDER_HOST;
  if (name == "device") return PT_MESH_BUILDER_DEVICE;
  throw std::runtime_error("--mesh-builder must be one of host, device; got '" + name + "'");
}

// --mesh-device-tree (an extension: pt_set_mesh_device_tree)
std::int32_t meshDeviceTreeKind(const std::string& name) {
  if (name == "linear") return PT_MESH_DEVICE_TREE_LINEAR;
  if (name == "sah") return PT_MESH_DEVICE_TREE_SAH;
  throw std::runtime_error("--mesh-device-tree must be one of linear, sah; got '" + name + "'");
}

// --share-nif-evaluations (an extension: the reference evaluates the NIF on every escaped path, PathTracerApp.cpp:147-198)
std::int32_t nifSharingMode(const std::string& name) {
  if (name == "off") return PT_NIF_SHARE_OFF;
  if (name == "batch") return PT_NIF_SHARE_BATCH;
  if (name == "step") return PT_NIF_SHARE_STEP;
  throw std::runtime_error("--share-nif-evaluations must be one of off, batch, step; got '" + name + "'");
}

pt_nif_sharing_stats PathTracerApp::sharingStatsRequest() {
  pt_nif_sharing_stats s{};
  s.struct_size = sizeof(pt_nif_sharing_stats);
  return s;
}

void PathTracerApp::countNifEvaluations(const std::vector<pt_nif_sharing_stats>& share) {
  for (const auto& s : share) { nifEscaped += s.escaped; nifEvaluations += s.evaluations; }
}

// NIF rows executed since the last save interval, against the escaped paths (Samples/sec still counts path-samples)
void PathTracerApp::logNifEvaluations() {
  const double shared = nifEscaped ? 100.0 * (double)(nifEscaped - std::min(nifEscaped, nifEvaluations)) / (double)nifEscaped : 0.0;
  pt_log::info_("NIF evaluations: executed {} of {} escaped ({} % shared)", nifEvaluations, nifEscaped, shared);
  nifEscaped = nifEvaluations = 0;
}

// --env-map-filter
std::int32_t envMapFilter(const std::string& name) {
  if (name == "nearest") return PT_ENV_FILTER_NEAREST;
  if (name == "bilinear") return PT_ENV_FILTER_BILINEAR;
  throw std::runtime_error("--env-map-filter must be one of nearest, bilinear; got '" + name + "'");
}

// --nif-memo-gib (an extension, like sharing): a non-negative number of GiB
std::uint64_t nifMemoBytes(const std::string& text) {
  std::size_t used = 0;
  double gib = -1.0;
  try { gib = std::stod(text, &used); } catch (const std::exception&) { used = 0; }
  if (text.empty() || used != text.size() || !(gib >= 0.0) || gib > 1e6)
    throw std::runtime_error("--nif-memo-gib must be a non-negative number of GiB; got '" + text + "'");
  return (std::uint64_t)(gib * (double)(1ull << 30));
}

// --scene (an extension: the reference's scene is compile-time, codelets.cpp:90,110-144).  Read and checked before any device is
// attached, with the library's own checks (ptmi_scene.h) and messages; the table goes to every handle in attach().
// `camera` receives the file's optional top-level "camera" (every key optional, defaults of pt_camera), checked like the table.
// A "triangle" or "parallelogram" takes "vertices": [[..], [..], [..]] instead of centre / radius / normal; a file that holds one is
// checked as pt_set_scene_ex checks it and leaves its table in `ex` (empty otherwise: the file goes through pt_set_scene as ever).
// A "mesh" also takes "normals" -- "file" (the OBJ's vn lines and corner indices) or an inline array of directions with an optional
// "normal_indices", one triple per triangle -- and then shades smooth (pt_set_mesh_normals); without the key it stays flat.
// A "mesh" also takes "texture": an image file read through EnvMapReader, relative to the scene file, with "uvs" -- "file" (the OBJ's
// vt lines and corner indices) or an inline array of (s, t) with an optional "uv_indices" -- and optionally "texture_filter" and
// "texture_wrap" (pt_set_mesh_texture); `textures` receives one entry per mesh, an empty image for a mesh without the key.
// A "mesh" takes inline "vertices" / "triangles" or "file": "x.obj" (relative to the scene file), and optionally "scale" and
// "translate", applied here in binary32 -- v * scale, then + translate, one rounded operation each -- before anything else; a
// file that holds one is checked as pt_set_scene_meshes checks it and leaves its geometry in `meshes`, in the order of its rows.
// What pt_set_mesh_texture takes, over a mesh's texture coordinates and its image as read.  (A size beyond 32 bits cannot come out
// of EnvMapReader: it caps a side at 16384; the library's own cap of 8192 is its check's to report.)
static pt_mesh_texture meshTextureView(const objreader::Mesh& m, const SceneTexture& tex) {
  pt_mesh_texture t{};
  t.struct_size = (std::uint32_t)sizeof(t);
  t.width = (std::uint32_t)tex.image.width; t.height = (std::uint32_t)tex.image.height;
  t.filter = tex.filter; t.wrap = tex.wrap;
  t.bgr = tex.image.bgr.data();
  t.uvs = m.uvs.data();
  t.n_uvs = (std::uint32_t)(m.uvs.size() / 2);
  t.uv_indices = m.uv_indices.empty() ? nullptr : m.uv_indices.data();
  return t;
}

std::vector<pt_scene_object> loadSceneFile(const std::string& path, pt_camera& camera, bool& hasCamera,
                                           std::vector<pt_scene_object_ex>& ex, std::vector<objreader::Mesh>& meshes,
                                           std::vector<SceneTexture>& textures) {
  const std::string at = "--scene '" + path + "': ";
  std::ifstream in(path, std::ios::binary);
  if (!in) throw std::runtime_error(at + "cannot open the file");
  std::stringstream text;
  text << in.rdbuf();
  json::Value root;
  try { root = json::parse(text.str()); } catch (const std::exception& e) { throw std::runtime_error(at + e.what()); }
  if (root.type != json::Value::Object || !root.has("objects") || root.at("objects").type != json::Value::Array)
    throw std::runtime_error(at + "expected an object with an array \"objects\"");
  const auto& list = root.at("objects").arr;
  if (list.empty() || list.size() > PT_MAX_SCENE_OBJECTS)
    throw std::runtime_error(at + "scene: object count must be 1.." + std::to_string(PT_MAX_SCENE_OBJECTS) + " (got " + std::to_string(list.size()) + ")");
  std::vector<pt_scene_object> objs(list.size());
  std::vector<pt_scene_object_ex> objsEx(list.size());
  bool anyPolygon = false;
  for (std::size_t i = 0; i < list.size(); ++i) {
    const json::Value& v = list[i];
    const std::string obj = "scene object " + std::to_string(i) + ": ";
    if (v.type != json::Value::Object) throw std::runtime_error(at + obj + "expected a JSON object");
    auto name = [&](const char* key) {
      if (!v.has(key) || v.at(key).type != json::Value::String) throw std::runtime_error(at + obj + "\"" + key + "\" must be a string");
      return v.at(key).str;
    };
    auto numbers = [&](const char* key, float* out, std::size_t k) {
      const json::Value& a = v.at(key);
      const bool scalar = k == 1 && a.type == json::Value::Number;
      if (!scalar && (a.type != json::Value::Array || a.arr.size() != k))
        throw std::runtime_error(at + obj + "\"" + key + "\" must be " + (k == 1 ? "a number" : "an array of " + std::to_string(k) + " numbers"));
      for (std::size_t c = 0; c < k; ++c) {
        const json::Value& x = scalar ? a : a.arr[c];
        if (x.type != json::Value::Number) throw std::runtime_error(at + obj + "\"" + key + "\" must hold numbers");
        out[c] = (float)x.num;
      }
    };
    for (const auto& kv : v.obj)
      if (kv.first != "shape" && kv.first != "material" && kv.first != "centre" && kv.first != "radius" && kv.first != "normal" &&
          kv.first != "colour" && kv.first != "emission" && kv.first != "vertices" && kv.first != "triangles" && kv.first != "file" &&
          kv.first != "scale" && kv.first != "translate" && kv.first != "normals" && kv.first != "normal_indices" &&
          kv.first != "texture" && kv.first != "uvs" && kv.first != "uv_indices" && kv.first != "texture_filter" && kv.first != "texture_wrap")
        throw std::runtime_error(at + obj + "unknown key \"" + kv.first + "\"");
    pt_scene_object& o = objs[i];
    o = pt_scene_object{};
    const std::string shape = name("shape"), material = name("material");
    if (shape == "sphere") o.shape = PT_SHAPE_SPHERE;
    else if (shape == "disc") o.shape = PT_SHAPE_DISC;
    else if (shape == "triangle") o.shape = PT_SHAPE_TRIANGLE;
    else if (shape == "parallelogram") o.shape = PT_SHAPE_PARALLELOGRAM;
    else if (shape == "mesh") o.shape = PT_SHAPE_MESH;
    else throw std::runtime_error(at + obj + "unknown shape '" + shape + "' (sphere, disc, triangle, parallelogram), or mesh");
    if (material == "diffuse") o.material = PT_MATERIAL_DIFFUSE;
    else if (material == "specular") o.material = PT_MATERIAL_SPECULAR;
    else if (material == "refractive") o.material = PT_MATERIAL_REFRACTIVE;
    else if (material == "emissive") o.material = PT_MATERIAL_EMISSIVE;
    else throw std::runtime_error(at + obj + "unknown material '" + material + "' (diffuse, specular, refractive, emissive)");
    const bool polygon = ptscene::is_polygon(o.shape), mesh = o.shape == PT_SHAPE_MESH;
    anyPolygon = anyPolygon || polygon || mesh;   // (a mesh needs the ex table too)
    pt_scene_object_ex& x = objsEx[i];
    x = pt_scene_object_ex{};
    if (!mesh)
      for (const char* key : {"triangles", "file", "scale", "translate", "normals", "normal_indices", "texture", "uvs", "uv_indices",
                              "texture_filter", "texture_wrap"})
        if (v.has(key)) throw std::runtime_error(at + obj + "\"" + key + "\" does not apply to a " + shape);
    if (mesh) {
      for (const char* key : {"centre", "radius", "normal"})
        if (v.has(key)) throw std::runtime_error(at + obj + "\"" + key + "\" does not apply to a mesh");
      objreader::Mesh m;
      SceneTexture tex;
      const std::size_t slash = path.find_last_of('/');
      auto beside = [&](const std::string& name) {   // a file named in the scene file is relative to it
        return (!name.empty() && name[0] == '/') || slash == std::string::npos ? name : path.substr(0, slash + 1) + name;
      };
      if (v.has("file")) {
        if (v.has("vertices") || v.has("triangles")) throw std::runtime_error(at + obj + "give \"file\" or \"vertices\" and \"triangles\", not both");
        if (v.at("file").type != json::Value::String) throw std::runtime_error(at + obj + "\"file\" must be a string");
        const std::string& name = v.at("file").str;
        const std::string full = beside(name);
        // "normals": "file" takes the OBJ's vn lines and its corners' normal indices (smooth shading: pt_set_mesh_normals)
        const bool fromFile = v.has("normals") && v.at("normals").type == json::Value::String;
        if (fromFile && v.at("normals").str != "file") throw std::runtime_error(at + obj + "\"normals\" must be \"file\" or an array of directions");
        if (fromFile && v.has("normal_indices")) throw std::runtime_error(at + obj + "\"normal_indices\" does not apply to \"normals\": \"file\"");
        try { m = objreader::read(full, fromFile); } catch (const std::exception& e) { throw std::runtime_error(at + obj + e.what()); }
        if (v.has("uvs") && v.at("uvs").type == json::Value::String) {   // "uvs": "file" takes the OBJ's vt lines and its corners' texture indices
          if (v.at("uvs").str != "file") throw std::runtime_error(at + obj + "\"uvs\" must be \"file\" or an array of (s, t) pairs");
          if (v.has("uv_indices")) throw std::runtime_error(at + obj + "\"uv_indices\" does not apply to \"uvs\": \"file\"");
          try {
            objreader::Mesh t = objreader::read_with_uvs(full);   // the same triangles in the same order: one fan rule
            m.uvs = std::move(t.uvs);
            m.uv_indices = std::move(t.uv_indices);
          } catch (const std::exception& e) { throw std::runtime_error(at + obj + e.what()); }
        }
      } else {
        if (!v.has("vertices") || !v.has("triangles")) throw std::runtime_error(at + obj + "a mesh needs \"file\", or \"vertices\" and \"triangles\"");
        const json::Value& vs = v.at("vertices");
        const json::Value& ts = v.at("triangles");
        if (vs.type != json::Value::Array || vs.arr.empty()) throw std::runtime_error(at + obj + "\"vertices\" must be a non-empty array of points");
        if (ts.type != json::Value::Array || ts.arr.empty()) throw std::runtime_error(at + obj + "\"triangles\" must be a non-empty array of index triples");
        for (const json::Value& q : vs.arr) {
          if (q.type != json::Value::Array || q.arr.size() != 3) throw std::runtime_error(at + obj + "\"vertices\" must hold arrays of 3 numbers");
          for (const json::Value& c : q.arr) {
            if (c.type != json::Value::Number) throw std::runtime_error(at + obj + "\"vertices\" must hold numbers");
            m.vertices.push_back((float)c.num);
          }
        }
        for (const json::Value& q : ts.arr) {
          if (q.type != json::Value::Array || q.arr.size() != 3) throw std::runtime_error(at + obj + "\"triangles\" must hold arrays of 3 indices");
          for (const json::Value& c : q.arr) {
            if (c.type != json::Value::Number || !(c.num >= 0.0) || c.num > 4294967295.0 || c.num != std::floor(c.num))
              throw std::runtime_error(at + obj + "\"triangles\" must hold non-negative integers");
            m.indices.push_back((std::uint32_t)c.num);
          }
        }
      }
      if (v.has("normals") && v.at("normals").type == json::Value::String) {
        if (!v.has("file")) throw std::runtime_error(at + obj + "\"normals\": \"file\" needs \"file\"");
      } else if (v.has("normals")) {   // inline: directions, and optionally an index triple per triangle (else one normal per vertex)
        const json::Value& ns = v.at("normals");
        if (ns.type != json::Value::Array || ns.arr.empty()) throw std::runtime_error(at + obj + "\"normals\" must be \"file\" or a non-empty array of directions");
        for (const json::Value& q : ns.arr) {
          if (q.type != json::Value::Array || q.arr.size() != 3) throw std::runtime_error(at + obj + "\"normals\" must hold arrays of 3 numbers");
          for (const json::Value& c : q.arr) {
            if (c.type != json::Value::Number) throw std::runtime_error(at + obj + "\"normals\" must hold numbers");
            m.normals.push_back((float)c.num);
          }
        }
        if (v.has("normal_indices")) {
          const json::Value& is = v.at("normal_indices");
          if (is.type != json::Value::Array || is.arr.size() != m.indices.size() / 3)
            throw std::runtime_error(at + obj + "\"normal_indices\" must hold one index triple per triangle");
          for (const json::Value& q : is.arr) {
            if (q.type != json::Value::Array || q.arr.size() != 3) throw std::runtime_error(at + obj + "\"normal_indices\" must hold arrays of 3 indices");
            for (const json::Value& c : q.arr) {
              if (c.type != json::Value::Number || !(c.num >= 0.0) || c.num > 4294967295.0 || c.num != std::floor(c.num))
                throw std::runtime_error(at + obj + "\"normal_indices\" must hold non-negative integers");
              m.normal_indices.push_back((std::uint32_t)c.num);
            }
          }
        }
      } else if (v.has("normal_indices")) throw std::runtime_error(at + obj + "\"normal_indices\" needs \"normals\"");
      if (v.has("texture")) {
        if (v.at("texture").type != json::Value::String) throw std::runtime_error(at + obj + "\"texture\" must be a string (an .hdr, .pfm or .exr file)");
        if (!v.has("uvs")) throw std::runtime_error(at + obj + "\"texture\" needs \"uvs\" (\"file\" or an array of (s, t) pairs)");
        if (v.at("uvs").type == json::Value::String) {
          if (!v.has("file")) throw std::runtime_error(at + obj + "\"uvs\": \"file\" needs \"file\"");
        } else {   // inline: (s, t) pairs, and optionally an index triple per triangle (else one pair per vertex)
          const json::Value& us = v.at("uvs");
          if (us.type != json::Value::Array || us.arr.empty()) throw std::runtime_error(at + obj + "\"uvs\" must be \"file\" or a non-empty array of (s, t) pairs");
          for (const json::Value& q : us.arr) {
            if (q.type != json::Value::Array || q.arr.size() != 2) throw std::runtime_error(at + obj + "\"uvs\" must hold arrays of 2 numbers");
            for (const json::Value& c : q.arr) {
              if (c.type != json::Value::Number) throw std::runtime_error(at + obj + "\"uvs\" must hold numbers");
              m.uvs.push_back((float)c.num);
            }
          }
          if (v.has("uv_indices")) {
            const json::Value& is = v.at("uv_indices");
            if (is.type != json::Value::Array || is.arr.size() != m.indices.size() / 3)
              throw std::runtime_error(at + obj + "\"uv_indices\" must hold one index triple per triangle");
            for (const json::Value& q : is.arr) {
              if (q.type != json::Value::Array || q.arr.size() != 3) throw std::runtime_error(at + obj + "\"uv_indices\" must hold arrays of 3 indices");
              for (const json::Value& c : q.arr) {
                if (c.type != json::Value::Number || !(c.num >= 0.0) || c.num > 4294967295.0 || c.num != std::floor(c.num))
                  throw std::runtime_error(at + obj + "\"uv_indices\" must hold non-negative integers");
                m.uv_indices.push_back((std::uint32_t)c.num);
              }
            }
          }
        }
        for (const char* key : {"texture_filter", "texture_wrap"})
          if (v.has(key) && v.at(key).type != json::Value::String) throw std::runtime_error(at + obj + "\"" + key + "\" must be a string");
        if (v.has("texture_filter")) {
          const std::string& f = v.at("texture_filter").str;
          if (f == "nearest") tex.filter = PT_TEX_FILTER_NEAREST;
          else if (f == "bilinear") tex.filter = PT_TEX_FILTER_BILINEAR;
          else throw std::runtime_error(at + obj + "unknown \"texture_filter\" '" + f + "' (nearest, bilinear)");
        }
        if (v.has("texture_wrap")) {
          const std::string& w = v.at("texture_wrap").str;
          if (w == "repeat") tex.wrap = PT_TEX_WRAP_REPEAT;
          else if (w == "clamp") tex.wrap = PT_TEX_WRAP_CLAMP;
          else throw std::runtime_error(at + obj + "unknown \"texture_wrap\" '" + w + "' (repeat, clamp)");
        }
        try { tex.image = env_map::read(beside(v.at("texture").str)); } catch (const std::exception& e) { throw std::runtime_error(at + obj + "\"texture\": " + e.what()); }
      } else {
        for (const char* key : {"uvs", "uv_indices", "texture_filter", "texture_wrap"})
          if (v.has(key)) throw std::runtime_error(at + obj + "\"" + key + "\" needs \"texture\"");
      }
      float scale[3] = {1.f, 1.f, 1.f}, translate[3] = {0.f, 0.f, 0.f};
      if (v.has("scale")) {
        if (v.at("scale").type == json::Value::Number) scale[0] = scale[1] = scale[2] = (float)v.at("scale").num;
        else numbers("scale", scale, 3);
      }
      if (v.has("translate")) numbers("translate", translate, 3);
      // "scale" applies to positions only: under a non-uniform one a normal would need the inverse transpose, which is not built
      if (!m.normals.empty() && (scale[0] != scale[1] || scale[1] != scale[2]))
        throw std::runtime_error(at + obj + "a non-uniform \"scale\" cannot be combined with \"normals\" (normals are not transformed)");
      if (v.has("scale") || v.has("translate"))
        for (std::size_t k = 0; k < m.vertices.size(); ++k) {
          volatile float scaled = m.vertices[k] * scale[k % 3];
          volatile float moved = scaled + translate[k % 3];
          m.vertices[k] = moved;
        }
      meshes.push_back(std::move(m));
      textures.push_back(std::move(tex));
    } else if (polygon) {
      for (const char* key : {"centre", "radius", "normal"})
        if (v.has(key)) throw std::runtime_error(at + obj + "\"" + key + "\" does not apply to a " + shape + " (it takes \"vertices\")");
      if (!v.has("vertices")) throw std::runtime_error(at + obj + "\"vertices\" is missing (a " + shape + " needs three)");
      const json::Value& a = v.at("vertices");
      if (a.type != json::Value::Array || a.arr.size() != 3) throw std::runtime_error(at + obj + "\"vertices\" must be an array of 3 points");
      for (std::size_t p = 0; p < 3; ++p) {
        if (a.arr[p].type != json::Value::Array || a.arr[p].arr.size() != 3)
          throw std::runtime_error(at + obj + "\"vertices\" must hold arrays of 3 numbers");
        for (std::size_t c = 0; c < 3; ++c) {
          if (a.arr[p].arr[c].type != json::Value::Number) throw std::runtime_error(at + obj + "\"vertices\" must hold numbers");
          x.vertex[p][c] = (float)a.arr[p].arr[c].num;
        }
      }
    } else {
    if (v.has("vertices")) throw std::runtime_error(at + obj + "\"vertices\" does not apply to a " + shape);
    for (const char* key : {"centre", "radius"})
      if (!v.has(key)) throw std::runtime_error(at + obj + "\"" + key + "\" is missing");
    numbers("centre", o.centre, 3);
    numbers("radius", &o.radius, 1);
    }
    if (o.shape == PT_SHAPE_DISC) {
      if (!v.has("normal")) throw std::runtime_error(at + obj + "\"normal\" is missing (a disc needs one)");
      numbers("normal", o.normal, 3);
    }
    if (v.has("colour") && v.has("emission")) throw std::runtime_error(at + obj + "give \"colour\" or \"emission\", not both");
    o.colour[0] = o.colour[1] = o.colour[2] = 1.f;
    if (v.has("colour")) numbers("colour", o.colour, 3);
    if (v.has("emission")) numbers("emission", o.colour, 3);
    std::memcpy(&x, &o, sizeof(o));   // the first 48 bytes of pt_scene_object_ex are pt_scene_object
  }
  std::vector<pt_mesh> views;
  for (const objreader::Mesh& m : meshes)
    views.push_back(pt_mesh{(std::uint32_t)sizeof(pt_mesh), (std::uint32_t)(m.vertices.size() / 3), (std::uint32_t)(m.indices.size() / 3),
                            m.vertices.data(), m.indices.data()});
  const std::string bad = !meshes.empty() ? ptmesh::check(objsEx.data(), (std::uint32_t)objsEx.size(), (std::uint32_t)sizeof(pt_scene_object_ex),
                                                          views.data(), (std::uint32_t)views.size())
                          : anyPolygon ? ptscene::check_ex(objsEx.data(), (std::uint32_t)objsEx.size(), (std::uint32_t)sizeof(pt_scene_object_ex))
                                     : ptscene::check(objs.data(), (std::uint32_t)objs.size());
  if (!bad.empty()) throw std::runtime_error(at + bad);
  for (std::size_t k = 0; k < meshes.size(); ++k) {   // the normals, as pt_set_mesh_normals checks them, before a device is attached
    const objreader::Mesh& m = meshes[k];
    if (m.normals.empty()) continue;
    const std::string badn = ptmesh::check_normals((std::uint32_t)k, (std::uint32_t)(m.vertices.size() / 3), (std::uint32_t)(m.indices.size() / 3),
                                                   m.indices.data(), m.normals.data(), (std::uint32_t)(m.normals.size() / 3),
                                                   m.normal_indices.empty() ? nullptr : m.normal_indices.data());
    if (!badn.empty()) throw std::runtime_error(at + badn);
  }
  for (std::size_t k = 0; k < meshes.size(); ++k) {   // the textures, as pt_set_mesh_texture checks them, before a device is attached
    const objreader::Mesh& m = meshes[k];
    if (textures[k].image.bgr.empty()) continue;
    const pt_mesh_texture t = meshTextureView(m, textures[k]);
    const std::string badt = ptmesh::check_texture((std::uint32_t)k, (std::uint32_t)(m.vertices.size() / 3), (std::uint32_t)(m.indices.size() / 3),
                                                   m.indices.data(), &t);
    if (!badt.empty()) throw std::runtime_error(at + badt);
  }
  ex.clear();
  if (anyPolygon) ex = objsEx;
  camera = ptcamera::default_camera();
  hasCamera = root.has("camera");
  if (hasCamera) {
    const json::Value& v = root.at("camera");
    if (v.type != json::Value::Object) throw std::runtime_error(at + "camera: expected a JSON object");
    auto numbers = [&](const char* key, float* out, std::size_t k) {
      if (!v.has(key)) return;
      const json::Value& a = v.at(key);
      const bool scalar = k == 1 && a.type == json::Value::Number;
      if (!scalar && (a.type != json::Value::Array || a.arr.size() != k))
        throw std::runtime_error(at + "camera: \"" + key + "\" must be " + (k == 1 ? "a number" : "an array of " + std::to_string(k) + " numbers"));
      for (std::size_t c = 0; c < k; ++c) {
        const json::Value& x = scalar ? a : a.arr[c];
        if (x.type != json::Value::Number) throw std::runtime_error(at + "camera: \"" + key + "\" must hold numbers");
        out[c] = (float)x.num;
      }
    };
    for (const auto& kv : v.obj)
      if (kv.first != "position" && kv.first != "look_at" && kv.first != "up" && kv.first != "lens_radius" && kv.first != "focus_distance")
        throw std::runtime_error(at + "camera: unknown key \"" + kv.first + "\"");
    numbers("position", camera.position, 3);
    numbers("look_at", camera.look_at, 3);
    numbers("up", camera.up, 3);
    numbers("lens_radius", &camera.lens_radius, 1);
    // a lens must say where it focuses: the default distance only stands in for a pinhole, which ignores it
    if (v.has("lens_radius") && camera.lens_radius > 0.f && !v.has("focus_distance")) camera.focus_distance = 0.f;
    numbers("focus_distance", &camera.focus_distance, 1);
    const std::string badCamera = ptcamera::check(&camera);
    if (!badCamera.empty()) throw std::runtime_error(at + badCamera);
  }
  return objs;
}

pt_nif_memo_stats PathTracerApp::memoStatsRequest() {
  pt_nif_memo_stats s{};
  s.struct_size = sizeof(pt_nif_memo_stats);
  return s;
}

void PathTracerApp::countMemo(const std::vector<pt_nif_memo_stats>& memo) {
  for (const auto& s : memo) { memoServed += s.served; memoEscaped += s.escaped; memoRows += s.evaluations; }
}

// escaped paths the memo served since the last save interval, and the NIF rows that still ran
void PathTracerApp::logMemo() {
  if (nifMemo) pt_log::info_("NIF memo: served {} of {} escaped, {} rows executed", memoServed, memoEscaped, memoRows);
  memoServed = memoEscaped = memoRows = 0;
}

void PathTracerApp::init(const OptionMap& options) {
  args = options;
  samplesPerPixel = args.u32("samples");
  samplesPerIpuStep = args.u32("samples-per-step");
  if (samplesPerIpuStep) samplesPerPixel = (std::uint32_t)roundSamplesPerPixel(samplesPerPixel, samplesPerIpuStep);
  // values the reference would divide by (PathTracerApp.cpp:232 `step % saveInterval`, tiles / ipus): reject them up front
  if (args.u32("ipus") == 0) throw std::runtime_error("--ipus must be at least 1.");
  if (args.u32("save-interval") == 0) throw std::runtime_error("--save-interval must be at least 1.");
  if (samplesPerIpuStep == 0) throw std::runtime_error("--samples-per-step must be at least 1.");
  nifSharing = nifSharingMode(args.str("share-nif-evaluations"));
  nifMemo = nifMemoBytes(args.str("nif-memo-gib"));
  meshBuilder = meshBuilderMode(args.str("mesh-builder"));
  meshDeviceTree = meshDeviceTreeKind(args.str("mesh-device-tree"));
  // --denoise (an extension): the values are checked here, before any device is attached
  denoise = args.flag("denoise");
  saveFeatures = args.flag("save-features");
  pt_denoise_default_params(&denoiseParams);
  denoiseParams.iterations = args.u32("denoise-iterations");
  denoiseParams.sigma_colour = args.f32("denoise-sigma-colour");
  denoiseParams.sigma_normal = args.f32("denoise-sigma-normal");
  denoiseParams.sigma_depth = args.f32("denoise-sigma-depth");
  if (denoiseParams.iterations < 1 || denoiseParams.iterations > 6)
    throw std::runtime_error("--denoise-iterations must be 1..6; got " + args.str("denoise-iterations"));
  for (const char* name : {"denoise-sigma-colour", "denoise-sigma-normal", "denoise-sigma-depth"})
    if (!std::isfinite(args.f32(name))) throw std::runtime_error(std::string("--") + name + " must be finite; got " + args.str(name));
  if (args.has("scene") && !args.str("scene").empty()) scene = loadSceneFile(args.str("scene"), camera, hasCamera, sceneEx, sceneMeshes, sceneTextures);
  // the reference hands --outfile to cv::imwrite, which picks the codec by extension (AccumulatedImage.cpp:49) and throws for one
  // it has no writer for -- here before anything is rendered, not at the first save interval
  if (!image_io::ldrWriterFor(args.str("outfile")))
    throw std::runtime_error("--outfile '" + args.str("outfile") + "': could not find a writer for the specified extension "
                             "(built in: .png .jpg .bmp .ppm .pnm .tif .tiff; the HDR image goes to <name>.exr)");
  // --env-map (an extension): the image is read and checked here, before any device is attached (so --compile-only validates it)
  const bool constantEnv = args.has("constant-env") && !args.str("constant-env").empty();
  envMapFilterMode = envMapFilter(args.str("env-map-filter"));
  // --env-guide env builds the guide from the environment: without one (no --assets, --env-map or --constant-env) the library
  // would answer PT_ERR_NOT_READY, and the tool says so in the library's words before it looks for any asset
  if (args.has("env-guide") && args.str("env-guide") == "env" && !constantEnv && (!args.has("env-map") || args.str("env-map").empty()) &&
      (!args.has("assets") || args.str("assets").empty()))
    throw std::runtime_error(std::string("--env-guide env: ") + ptguide::kNoEnvironment);
  if (args.has("env-map") && !args.str("env-map").empty()) {
    if (constantEnv) throw std::runtime_error("--env-map and --constant-env are both given: the environment is one or the other");
    try {
      envMap = env_map::read(args.str("env-map"));
    } catch (const std::exception& e) {
      throw std::runtime_error(std::string("--env-map ") + e.what());
    }
    for (std::size_t i = 0; i < envMap.bgr.size(); ++i)
      if (!(envMap.bgr[i] >= 0.f) || !std::isfinite(envMap.bgr[i]))
        throw std::runtime_error("--env-map '" + args.str("env-map") + "': texel at row " + std::to_string(i / 3 / envMap.width) + ", column " +
                                 std::to_string(i / 3 % envMap.width) + ", channel " + std::to_string(i % 3) + " is " + std::to_string(envMap.bgr[i]) +
                                 ": texels must be finite and not negative");
    pt_log::info_("Environment map '{}': {} x {}, {} filter", args.str("env-map"), envMap.width, envMap.height, args.str("env-map-filter"));
  } else if (!constantEnv) {
    if (!loadNifModels(args.u32("ipus"), args.str("assets"))) throw std::runtime_error("Could not load NIF model.");
  }
  // --env-guide (an extension): read, checked and its tables built once here with the library's own code (ptmi_env_guide.h),
  // before any device is attached (so --compile-only validates it); the image goes to every handle in execute()
  if (args.has("env-guide") && !args.str("env-guide").empty()) {
    const std::string file = args.str("env-guide");
    envGuideFromMap = file == "map";
    envGuideFromEnv = file == "env";
    if (envGuideFromEnv) {
      // no image: the library builds the guide from the environment each handle holds (pt_set_env_guide_from_environment)
      const pt_env_guide_auto a = envGuideAutoRequest(args.str("env-guide-size"), args.f32("env-guide-alpha"), args.u32("env-guide-supersample"));
      const std::string bad = ptguide::check_auto(&a);
      if (!bad.empty()) throw std::runtime_error("--env-guide env: " + bad);
      pt_log::info_("Environment guide from the environment in force: {} x {} cells, {} x {} lookups per cell, alpha {}", a.rows, a.cols,
                    a.supersample, a.supersample, ptguide::num(a.alpha));
    } else if (envGuideFromMap) {
      if (envMap.bgr.empty()) throw std::runtime_error("--env-guide map needs --env-map: there is no map to reuse");
    } else {
      try {
        envGuide = env_map::read(file);
      } catch (const std::exception& e) {
        throw std::runtime_error(std::string("--env-guide ") + e.what());
      }
    }
    if (!envGuideFromEnv) {
      const pt_env_guide g = envGuideRequest(args.str("env-guide-size"), args.f32("env-guide-alpha"));
      std::string bad = ptguide::check(&g);
      ptguide::Table table;
      if (bad.empty()) bad = ptguide::build(g, table);
      if (!bad.empty()) throw std::runtime_error("--env-guide '" + file + "': " + bad);
      pt_log::info_("Environment guide '{}': {} x {} image, {} x {} cells, alpha {}", file, g.width, g.height, g.rows, g.cols, table.alpha);
    }
  }
  // --light-guide-beta (an extension): checked with the environment guide's alpha by the library's own code
  // (ptmi_light_guide.h), before any device is attached; set on every handle in execute()
  lightGuideBeta = args.f32("light-guide-beta");
  {
    const pt_light_guide g{(std::uint32_t)sizeof(pt_light_guide), lightGuideBeta};
    const std::string bad = ptlight::check(&g, envGuideRows ? (double)envGuideAlpha : 0.0);
    if (!bad.empty()) throw std::runtime_error("--light-guide-beta: " + bad);
    lightGuidePolygons = args.flag("light-guide-polygons");
    if (lightGuidePolygons && !(lightGuideBeta > 0.f))
      throw std::runtime_error("--light-guide-polygons needs --light-guide-beta > 0: there is no emitter guide to extend");
    if (lightGuideBeta > 0.f) {
      ptlight::Table table;
      if (lightGuidePolygons && !sceneEx.empty()) {   // the table as the library will build it: the stored vertices
        std::vector<pt_scene_object_ex> stored(sceneEx);
        ptscene::normalise_ex(stored.data(), (std::uint32_t)stored.size());
        float vertex[PT_MAX_SCENE_OBJECTS][3][3] = {};
        pt_scene_object head[PT_MAX_SCENE_OBJECTS] = {};
        for (std::size_t i = 0; i < stored.size(); ++i) {
          std::memcpy(&head[i], &stored[i], sizeof(pt_scene_object));
          std::memcpy(vertex[i], stored[i].vertex, sizeof(vertex[i]));
        }
        ptlight::build(lightGuideBeta, head, (std::uint32_t)stored.size(), table, vertex);
      } else
      ptlight::build(lightGuideBeta, scene.data(), (std::uint32_t)scene.size(), table);   // (no --scene: the built-in one, which has no emitter)
      if (table.active() && table.polygons) pt_log::info_("light guide: beta {}, {} emitters, polygons included", ptlight::num(lightGuideBeta), table.n);
      else if (table.active()) pt_log::info_("light guide: beta {}, {} emitters", ptlight::num(lightGuideBeta), table.n);   // the value as given, %g
      else pt_log::info_("light guide: inactive: the scene has no emitter");
    }
  }
}

// The pt_env_guide of --env-guide / --env-guide-size / --env-guide-alpha over the image read in the constructor.
pt_env_guide PathTracerApp::envGuideRequest(const std::string& size, float alpha) {
  const env_map::Image& img = envGuideFromMap ? envMap : envGuide;
  pt_env_guide g{};
  g.struct_size = sizeof(pt_env_guide);
  g.width = (std::uint32_t)img.width; g.height = (std::uint32_t)img.height;
  g.bgr = img.bgr.data();
  g.alpha = alpha;
  if (size.empty()) {
    ptguide::default_grid(g.width, g.height, g.rows, g.cols);
  } else {
    unsigned r = 0, c = 0;
    char tail = 0;
    if (std::sscanf(size.c_str(), "%ux%u%c", &r, &c, &tail) != 2) throw std::runtime_error("--env-guide-size expects RxC, e.g. 64x128; got '" + size + "'");
    g.rows = r; g.cols = c;
  }
  envGuideRows = g.rows; envGuideCols = g.cols; envGuideAlpha = alpha;
  return g;
}

// The pt_env_guide_auto of --env-guide env / --env-guide-size / --env-guide-alpha / --env-guide-supersample; follow is on, so
// a NIF loaded later (the interactive load_nif) keeps the guide current.
pt_env_guide_auto PathTracerApp::envGuideAutoRequest(const std::string& size, float alpha, std::uint32_t supersample) {
  pt_env_guide_auto a{};
  a.struct_size = sizeof(pt_env_guide_auto);
  a.rows = 256; a.cols = 512;
  if (!size.empty()) {
    unsigned r = 0, c = 0;
    char tail = 0;
    if (std::sscanf(size.c_str(), "%ux%u%c", &r, &c, &tail) != 2) throw std::runtime_error("--env-guide-size expects RxC, e.g. 64x128; got '" + size + "'");
    a.rows = r; a.cols = c;
  }
  a.supersample = supersample;
  a.alpha = alpha;
  a.follow = 1;
  envGuideRows = a.rows; envGuideCols = a.cols; envGuideAlpha = alpha; envGuideSupersample = supersample;
  return a;
}

bool PathTracerApp::loadNifModels(std::size_t numDevices, const std::string& assetPath) {
  try {
    const auto metaFile = assetPath + "/nif_metadata.txt";
    const auto h5File = assetPath + "/converted.hdf5";          // the reference's asset (PathTracerApp.cpp:110)
    const auto weightFile = assetPath + "/converted.ptnif";      // flat side-car written by nif_assets.write_ptnif
    std::shared_ptr<NifModel::Data> nifData;
    if (std::ifstream(h5File).good()) {
      nifData = std::make_shared<NifModel::Data>(h5File, metaFile);
    } else if (std::ifstream(weightFile).good()) {
      nifData = std::make_shared<NifModel::Data>(weightFile, metaFile);
    } else if (args.flag("synthetic-nif")) {
      pt_log::warn_("'{}' not found: using seeded synthetic NIF weights", weightFile);
      nifData = NifModel::Data::synthetic(metaFile, 2024u);
    } else {
      throw std::runtime_error("neither '" + h5File + "' nor '" + weightFile + "' found (pass --synthetic-nif for stand-in weights)");
    }
    models.clear();
    for (std::size_t c = 0; c < numDevices; ++c)
      models.push_back(std::make_unique<NifModel>(nifData, "env_nif_gpu" + std::to_string(c)));
  } catch (std::exception& e) {
    pt_log::error_("Could not load NIF model from '{}'. Exception: {}", assetPath, e.what());
    return false;
  }
  return true;
}

void PathTracerApp::attach() {
  if (pt_abi_version() != PTMI_ABI_VERSION)   // built against one include/ptmi.h, running on another libptmi.so
    throw std::runtime_error("libptmi.so has ABI version " + std::to_string(pt_abi_version()) + ", this host was built against " +
                             std::to_string(PTMI_ABI_VERSION));
  const auto imageWidth = args.u32("width"), imageHeight = args.u32("height");
  const std::size_t numDevices = args.u32("ipus");
  geometry.numTiles *= numDevices;  // tiles scale with the device count as on a multi-IPU target
  // logical device d runs on GPU deviceMap[d] (default d).  RCCL needs one GPU per rank: logical devices that share a GPU
  // (a one-GPU box rehearsing the multi-device loop) gather their HDR tiles through the host instead.
  std::vector<std::int32_t> deviceMap(numDevices);
  for (std::size_t d = 0; d < numDevices; ++d) deviceMap[d] = (std::int32_t)d;
  if (args.has("devices") && !args.str("devices").empty()) {
    std::vector<std::int32_t> listed;
    std::stringstream list(args.str("devices"));
    for (std::string item; std::getline(list, item, ',');) {
      std::size_t used = 0;
      int v = -1;
      try { v = std::stoi(item, &used); } catch (const std::exception&) { used = 0; }
      if (used != item.size() || item.empty() || v < 0) throw std::runtime_error("--devices expects a comma-separated list of GPU ordinals, got '" + args.str("devices") + "'");
      listed.push_back(v);
    }
    if (listed.size() != numDevices) throw std::runtime_error("--devices must name one GPU per logical device (--ipus " + std::to_string(numDevices) + ")");
    deviceMap = listed;
  }
  hostGather = args.flag("host-gather");
  for (std::size_t d = 0; d < numDevices && !hostGather; ++d)
    for (std::size_t o = 0; o < d; ++o)
      if (deviceMap[o] == deviceMap[d]) {
        pt_log::info_("Logical devices {} and {} share GPU {}: HDR tiles are gathered through the host, not over RCCL", o, d, deviceMap[d]);
        hostGather = true;
        break;
      }
  const auto raysPerJob = calculateMaxRaysPerTile(imageWidth, imageHeight, geometry);
  ipuJobs.reserve(geometry.numTiles);
  for (std::size_t t = 0; t < geometry.numTiles; ++t) ipuJobs.emplace_back(raysPerJob, args, t);   // PathTracerApp.cpp:323-326
  const std::size_t jobsPerDevice = geometry.numTiles / numDevices;
  const std::size_t itemsPerDevice = raysPerJob * jobsPerDevice;
  for (std::size_t d = 0; d < numDevices; ++d) {
    pt_config cfg{};
    cfg.struct_size = sizeof(pt_config);
    // every job of the device contributes its slice and the per-tile scalars (the host half of buildGraph)
    for (std::size_t j = 0; j < jobsPerDevice; ++j)
      ipuJobs[d * jobsPerDevice + j].buildGraph(cfg, d, j * raysPerJob, geometry, args);
    cfg.max_path_length = args.u32("max-path-length");
    cfg.aa_noise_type = aaNoiseType(args.str("aa-noise-type"));
    cfg.sample_precision = PT_SAMPLES_HALF;
    cfg.device = deviceMap[d];
    // with load balancing on the resident film the devices trade image tiles: room for any deal with equal tile counts
    deviceCapacity = itemsPerDevice;
    if (args.flag("enable-load-balancing"))
      deviceCapacity = std::max(deviceCapacity, maxTileItemsPerDevice(imageWidth, imageHeight, numDevices));
    cfg.max_work_items = (std::uint32_t)deviceCapacity;
    pt_handle h = nullptr;
    if (pt_create(&cfg, &h)) throw std::runtime_error(std::string("Could not attach to device: ") + pt_last_error(nullptr));
    devices.push_back(h);
    if (pt_set_nif_sharing(h, nifSharing))
      throw std::runtime_error(std::string("--share-nif-evaluations: ") + pt_last_error(h));
    if (meshBuilder != PT_MESH_BUILDER_HOST) {   // (the default makes no call at all)
      const pt_mesh_build_options mo{(std::uint32_t)sizeof(pt_mesh_build_options), meshBuilder, PT_MESH_POSE_REBUILD};
      if (pt_set_mesh_build(h, &mo)) throw std::runtime_error(std::string("--mesh-builder: ") + pt_last_error(h));
    }
    if (meshDeviceTree != PT_MESH_DEVICE_TREE_LINEAR)   // (the default makes no call at all)
      if (pt_set_mesh_device_tree(h, meshDeviceTree)) throw std::runtime_error(std::string("--mesh-device-tree: ") + pt_last_error(h));
    if (!sceneMeshes.empty()) {   // the file holds a mesh
      std::vector<pt_mesh> views;
      for (const objreader::Mesh& m : sceneMeshes)
        views.push_back(pt_mesh{(std::uint32_t)sizeof(pt_mesh), (std::uint32_t)(m.vertices.size() / 3), (std::uint32_t)(m.indices.size() / 3),
                                m.vertices.data(), m.indices.data()});
      if (pt_set_scene_meshes(h, sceneEx.data(), (std::uint32_t)sceneEx.size(), (std::uint32_t)sizeof(pt_scene_object_ex), views.data(),
                              (std::uint32_t)views.size()))
        throw std::runtime_error(std::string("--scene: ") + pt_last_error(h));
      for (std::size_t k = 0; k < sceneMeshes.size(); ++k) {   // a mesh with "normals" shades smooth
        const objreader::Mesh& m = sceneMeshes[k];
        if (!m.normals.empty() && pt_set_mesh_normals(h, (std::uint32_t)k, m.normals.data(), (std::uint32_t)(m.normals.size() / 3),
                                                     m.normal_indices.empty() ? nullptr : m.normal_indices.data()))
          throw std::runtime_error(std::string("--scene: ") + pt_last_error(h));
      }
      for (std::size_t k = 0; k < sceneMeshes.size(); ++k) {   // a mesh with "texture", after its normals
        if (sceneTextures[k].image.bgr.empty()) continue;
        const pt_mesh_texture t = meshTextureView(sceneMeshes[k], sceneTextures[k]);
        if (pt_set_mesh_texture(h, (std::uint32_t)k, &t)) throw std::runtime_error(std::string("--scene: ") + pt_last_error(h));
      }
    } else if (!sceneEx.empty()) {   // the file holds a polygon
      if (pt_set_scene_ex(h, sceneEx.data(), (std::uint32_t)sceneEx.size(), (std::uint32_t)sizeof(pt_scene_object_ex)))
        throw std::runtime_error(std::string("--scene: ") + pt_last_error(h));
    } else if (!scene.empty() && pt_set_scene(h, scene.data(), (std::uint32_t)scene.size()))
      throw std::runtime_error(std::string("--scene: ") + pt_last_error(h));
    if (hasCamera && pt_set_camera(h, &camera))
      throw std::runtime_error(std::string("--scene: ") + pt_last_error(h));
  }
  // one memo per logical device: logical devices that share a GPU need room for all of theirs, or none runs with one
  for (std::size_t d = 0; d < numDevices && nifMemo; ++d) {
    const int rc = pt_set_nif_memo(devices[d], nifMemo);
    if (rc == PT_OK) continue;
    if (rc != PT_ERR_OUT_OF_MEMORY) throw std::runtime_error(std::string("--nif-memo-gib: ") + pt_last_error(devices[d]));
    pt_log::warn_("--nif-memo-gib {}: {} memos do not fit on their GPUs ({}): rendering without a NIF memo", args.str("nif-memo-gib"),
                  numDevices, pt_last_error(devices[d]));
    for (std::size_t o = 0; o < d; ++o) pt_set_nif_memo(devices[o], 0);
    nifMemo = 0;
  }
  if (numDevices > 1 && hostGather) {
    pt_log::info_("HDR tiles of {} devices are gathered through the host", numDevices);
  } else if (numDevices > 1) {
    // one RCCL communicator over the devices of this process: rank d = device d, HDR tiles are gathered to rank 0
    if (pt_comm_init_all(devices.data(), (int)numDevices))
      throw std::runtime_error(std::string("Could not create the RCCL communicator: ") + pt_last_error(devices[0]));
    pt_log::info_("RCCL communicator over {} devices", numDevices);
  }
  pt_log::info_("Tracebuffer shape: [{}, {}]", ipuJobs.size(), sizeof(TraceRecord) * raysPerJob);
}

void PathTracerApp::initialiseState(std::uint32_t imageWidth, std::uint32_t imageHeight) {
  auto jobs = createTracingJobs(imageWidth, imageHeight, geometry);
  pt_log::info_("Created worklists for {} tiles", jobs.size());
  traceState = std::make_unique<PathTracerState>(imageWidth, imageHeight, jobs.size() * jobs.front().size());
  traceState->work.randomiseWorkList(jobs);
  traceState->work.getWork().active() = traceState->work.getWork().inactive();
}

// One call per device, each from its own thread (the devices work at the same time, as the IPUs of one Poplar engine do:
// PathTracerApp.cpp:205-252).  The FIRST failure is the one reported; the thread that fails asks every other device
// to abort its communicator (pt_comm_abort), so a sibling waiting inside the HDR gather for the failed rank returns at
// once with PT_ERR_COMM instead of at its deadline -- the join below can therefore never wait for ever.
template <class F>
void PathTracerApp::onEveryDevice(const char* what, F&& call) {
  std::vector<std::string> errors(devices.size());
  std::atomic<int> firstFailed{-1};
  if (devices.size() == 1) {
    if (call(0)) { errors[0] = pt_last_error(devices[0]); firstFailed = 0; }
  } else {
    std::vector<std::thread> runners;
    for (std::size_t d = 0; d < devices.size(); ++d)
      runners.emplace_back([&, d]() {
        if (!call(d)) return;
        errors[d] = pt_last_error(devices[d]);
        int none = -1;
        if (firstFailed.compare_exchange_strong(none, (int)d))
          for (std::size_t o = 0; o < devices.size(); ++o) if (o != d) pt_comm_abort(devices[o]);
      });
    for (auto& t : runners) t.join();
  }
  const int f = firstFailed.load();
  if (f >= 0) throw std::runtime_error(std::string(what) + " failed on device " + std::to_string(f) + ": " + errors[(std::size_t)f]);
}

void PathTracerApp::execute() {
  const auto imageWidth = args.u32("width"), imageHeight = args.u32("height");
  const auto seed = args.u64("seed");
  const float antiAliasingScale = args.f32("aa-noise-scale");
  const float fieldOfView = args.f32("fov") * (float)(M_PI / 180.f);      // PathTracerApp.cpp:574
  const auto steps = samplesPerPixel / samplesPerIpuStep;
  const float degrees = args.f32("env-map-rotation");
  const float radians = (degrees / 360.f) * (float)(2.0 * M_PI);          // PathTracerApp.cpp:584

  renderStartTime = std::chrono::steady_clock::now();
  pt_log::debug_("Host-phase trace ranges: {}", pt_trace::api().push ? pt_trace::api().library : "no ROCTx library found (ranges are no-ops)");

  // programs init_nif_weights and init_render_settings (PathTracerApp.cpp:612-614)
  auto initialisation = std::make_unique<pt_trace::Range>("initialisation");   // PathTracerApp.cpp:567-639
  for (std::size_t d = 0; d < devices.size(); ++d) {
    if (args.has("constant-env") && !args.str("constant-env").empty()) {
      float rgb[3] = {1, 1, 1};
      if (std::sscanf(args.str("constant-env").c_str(), "%f,%f,%f", &rgb[0], &rgb[1], &rgb[2]) != 3)
        throw std::runtime_error("--constant-env expects r,g,b");
      check(devices[d], pt_set_constant_env(devices[d], rgb), "set_constant_env");
    } else if (!envMap.bgr.empty()) {
      check(devices[d], pt_set_env_map(devices[d], envMap.bgr.data(), (std::uint32_t)envMap.width, (std::uint32_t)envMap.height, envMapFilterMode),
            "set_env_map");
    } else {
      models[d]->analyseModel((std::size_t)imageWidth * imageHeight / devices.size());
      models[d]->upload(devices[d]);
    }
    check(devices[d], pt_set_render_settings(devices[d], seed, antiAliasingScale, fieldOfView, radians, samplesPerIpuStep),
          "init_render_settings");
    if (envGuideRows && envGuideFromEnv) {   // --env-guide env: every handle derives the same tables from its own replica
      const pt_env_guide_auto a = envGuideAutoRequest(std::to_string(envGuideRows) + "x" + std::to_string(envGuideCols), envGuideAlpha, envGuideSupersample);
      check(devices[d], pt_set_env_guide_from_environment(devices[d], &a), "set_env_guide_from_environment");
      pt_env_guide_info info{};
      info.struct_size = sizeof(pt_env_guide_info);
      check(devices[d], pt_get_env_guide_info(devices[d], &info), "get_env_guide_info");
      pt_log::info_("Environment guide built on device {}: {} x {} cells, supersample {}, build_ms {}, {} values clamped", d, info.rows, info.cols,
                    info.supersample, info.build_ms, info.clamped);
    } else if (envGuideRows) {   // --env-guide: every handle samples by the same guide
      const pt_env_guide g = envGuideRequest(std::to_string(envGuideRows) + "x" + std::to_string(envGuideCols), envGuideAlpha);
      check(devices[d], pt_set_env_guide(devices[d], &g), "set_env_guide");
    }
    if (lightGuideBeta > 0.f) {   // --light-guide-beta: every handle samples its emitters alike
      const pt_light_guide g{(std::uint32_t)sizeof(pt_light_guide), lightGuideBeta};
      const pt_light_guide_ex gx{(std::uint32_t)sizeof(pt_light_guide_ex), lightGuideBeta, (std::uint32_t)PT_LIGHT_GUIDE_POLYGONS};
      if (lightGuidePolygons) check(devices[d], pt_set_light_guide_ex(devices[d], &gx), "set_light_guide_ex");
      else check(devices[d], pt_set_light_guide(devices[d], &g), "set_light_guide");
    }
  }
  initialiseState(imageWidth, imageHeight);
  initialisation.reset();
  pt_trace::Range rendering("rendering");                                       // PathTracerApp.cpp:640

  pt_log::info_("Render started");
  // Nothing but the film ever has to leave the devices -- load balancing included: the balancer gets per-tile path-length
  // sums (kilobytes, pt_tile_costs) at the save intervals instead of the whole trace buffer every step.  The reference's
  // own loop (worklist to the host and back every step, per-item balancing) remains as --host-film, and serves the UI.
  if (args.flag("host-film") || args.u32("ui-port") != 0) executeHostFilm(steps);
  else executeResidentFilm(steps);

  auto endTime = std::chrono::steady_clock::now();
  const auto elapsedSecs = std::chrono::duration<double>(endTime - renderStartTime).count();
  pt_log::info_("Render finished: {} seconds", elapsedSecs);
  const std::size_t pixelsPerFrame = (std::size_t)imageWidth * imageHeight;
  finalSamplesPerSec = (pixelsPerFrame / elapsedSecs) * samplesPerPixel;   // PathTracerApp.cpp:786-789
  pt_log::info_("Samples/sec: {}", finalSamplesPerSec);
  pt_log::info_("Samples/sec/tile: {}", finalSamplesPerSec / ipuJobs.size());
}

void PathTracerApp::defunctState(std::uint32_t imageWidth, std::uint32_t imageHeight) {
  if (defunctTraceState) {
    defunctTraceState->film.reset();   // avoid reallocation: the worklists are large (PathTracerApp.cpp:512-515)
  } else {
    defunctTraceState.reset(new PathTracerState(imageWidth, imageHeight, traceState->work.getWork().active().size()));
  }
  // Swap and then copy the up-to-date work from the now defunct worklist:
  std::swap(traceState, defunctTraceState);
  traceState->work.getWork().active() = defunctTraceState->work.getWork().active();
  traceState->work.getWork().inactive() = defunctTraceState->work.getWork().active();
}

InterfaceServer::Status PathTracerApp::processUserInput(InterfaceServer::State& state, std::uint32_t imageWidth,
                                                        std::uint32_t imageHeight) {
  if (state.stop) {
    pt_log::info_("Rendering stopped by remote UI");
    return InterfaceServer::Status::Stop;
  }
  if (state.detach) {
    pt_log::info_("Remote UI disconnected.");   // the render just continues
    return InterfaceServer::Status::Disconnected;
  }
  if (!state.newNif.empty()) {
    pt_log::info_("Loading NIF: {}", state.newNif);
    if (loadNifModels(models.size(), state.newNif)) {
      // program init_nif_weights again (PathTracerApp.cpp:548-557): pt_upload_nif is re-callable
      for (std::size_t d = 0; d < devices.size(); ++d) models[d]->upload(devices[d]);
    }
  }
  defunctState(imageWidth, imageHeight);
  return InterfaceServer::Status::Restart;
}

void PathTracerApp::saveDenoisedAndFeatures(const std::string& fileName, std::size_t step, float exposure, float gamma, bool filmOnDevice) {
  if (!denoise && !saveFeatures) return;
  const std::size_t w = args.u32("width"), h = args.u32("height");
  const auto dot = fileName.find_last_of('.');
  const std::string base = fileName.substr(0, dot), ext = dot == std::string::npos ? std::string() : fileName.substr(dot);
  auto check = [&](int rc, const char* what) {
    if (rc) throw std::runtime_error(std::string(what) + " failed: " + pt_last_error(devices[0]));
  };
  if (denoise) {
    pt_trace::Range r("denoise");
    std::vector<float> out(w * h * 3);
    if (filmOnDevice) {
      check(pt_denoise(devices[0], &denoiseParams, PT_DENOISE_FILM, nullptr, out.data()), "pt_denoise");
    } else {
      Image3<float> host = traceState->film.getHdrImage();   // the running sum; the saved image is sum * (1 / step) (AccumulatedImage::saveImages)
      const float s = 1.f / step;
      for (auto& v : host.data) v *= s;
      check(pt_denoise(devices[0], &denoiseParams, PT_DENOISE_HOST_IMAGE, host.data.data(), out.data()), "pt_denoise");
    }
    image_io::writeExr(base + "_denoised.exr", out.data(), w, h);
    // tone-mapped as AccumulatedImage::updateLdrImage does the plain image
    std::vector<std::uint8_t> ldr(out.size());
    const float exposureScale = std::pow(2.f, exposure), invGamma = 1.f / gamma;
    for (std::size_t i = 0; i < out.size(); ++i) {
      const float v = std::pow(out[i] * exposureScale, invGamma) * 255.0f;
      ldr[i] = (std::uint8_t)std::min(255.0f, std::max(0.0f, std::nearbyint(v)));
    }
    image_io::writeLdr(base + "_denoised" + ext, ldr.data(), w, h);
    pt_log::info_("Saved denoised images at step {}", step);
  }
  if (saveFeatures) {
    std::vector<float> normal(w * h * 3), albedo(w * h * 3), depth(w * h), depth3(w * h * 3);
    pt_features f{};
    f.struct_size = sizeof(pt_features);
    f.normal = normal.data(); f.albedo = albedo.data(); f.depth = depth.data();
    check(pt_feature_buffers(devices[0], &f), "pt_feature_buffers");
    for (std::size_t i = 0; i < depth.size(); ++i) depth3[3 * i] = depth3[3 * i + 1] = depth3[3 * i + 2] = depth[i];
    image_io::writeExr(base + "_normal.exr", normal.data(), w, h);
    image_io::writeExr(base + "_albedo.exr", albedo.data(), w, h);
    image_io::writeExr(base + "_depth.exr", depth3.data(), w, h);
  }
}

void PathTracerApp::executeResidentFilm(std::uint32_t steps) {
  const auto imageWidth = args.u32("width"), imageHeight = args.u32("height");
  const float configExposure = args.f32("exposure"), configGamma = args.f32("gamma");
  const auto fileName = args.str("outfile");
  const auto saveInterval = args.u32("save-interval");
  const bool loadBalanceEnabled = args.flag("enable-load-balancing");
  pt_log::info_("Step loop: film resident on the device{}", devices.size() > 1 ? "s" : "");

  // program setup, once: every device gets its slice of the (shuffled) worklist -- pixel coordinates, zero accumulators --
  // and keeps it; with load balancing the slices are re-dealt at the save intervals (below)
  const auto& work = traceState->work.getWork().active();
  const std::size_t itemsPerDevice = work.size() / devices.size();
  const std::size_t slot = deviceCapacity;      // items per device incl. padding: equal on all devices (the gather's slot)
  const TraceRecord padding(std::numeric_limits<std::uint16_t>::max(), std::numeric_limits<std::uint16_t>::max());
  std::vector<RecordList> deviceWork(devices.size());
  for (std::size_t d = 0; d < devices.size(); ++d) {
    deviceWork[d].assign(work.begin() + d * itemsPerDevice, work.begin() + (d + 1) * itemsPerDevice);
    deviceWork[d].resize(slot, padding);
  }
  std::vector<float> tiles(devices.size() * slot * 3);   // rank 0 receives [device][slot][3] BGR film sums
  RecordList filmRecords;                                 // the gathered film as records AccumulatedImage::accumulate takes
  // Declared AFTER everything its job reads (filmRecords): if the step loop throws, unwinding destroys -- and so joins --
  // the task first, while those buffers are still alive.
  AsyncTask hostProcessing;
  onEveryDevice("setup", [&](std::size_t d) {
    pt_trace::Range r("setup");
    return pt_setup(devices[d], reinterpret_cast<const pt_trace_record*>(deviceWork[d].data()), slot);
  });
  const std::size_t nTiles = balanceTileCount(imageWidth, imageHeight);
  if (loadBalanceEnabled)
    onEveryDevice("tile costs", [&](std::size_t d) { return pt_tile_costs_enable(devices[d], kBalanceTile, kBalanceTile); });
  if (slot > itemsPerDevice)
    // padding items (u = v = 65535, LoadBalancer.cpp:66-71) are not traced (the reference's tiles trace
    // them and discard the result); the film and the tile costs skip them, Samples/sec and Rays/sec count image pixels only
    pt_log::info_("Load balancing: {} of {} work items per device are padding ({}%): room for any deal of {} image tiles", slot - itemsPerDevice,
                  slot, 100.0 * (double)(slot - itemsPerDevice) / (double)slot, nTiles);

  for (auto step = 1u; step <= steps; ++step) {
    auto loopStartTime = std::chrono::steady_clock::now();
    std::vector<pt_stats> stats(devices.size());
    std::vector<pt_nif_sharing_stats> share(devices.size(), sharingStatsRequest());
    std::vector<pt_nif_memo_stats> memo(devices.size(), memoStatsRequest());
    // path_trace, then on the device what the host task does in the reference's loop: film += (b,g,r)/sampleCount and
    // clear the accumulators (PathTracerApp.cpp:717-745)
    onEveryDevice("Device step", [&](std::size_t d) {
      int rc;
      { pt_trace::Range r("ipu_render"); rc = pt_path_trace(devices[d]) || pt_get_stats(devices[d], &stats[d]); }   // PathTracerApp.cpp:688-699
      if (rc) return rc;
      if ((rc = pt_get_nif_sharing_stats(devices[d], &share[d])) || (rc = pt_get_nif_memo_stats(devices[d], &memo[d]))) return rc;
      pt_trace::Range r("accumulate_framebuffers");                                                                // :725-727, on the device
      return pt_film_accumulate(devices[d]);
    });
    std::size_t totalRays = 0;
    for (auto& s : stats) totalRays += s.segments;    // what clearInactiveAccumulators sums (LoadBalancer.cpp:198-213)
    pt_log::debug_("Path-Trace ms: {}", stats[0].path_trace_ms);
    pt_log::debug_("NIF ms: {}", stats[0].nif_ms);
    pt_log::debug_("Total ms per step: {}", stats[0].total_ms);
    countNifEvaluations(share);
    countMemo(memo);

    if (step % saveInterval == 0 || step == steps) {
      logNifEvaluations();
      logMemo();
      { pt_trace::Range r("wait_for_host"); hostProcessing.waitForCompletion(); }   // the previous save still reads filmRecords (:702-706)
      // the ONE exchange of the multi-GPU path: HDR tiles to device 0 over RCCL, then to the host film
      // (--host-gather, or logical devices sharing a GPU: no communicator, every device hands its own tile to the host)
      onEveryDevice("HDR gather", [&](std::size_t d) {
        pt_trace::Range r("hdr_gather");
        if (hostGather) return pt_gather_hdr(devices[d], PT_HDR_FILM, slot, tiles.data() + d * slot * 3);
        return pt_gather_hdr(devices[d], PT_HDR_FILM, slot, d == 0 ? tiles.data() : nullptr);
      });
      filmRecords.clear();
      filmRecords.reserve(devices.size() * slot);
      for (std::size_t d = 0; d < devices.size(); ++d)
        for (std::size_t i = 0; i < slot; ++i) {
          TraceRecord r = deviceWork[d][i];
          const float* t = &tiles[(d * slot + i) * 3];
          r.b = t[0]; r.g = t[1]; r.r = t[2];
          r.sampleCount = 1;                  // accumulate() multiplies by 1 / sampleCount: the sums pass through
          filmRecords.push_back(r);
        }
      if (loadBalanceEnabled && step != steps) {
        // N3 without the worklist leaving the devices (LoadBalancer::allocateWorkByPathLength, LoadBalancer.cpp:141-192):
        // per-tile path-length sums from every device, tiles re-dealt by cost, and the film follows its pixels
        // (pt_film_seed), so every pixel's fp32 sum continues in step order: the image is bit-identical to the unbalanced one.
        pt_trace::Range balancing("run_load_balancing");                                                           // :748-751
        pt_log::info_("Load balancing started ({} image tiles over {} device{})", nTiles, devices.size(), devices.size() > 1 ? "s" : "");
        std::vector<std::vector<std::uint64_t>> part(devices.size(), std::vector<std::uint64_t>(nTiles));
        onEveryDevice("tile costs", [&](std::size_t d) { return pt_tile_costs(devices[d], part[d].data(), nTiles); });
        std::vector<std::uint64_t> cost(nTiles, 0);
        for (auto& p : part) for (std::size_t t = 0; t < nTiles; ++t) cost[t] += p[t];
        pt_log::debug_("Load balancing: {} bytes of tile costs from each device (the trace buffer is {} bytes)", nTiles * sizeof(std::uint64_t),
                       slot * sizeof(TraceRecord));
        const auto owner = dealTilesByPathLength(cost, devices.size());
        std::vector<float> running((std::size_t)imageWidth * imageHeight * 3, 0.f);   // the film so far, by pixel
        for (const auto& r : filmRecords)
          if (r.u < imageWidth && r.v < imageHeight) {
            float* p = &running[((std::size_t)r.v * imageWidth + r.u) * 3];
            p[0] = r.b; p[1] = r.g; p[2] = r.r;
          }
        std::vector<std::vector<float>> seed(devices.size());
        for (std::size_t d = 0; d < devices.size(); ++d) {
          deviceWork[d] = tileWorkList(imageWidth, imageHeight, owner, (std::int32_t)d, slot);
          seed[d].assign(slot * 3, 0.f);
          for (std::size_t i = 0; i < slot; ++i) {
            const auto& r = deviceWork[d][i];
            if (r.u < imageWidth && r.v < imageHeight)
              std::copy_n(&running[((std::size_t)r.v * imageWidth + r.u) * 3], 3, &seed[d][i * 3]);
          }
        }
        onEveryDevice("re-deal", [&](std::size_t d) {
          return pt_setup(devices[d], reinterpret_cast<const pt_trace_record*>(deviceWork[d].data()), slot) ||
                 pt_film_seed(devices[d], seed[d].data(), slot);
        });
        pt_log::info_("Load balancing finished");
      }
      hostProcessing.run([&, step]() {
        pt_trace::Range async("async_work");                                                                        // :718
        traceState->film.reset();
        traceState->film.accumulate(filmRecords);
        pt_trace::Range save("save_images");                                                                        // :761
        traceState->film.saveImages(fileName, step, configExposure, configGamma);   // hdr / step, as ever
        pt_log::info_("Saved images at step {}", step);
      });
      if (denoise || saveFeatures) {
        hostProcessing.waitForCompletion();   // the plain images first; the device calls below are made from this thread
        saveDenoisedAndFeatures(fileName, step, configExposure, configGamma, devices.size() == 1 && !loadBalanceEnabled);
      }
    }

    pt_trace::Range logging("log_stats");                                                                           // :765
    auto loopEndTime = std::chrono::steady_clock::now();
    auto secs = std::chrono::duration<double>(loopEndTime - loopStartTime).count();
    const auto pixelSamplesPerStep = (double)imageWidth * imageHeight * samplesPerIpuStep;
    pt_log::info_("Completed render step {}/{} in {} seconds (Samples/sec {}) (Rays/sec {})", step, steps, secs,
                  pixelSamplesPerStep / secs, totalRays / secs);
  }
  hostProcessing.waitForCompletion();
}

void PathTracerApp::executeHostFilm(std::uint32_t steps) {
  const auto imageWidth = args.u32("width"), imageHeight = args.u32("height");
  const auto fileName = args.str("outfile");
  const bool loadBalanceEnabled = args.flag("enable-load-balancing");
  const auto saveInterval = args.u32("save-interval");
  const auto seed = args.u64("seed");
  const float antiAliasingScale = args.f32("aa-noise-scale");
  std::atomic<std::size_t> totalRays{0};   // written by the host task, read by the step log
  const std::size_t itemsPerDevice = traceState->work.getWork().active().size() / devices.size();

  // Setup remote user interface (PathTracerApp.cpp:616-633):
  std::unique_ptr<InterfaceServer> uiServer;
  InterfaceServer::State state;
  state.exposure = args.f32("exposure");
  state.gamma = args.f32("gamma");
  state.fov = args.f32("fov") * (float)(M_PI / 180.f);
  state.envRotationDegrees = args.f32("env-map-rotation");
  state.interactiveSamples = args.u32("interactive-samples");
  if (const auto uiPort = args.u32("ui-port")) {
    uiServer.reset(new InterfaceServer((int)uiPort));
    uiServer->setInitialState(state);
    uiServer->start();
    uiServer->initialiseVideoStream(imageWidth, imageHeight);
  }
  // Declared AFTER the server, the state and the counter its job uses: if anything in the loop throws, unwinding joins
  // the task (its destructor) before the InterfaceServer it talks to is destroyed.
  AsyncTask hostProcessing;
  pt_log::info_("Step loop: the reference's (worklist to the host and back every step, host film)");
  constexpr std::size_t sampleCountReversionStep = 5;
  std::uint32_t lastStep = 0;   // steps accumulated into the current film
  auto sendRenderSettings = [&]() {   // program init_render_settings (PathTracerApp.cpp:678-686)
    const float radians = (state.envRotationDegrees / 360.f) * (float)(2.0 * M_PI);
    for (auto h : devices)
      check(h, pt_set_render_settings(h, seed, antiAliasingScale, state.fov, radians, samplesPerIpuStep), "init_render_settings");
  };

  for (auto step = 1u; step <= steps; ++step) {
    auto loopStartTime = std::chrono::steady_clock::now();

    // Do the simple thing and restart the entire render if any state changed (PathTracerApp.cpp:656-676):
    if (uiServer && uiServer->stateChanged()) {
      pt_trace::Range r("ui_processing");                                     // PathTracerApp.cpp:653
      state = uiServer->consumeState();
      const auto status = processUserInput(state, imageWidth, imageHeight);
      // (the previous step's host task may still be sending to the client: join it before the server goes away -- the
      // reference resets the server while that task can still be running)
      if (status == InterfaceServer::Status::Stop) {
        hostProcessing.waitForCompletion();
        uiServer.reset();
        break;
      }
      if (status == InterfaceServer::Status::Disconnected) {
        hostProcessing.waitForCompletion();
        uiServer.reset();
      } else if (status == InterfaceServer::Status::Restart) {
        renderStartTime = loopStartTime;   // the final Samples/sec counts from the restart (:669)
        step = 1;
        samplesPerIpuStep = state.interactiveSamples;
      }
    } else {
      // (no `uiServer &&` here, as in the reference: a client that restarts the render and then detaches or closes must
      // not leave the device on the interactive sample count for the rest of the run)
      if (step == sampleCountReversionStep) {
        // No UI input for a few steps so revert to performant number of samples:
        samplesPerIpuStep = args.u32("samples-per-step");
        pt_log::debug_("Interaction stopped reverting samples per step to: {}", samplesPerIpuStep);
      }
    }
    // Render settings can only be updated on these steps (:678-686), server or no server:
    if (step == 1 || step == sampleCountReversionStep) { pt_trace::Range r("update_ipu_settings"); sendRenderSettings(); }

    // setup -> path_trace -> read_results on every device (PathTracerApp.cpp:692-694).  The worklist is
    // cut into equal contiguous slices, one per device, as tiles are cut over IPUs.
    auto& active = traceState->work.getWork().active();
    std::vector<pt_stats> stats(devices.size());
    std::vector<pt_nif_sharing_stats> share(devices.size(), sharingStatsRequest());
    std::vector<pt_nif_memo_stats> memo(devices.size(), memoStatsRequest());
    onEveryDevice("Device step", [&](std::size_t d) {
      auto* slice = reinterpret_cast<pt_trace_record*>(active.data() + d * itemsPerDevice);
      pt_handle h = devices[d];
      pt_trace::Range r("ipu_render");                                        // :688-699
      return pt_setup(h, slice, itemsPerDevice) || pt_path_trace(h) || pt_read_results(h, slice, itemsPerDevice, &stats[d]) ||
             pt_get_nif_sharing_stats(h, &share[d]) || pt_get_nif_memo_stats(h, &memo[d]);
    });
    countNifEvaluations(share);
    countMemo(memo);
    if (step % saveInterval == 0 || step == steps) { logNifEvaluations(); logMemo(); }
    pt_log::debug_("Path-Trace ms: {}", stats[0].path_trace_ms);
    pt_log::debug_("NIF ms: {}", stats[0].nif_ms);
    pt_log::debug_("Total ms per step: {}", stats[0].total_ms);
    pt_log::debug_("Step {} took {} samples per pixel from sample index {}", step, samplesPerIpuStep, stats[0].first_sample);   // (pt_stats.paths counts real pixels only: not padding)

    const auto deviceDone = std::chrono::steady_clock::now();
    { pt_trace::Range r("wait_for_host"); hostProcessing.waitForCompletion(); }   // join the previous async task before swapping (:703-708)
    traceState->work.getWork().swap();
    pt_log::debug_("Device calls (setup + path_trace + read_results) wall ms: {}",
                   std::chrono::duration<double, std::milli>(deviceDone - loopStartTime).count());
    pt_log::debug_("Waited for host film task ms: {}",
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - deviceDone).count());

    // The work list and film are captured by pointer: user interaction may make them defunct while this runs (:717)
    hostProcessing.run([&, step, workPtr = &traceState->work, filmPtr = &traceState->film]() {
      pt_trace::Range async("async_work");                                    // :718
      { pt_trace::Range r("accumulate_framebuffers"); filmPtr->accumulate(workPtr->getWork().inactive()); }   // :725-727
      if (uiServer) {
        const auto ui = uiServer->getState();
        {
          pt_trace::Range r("tone_map");                                      // :732-734 (+ ui_encode_video: the preview is sent as text here)
          uiServer->sendPreviewImage(filmPtr->updateLdrImage(step, ui.exposure, ui.gamma));
        }
        pt_trace::Range r("ui_send_events");                                  // :738
        uiServer->updateProgress((int)step, (int)steps);
      }
      if (loadBalanceEnabled && step > 1) { pt_trace::Range r("run_load_balancing"); workPtr->allocateWorkByPathLength(ipuJobs); }   // :748-751
      { pt_trace::Range r("clear_accumulators"); totalRays = workPtr->clearInactiveAccumulators(); }                                   // :753-755
      if (step % saveInterval == 0 || step == steps) {
        if (uiServer) {
          // with a UI attached the raw image is transmitted at the save interval instead of saved (:748-753)
          uiServer->startSendingRawImage(filmPtr->getHdrImage(), step);
        } else {
          pt_trace::Range r("save_images");                                   // :761
          filmPtr->saveImages(fileName, step, state.exposure, state.gamma);
          pt_log::info_("Saved images at step {}", step);
        }
      }
    });
    if ((denoise || saveFeatures) && !uiServer && (step % saveInterval == 0 || step == steps)) {
      hostProcessing.waitForCompletion();   // the host film of this step is complete and saved; device calls are made from this thread
      saveDenoisedAndFeatures(fileName, step, state.exposure, state.gamma, false);
    }

    auto loopEndTime = std::chrono::steady_clock::now();
    auto secs = std::chrono::duration<double>(loopEndTime - loopStartTime).count();
    const auto pixelSamplesPerStep = (double)imageWidth * imageHeight * samplesPerIpuStep;
    pt_log::info_("Completed render step {}/{} in {} seconds (Samples/sec {}) (Rays/sec {})", step, steps, secs,
                  pixelSamplesPerStep / secs, totalRays.load() / secs);
    if (uiServer) uiServer->updateSampleRate((float)(pixelSamplesPerStep / secs), (float)(totalRays.load() / secs));
    lastStep = step;
  }
  hostProcessing.waitForCompletion();
  if (args.u32("ui-port") != 0 && lastStep) {
    // the film the client saw last is also left on disk, so an interactive session ends with an image like a batch run
    traceState->film.saveImages(fileName, lastStep, state.exposure, state.gamma);
    pt_log::info_("Saved images at step {}", lastStep);
  }
}
