// Application object: reference src/PathTracerApp.hpp:36-57.  init() / execute() / addToolOptions() keep
// their roles; build() (Poplar graph construction) has no counterpart -- the device program is libptmi.so.
#pragma once
#include <chrono>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "AccumulatedImage.hpp"
#include "EnvMapReader.hpp"
#include "ObjReader.hpp"
#include "InterfaceServer.hpp"
#include "IpuPathTraceJob.hpp"
#include "LoadBalancer.hpp"
#include "NifModel.hpp"
#include "Options.hpp"
#include "ptmi.h"

struct PathTracerState {
  PathTracerState(std::uint32_t imageWidth, std::uint32_t imageHeight, std::size_t workItems)
      : work(workItems), film(imageWidth, imageHeight) {}
  LoadBalancer work;
  AccumulatedImage film;
};

/// --scene: the "texture" of a mesh -- the image as EnvMapReader read it and the two modes (pt_set_mesh_texture); the texture
/// coordinates travel in the mesh (objreader::Mesh::uvs, uv_indices).
struct SceneTexture {
  env_map::Image image;
  std::int32_t filter = PT_TEX_FILTER_BILINEAR, wrap = PT_TEX_WRAP_REPEAT;
};

struct PathTracerApp {
  PathTracerApp();
  virtual ~PathTracerApp();

  /// All initialisation that needs no device (PathTracerApp.cpp:60-72).
  void init(const OptionMap& args);
  /// Acquire the GPU(s) and upload constants: what GraphManager::run + build() do before execute().
  void attach();
  /// The host step loop (PathTracerApp.cpp:566-792).
  void execute();
  /// The 25 tool options of PathTracerApp.cpp:794-830 plus the 8 standard ones of main.cpp:8-37.
  static std::vector<OptionSpec> addToolOptions();

  double samplesPerSecond() const { return finalSamplesPerSec; }

private:
  bool loadNifModels(std::size_t numDevices, const std::string& assetPath);
  pt_env_guide envGuideRequest(const std::string& size, float alpha);
  pt_env_guide_auto envGuideAutoRequest(const std::string& size, float alpha, std::uint32_t supersample);
  void initialiseState(std::uint32_t imageWidth, std::uint32_t imageHeight);
  /// One call on every device, each from its own thread (devices run concurrently and exchange no ray data,
  /// PathTracerApp.cpp:205-252); throws with the first device's message on failure.
  template <class F> void onEveryDevice(const char* what, F&& call);
  /// Step loop with the film resident on the devices: path_trace + pt_film_accumulate per step, one RCCL gather of HDR
  /// tiles to device 0 at every save interval.
  void executeResidentFilm(std::uint32_t steps);
  /// User interaction invalidates all rendering in progress: new (or recycled) tracer state is swapped in and the up-to-date
  /// worklist copied over, so nobody waits for the defunct host task (PathTracerApp.cpp:507-528).
  void defunctState(std::uint32_t imageWidth, std::uint32_t imageHeight);
  /// PathTracerApp.cpp:530-564: stop / detach / NIF hot-reload + restart.
  InterfaceServer::Status processUserInput(InterfaceServer::State& state, std::uint32_t imageWidth, std::uint32_t imageHeight);
  /// Step loop as the reference runs it (setup -> path_trace -> read_results, host film): needed when the balancer
  /// re-deals the worklist from the returned path lengths every step.
  void executeHostFilm(std::uint32_t steps);
  /// --share-nif-evaluations: NIF rows executed against escaped paths, summed over the devices and logged at save intervals.
  static pt_nif_sharing_stats sharingStatsRequest();
  void countNifEvaluations(const std::vector<pt_nif_sharing_stats>& share);
  void logNifEvaluations();
  /// --nif-memo-gib: escaped paths served by the memo and NIF rows executed, summed over the devices, logged at save intervals.
  static pt_nif_memo_stats memoStatsRequest();
  void countMemo(const std::vector<pt_nif_memo_stats>& memo);
  void logMemo();
  /// --denoise / --save-features: at a save, after the plain images are on disk (which stay as they are, byte for byte), write
  /// <basename>_denoised.exr and _denoised<ext> (pt_denoise on device 0: the resident film when `filmOnDevice`, else the host
  /// film / step as PT_DENOISE_HOST_IMAGE) and <basename>_normal.exr, _albedo.exr, _depth.exr (pt_feature_buffers).  Called
  /// from the thread that drives the devices, with no host task running.
  void saveDenoisedAndFeatures(const std::string& fileName, std::size_t step, float exposure, float gamma, bool filmOnDevice);

  OptionMap args;
  std::uint32_t samplesPerPixel = 0;
  std::uint32_t samplesPerIpuStep = 0;
  IpuJobList ipuJobs;
  DeviceGeometry geometry;
  std::vector<pt_handle> devices;
  std::vector<std::unique_ptr<NifModel>> models;
  std::unique_ptr<PathTracerState> traceState;
  std::unique_ptr<PathTracerState> defunctTraceState;   // keeps defunct data alive while the async host task finishes on it
  std::size_t deviceCapacity = 0;   // work items per device incl. padding (pt_config.max_work_items)
  bool hostGather = false;   ///< HDR tiles through the host (one copy per device) instead of the RCCL gather
  double finalSamplesPerSec = 0.0;
  std::int32_t nifSharing = PT_NIF_SHARE_OFF;
  std::int32_t meshBuilder = PT_MESH_BUILDER_HOST;   ///< --mesh-builder: who builds the meshes' trees (pt_set_mesh_build)
  std::int32_t meshDeviceTree = PT_MESH_DEVICE_TREE_LINEAR;   ///< --mesh-device-tree: which tree the device builder builds (pt_set_mesh_device_tree)
  std::uint64_t nifEscaped = 0, nifEvaluations = 0;
  std::uint64_t nifMemo = 0;   ///< --nif-memo-gib in bytes per logical device, 0 = off
  std::uint64_t memoServed = 0, memoEscaped = 0, memoRows = 0;
  std::vector<pt_scene_object> scene;   ///< --scene: the table every handle renders (empty: the built-in scene)
  std::vector<pt_scene_object_ex> sceneEx;   ///< --scene: the same with vertices, when the file holds a polygon (else empty)
  std::vector<objreader::Mesh> sceneMeshes;   ///< --scene: the meshes of the file's "mesh" objects, in the order of their rows
  std::vector<SceneTexture> sceneTextures;    ///< --scene: one per mesh, in the same order (an empty image: the mesh has no texture)
  pt_camera camera{};                   ///< --scene: the file's "camera", set on every handle when hasCamera
  env_map::Image envMap;                ///< --env-map: the image every handle takes as its environment (empty: NIF or constant)
  std::int32_t envMapFilterMode = 1;    ///< --env-map-filter (PT_ENV_FILTER_*)
  env_map::Image envGuide;              ///< --env-guide: the image every handle's diffuse bounces are guided by (empty: unguided; "map": envMap is used)
  bool envGuideFromMap = false;         ///< --env-guide map
  bool envGuideFromEnv = false;         ///< --env-guide env: no image, the library builds the guide from the environment in force
  std::uint32_t envGuideSupersample = 2; ///< --env-guide-supersample
  std::uint32_t envGuideRows = 0, envGuideCols = 0;   ///< --env-guide-size (default: the largest powers of two that fit)
  float envGuideAlpha = 0.5f;           ///< --env-guide-alpha
  float lightGuideBeta = 0.f;           ///< --light-guide-beta (0 = off)
  bool lightGuidePolygons = false;      ///< --light-guide-polygons: draw from emissive triangles and parallelograms too
  bool hasCamera = false;
  bool denoise = false, saveFeatures = false;   ///< --denoise, --save-features
  pt_denoise_params denoiseParams{};            ///< --denoise-iterations / -sigma-colour / -sigma-normal / -sigma-depth over the library's defaults
  std::chrono::steady_clock::time_point renderStartTime;   // reset when the UI restarts the render (PathTracerApp.cpp:669)
};

std::size_t roundSamplesPerPixel(std::size_t samplesPerPixel, std::size_t samplesPerIpuStep);
