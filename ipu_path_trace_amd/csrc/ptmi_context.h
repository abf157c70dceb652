// ptmi_context.h -- the owners of device and pinned memory, per-handle state (pt_context), error helpers, trace parameters
// Part of the one translation unit ptmi.hip (host side of include/ptmi.h); included there, in this order:
// ptmi_step_plan.h, ptmi_context.h, ptmi_probe.h, ptmi_nif_pack.h, ptmi_nif_launch.h, [ptmi.hip: the entry points, with
// ptmi_nif_group.h among the stages of a step], ptmi_mesh_api.h, ptmi_film_comm.h, ptmi_denoise.h, ptmi_nif_train.h.
#pragma once

using ptplan::TraceGrid;
using ptplan::trace_grid;
using ptplan::item_divider;

namespace {

thread_local std::string g_create_error;

// ---- binary16 helpers on the host (weights arrive as raw fp16 bytes)
inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

uint16_t host_f2h(float f) {
  uint32_t x = f2u(f), sign = (x >> 16) & 0x8000u, ax = x & 0x7fffffffu;
  if (ax >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | ((ax > 0x7f800000u) ? 0x200u : 0u));
  if (ax >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);
  if (ax < 0x33000001u) return (uint16_t)sign;
  int e = (int)(ax >> 23) - 127;
  uint32_t m = (ax & 0x7fffffu) | 0x800000u, shift, hexp;
  if (e < -14) { shift = (uint32_t)(13 + (-14 - e)); hexp = 0; } else { shift = 13; hexp = (uint32_t)(e + 15); }
  uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), halfway = 1u << (shift - 1);
  if (rem > halfway || (rem == halfway && (q & 1u))) q += 1u;
  uint32_t h = hexp == 0 ? q : ((hexp - 1u) << 10) + q;
  return (uint16_t)(sign | h);
}

float host_h2f(uint16_t h) {
  uint32_t sign = ((uint32_t)h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  if (e == 0) {
    if (m == 0) return u2f(sign);
    float v = (float)m * 5.9604644775390625e-08f;
    return sign ? -v : v;
  }
  if (e == 31) return u2f(sign | 0x7f800000u | (m << 13));
  return u2f(sign | ((e + 112u) << 23) | (m << 13));
}

inline float host_hround(float f) { return host_h2f(host_f2h(f)); }

// Move-only owner of `count` elements of device memory (DevBuf) or of pinned host memory (PinnedBuf).  It converts to T*, so
// kernel arguments, parameter structs and pointer arithmetic read as with a raw pointer.  Every buffer of a handle is one of
// these, a member of pt_context: deleting the handle frees them, and that is the only place (pt_destroy makes the device
// current and drains the streams first).  release() gives the allocation up without freeing it.
template <typename T, bool kPinned>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : n_(o.n_), p_(o.release()) {}
  Buf& operator=(Buf&& o) noexcept {   // (deletes the copy operations)
    if (this != &o) { reset(); n_ = o.n_; p_ = o.release(); }
    return *this;
  }
  ~Buf() { reset(); }
  // frees what it held first; empty on failure
  hipError_t alloc(size_t count) {
    reset();
    void* p = nullptr;
    const hipError_t e = kPinned ? hipHostMalloc(&p, count * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, count * sizeof(T));
    if (e == hipSuccess) { p_ = static_cast<T*>(p); n_ = count; }
    return e;
  }
  void reset() { if (T* p = release()) (void)(kPinned ? hipHostFree(p) : hipFree(p)); }
  T* release() { n_ = 0; return std::exchange(p_, nullptr); }
  size_t count() const { return n_; }
  operator T*() const { return p_; }

 private:
  size_t n_ = 0;
  T* p_ = nullptr;
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinnedBuf = Buf<T, true>;

struct HostLayer {
  uint32_t rows, cols;
  std::vector<uint16_t> kernel;  // [rows][cols]
  std::vector<uint16_t> bias;    // [cols] or empty
  bool relu;
};

// Everything pt_nif_train_begin makes (ptmi_nif_train.h): parameters, the target image, master weights, Adam moments, the
// per-layer input buffers and gradients.  One object, owned by the handle: pt_nif_train_end (or a new begin, or pt_destroy)
// drops it and every DevBuf in it frees itself.
struct NifTrainState {
  pt_nif_train_params p{};
  struct Layer { uint32_t rows, cols, relu; size_t w_off, b_off; };   // offsets into the parameter blob: kernel, then bias
  std::vector<Layer> layers;
  size_t n_params = 0;
  uint32_t map_w = 0, map_h = 0, skip = 0;
  float mean[3] = {0, 0, 0}, max = 0;
  uint64_t step = 0;
  DevBuf<float4> d_target;                  // [map_h][map_w] (t_b, t_g, t_r, 0)
  DevBuf<float> d_w, d_g, d_m, d_v;         // parameter blob, its gradient, Adam moments
  DevBuf<float> d_u, d_vv, d_t;             // the batch: u, v [batch], target [batch][3]
  std::vector<DevBuf<float>> d_act;         // d_act[l]: input of layer l, [batch][rows_l]
  DevBuf<float> d_y;                        // head output [batch][3]
  DevBuf<float> d_dz[2];                    // gradient w.r.t. a layer's pre-activation, ping-pong, [batch][hidden]
  DevBuf<float> d_partial;                  // [kTrainSlabs][largest rows x cols + cols]
  size_t partial_stride = 0;
  DevBuf<double> d_red;                     // kTrainStatBlocks x 3 partials of the statistics / the loss
  DevBuf<float> d_enc;                      // mean0..2, max, then the loss
  DevBuf<uint16_t> d_half;                  // the blob rounded to binary16 (export)
  DevBuf<uint32_t> d_overflow;              // [layers]

  // mixed precision (pt_nif_train_set_precision): everything below is empty in PT_NIF_TRAIN_F32, the mode begin starts in
  pt_nif_train_precision prec{};            // the mode in force and its initial scale, dynamic, growth_interval
  struct Layer16 { uint32_t ldx, ldw, ldt; size_t w16_off, w16t_off; };   // leading dimensions in halves: input, w16, w16^T
  std::vector<Layer16> layers16;
  std::vector<DevBuf<uint16_t>> d_act16;    // d_act16[l]: input of layer l, [batch][ldx_l], padding zero
  DevBuf<uint16_t> d_dz16[2];               // hidden gradients, ping-pong, [batch][hidden]
  DevBuf<uint16_t> d_dzh16;                 // the head's gradient, [batch][32], columns 3.. zero
  DevBuf<uint16_t> d_w16, d_w16t;           // half(w) per layer as [rows][ldw] and [cols][ldt], padding zero
  DevBuf<ptd::TrainCtl> d_ctl;              // the control block
};

}  // namespace

struct pt_context {
  pt_config cfg{};
  std::string error;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int n_cus = 256;

  // worklist
  uint32_t n_items = 0;
  uint32_t capacity = 0;
  DevBuf<ptd::TraceRecordDev> d_records;
  ptd::Accum acc{};                          // device-visible: raw pointers into the six owners below
  DevBuf<uint32_t> d_acc_pix, d_acc_count, d_acc_length;
  DevBuf<float> d_acc_r, d_acc_g, d_acc_b;
  uint32_t n_real = 0;                       // work items that are not padding (u < width and v < height: AccumulatedImage.cpp:66)
  DevBuf<unsigned long long> d_counters;     // [0] segments, [1] escaped or emitter paths, [2] real items (pt_setup), [3] emitter paths
  PinnedBuf<unsigned long long> h_counters;  // the same in pinned host memory: copied on the stream at the end of a step (no blocking hipMemcpy)

  // batch buffers, a ring of kBatchSets sets (ptmi_step_plan.h: ring_slot): the trace kernel of batch b+1 runs on
  // `trace_stream` while the NIF kernel of batch b (MFMA-bound) runs on `stream`, and a third set keeps a batch's trip
  // N -> E -> A -> T -> S -> N from setting the pace of the step
  uint32_t iters_per_batch = 1;
  uint32_t first_batch_iters = 1;   // iterations of a step's first batch (see enqueue_path_trace)
  size_t batch_paths_cap = 0;
  size_t queue_cap = 0;
  // Grid of the persistent trace kernel: six workgroups per CU (1536 on an MI355X).  Measured, scripts/sweep_trace_blocks.py:
  // 9.1 ms per 331 M-path step for 1280...1536 workgroups against 10.2 for 1600...2048 (the grid of rounds 1-3), the C2 step
  // unchanged -- the 60-VGPR / 106-SGPR kernel is resident six-fold per CU, not eight-fold as
  // hipOccupancyMaxActiveBlocksPerMultiprocessor reports, so a larger grid runs its last workgroups on part of the chip.
  static constexpr int kTraceBlocksPerCu = 6;
  static constexpr uint32_t kBatchSets = 3;
  // Bytes of batch buffers per path of batch capacity: in every set, per path plen 1 + rad 12 and per queue slot (one per
  // path, rounded up per region) q_* 24; once per handle, per queue slot, survivor note 16 + path state 48.
  static constexpr uint64_t kBatchBytesPerPath = kBatchSets * (1 + 12 + 24) + 16 + 48;
  uint32_t trace_blocks = 1536;
  uint32_t ring_depth = kBatchSets;    // sets a step cycles through; the profiling build can lower it (PTMI_BATCH_SETS)
  // Scratch of the trace kernel, written and read inside one launch (pt_trace.h).  The trace launches of a handle follow each
  // other on one stream, so one copy serves every set.
  DevBuf<uint4> d_survivors;           // primary-phase notes of the trace kernel, one region per trace workgroup
  DevBuf<float4> d_states;             // path states after the first shading, three planes of queue_cap float4
  struct BatchBuffers {
    DevBuf<float> q_u, q_v, q_tr, q_tg, q_tb;
    DevBuf<uint32_t> q_path;
    DevBuf<uint32_t> region_count;
    DevBuf<uint8_t> plen;
    DevBuf<float> rad_r, rad_g, rad_b;
    hipEvent_t traced = nullptr;       // trace kernel of the batch using this set has finished
    hipEvent_t accumulated = nullptr;  // accumulate kernel has consumed this set
    hipEvent_t raw_read = nullptr;     // (mapped step) the raw-pair pass R(b) has read the set's q_u / q_v
    // geometry of the last batch whose NIF stage ran on this set (pt_calibrate_nif replays the larger one): 0 = none yet
    uint32_t last_paths = 0, last_regions = 0, last_region_cap = 0;
    // ... and, if that batch ran with sharing on, where its distinct queue lies: count index (-1 = not shared), store base
    int32_t share_batch = -1;
    uint32_t share_base = 0, share_region_cap = 0;
  } bb[kBatchSets];
  hipStream_t trace_stream = nullptr;
  hipStream_t acc_stream = nullptr;   // accumulate(b) runs here, so NIF(b+1) follows NIF(b) back to back on `stream`
  bool serial = false;   // profiling build only: trace kernels share the NIF stream

  // render settings
  bool settings_valid = false;
  uint64_t seed = 0;
  float aa_scale = 0, fov = 0, azimuth = 0;
  uint32_t samples_per_step = 0;
  uint32_t sample_cursor = 0;  // absolute index of the next sample iteration

  // scene (pt_set_scene): the table in force, stored normalised; scene_n = 0: the built-in scene (pt_trace.h::scene_const)
  pt_scene_object scene[PT_MAX_SCENE_OBJECTS] = {};
  uint32_t scene_n = 0;
  // ... and, for a table given through pt_set_scene_ex, the polygons' vertices (a polygon's row above holds centre = v0,
  // radius = 0 and its normal); scene_poly: the table holds a polygon, the POLY kernel instances run
  float scene_vertex[PT_MAX_SCENE_OBJECTS][3][3] = {};
  bool scene_poly = false;
  // ... and, for a table given through pt_set_scene_meshes, the meshes (ptmi_mesh.h; a mesh's row above holds shape 4 and zeros).
  // scene_mesh: the table holds a mesh, the MESH kernel instances run.  The device buffers are sized once, for 2 T - 1 nodes per
  // mesh; a new camera pose rebuilds the trees into them from the host copy of the world-space frames (ensure_meshes).
  bool scene_mesh = false;
  struct MeshSet {
    struct One {
      uint32_t object_index, n_triangles, tri_base, node_base, n_nodes, max_leaf, depth;
      float pad;
      double build_ms;
      // vertex normals (pt_set_mesh_normals): the world normals per corner in triangle order, nine floats per triangle; empty: flat
      uint32_t n_vertices, n_normals;
      bool per_corner;
      std::vector<float> normals;
      std::vector<uint32_t> normal_indices;   // the caller's [n_triangles][3] when per_corner (pt_update_mesh_vertices looks new normals up by them)
      // pt_update_mesh_vertices wrote this mesh's frames / corner normals on the device: its part of `world` / `normals` on the
      // host is stale until refresh_mesh_host copies it back
      bool world_stale = false, normals_stale = false;
      // texture (pt_set_mesh_texture): the (s, t) per corner in triangle order, six floats per triangle; empty: no texture
      uint32_t n_uvs = 0, tex_w = 0, tex_h = 0;
      int32_t tex_filter = 0, tex_wrap = 0;
      bool uv_per_corner = false;
      std::vector<float> uvs;
    };
    std::vector<One> mesh;                 // in declaration order
    size_t triangles() const { size_t t = 0; for (const One& m : mesh) t += m.n_triangles; return t; }   // of all meshes
    std::vector<float> world;              // twelve floats per triangle (v0, e1, e2, n), the meshes one after the other
    DevBuf<ptmesh::Node> d_nodes;          // mesh m at node_base = sum over the meshes before it of 2 T - 1
    DevBuf<ptmesh::F4> d_tris;             // three per slot, mesh m's slots from tri_base
    DevBuf<uint32_t> d_orig;               // slot -> triangle index in its mesh
    std::vector<uint32_t> indices;         // the meshes' own [n_triangles][3], one after the other: per-vertex normals are looked up by them
    DevBuf<ptmesh::F4> d_normals;          // three per slot over ALL slots, allocated by the first pt_set_mesh_normals of the scene
    bool smooth() const { for (const One& m : mesh) if (!m.normals.empty()) return true; return false; }
    DevBuf<float> d_uvs;                   // six per slot over ALL slots, allocated by the first pt_set_mesh_texture of the scene
    DevBuf<ptmesh::TexDesc> d_desc;        // one per scene row (PT_MAX_SCENE_OBJECTS), allocated with d_uvs; desc: its host copy
    std::vector<DevBuf<ptmesh::F4>> d_texels;   // mesh m's own image, (B, G, R, 0) per texel; one entry per mesh once a texture was attached
    ptmesh::TexDesc desc[PT_MAX_SCENE_OBJECTS] = {};
    bool textured() const { for (const One& m : mesh) if (!m.uvs.empty()) return true; return false; }
    ptd::PolyEdges row[PT_MAX_SCENE_OBJECTS] = {};   // what a mesh's row carries in the kernel arguments (ptd::MeshRow)
    bool built = false, built_world = false;         // the trees on the device are valid / were built in the world frame ...
    ptcamera::Basis built_for{};                     // ... or for this camera
    // pt_set_mesh_build (ptmi_mesh_build.h): what the device builder and the refit need, allocated while a device option is set
    // and sized for the largest mesh -- empty for a handle that never sets one
    struct DeviceBuild {
      DevBuf<float> world;                           // the world frames, twelve floats per triangle, as `world` above
      DevBuf<float> corner, corner_uv;               // world corner normals (nine per triangle) / uvs (six), triangle order, over ALL triangles
      DevBuf<uint64_t> code[2];                      // Morton codes before / after the sort
      DevBuf<uint32_t> index[2];                     // triangle indices before / after the sort
      DevBuf<uint32_t> words;                        // ptlbvh::Scratch (kScratchWords per key) and the centroids' bounds
      DevBuf<uint32_t> stats;                        // ptlbvh::kStats words per mesh: n_nodes, depth, max_leaf, pad
      DevBuf<uint8_t> sort_tmp;                      // the radix sort's temporary storage
      size_t cap = 0;                                // triangles of the largest mesh
      uint64_t bytes = 0;
      // pt_set_mesh_device_tree (ptmi_mesh_sah.h): the SAH builder's arrays (ptsah::Work) for the largest mesh, allocated while
      // the kind is PT_MESH_DEVICE_TREE_SAH under a device option
      DevBuf<uint32_t> sah_words;
      uint64_t sah_bytes = 0;
    } dev;
    int topo_builder = -1;                           // the builder whose topology lies on the device for these triangles (-1: none a refit may use)
    int topo_kind = 0;                               // ... and, for the device builder, the kind of tree (PT_MESH_DEVICE_TREE_*)
    // pt_update_mesh_vertices (ptmi_mesh_update.h): allocated by the first update of the scene, beside `dev` -- empty for a
    // handle that never updates a mesh
    struct Update {
      DevBuf<uint32_t> indices;                      // the meshes' own [n_triangles][3], one after the other, as `indices` above
      DevBuf<float> vertices;                        // staging: the new vertices of the mesh being updated (cap_vertices x 3)
      DevBuf<uint32_t> normal_indices;               // [n_triangles][3] over ALL triangles; a per-corner mesh's part is filled
      DevBuf<float> normals;                         // staging: the new normals (cap_normals x 3)
      DevBuf<uint64_t> fault;                        // two words: the first fault among the frames / among the normals
      size_t cap_vertices = 0, cap_normals = 0;
      uint64_t bytes = 0;                            // of the above, and of what an update had ensure_mesh_device add to `dev`
    } upd;
  } mesh;
  // pt_update_mesh_vertices: counters since pt_create, and the last update's times
  uint64_t mesh_updates = 0, mesh_update_refits = 0, mesh_update_rebuilds = 0, mesh_update_fallbacks = 0;
  int32_t mesh_update_last_kind = 0;
  double mesh_update_frames_ms = 0, mesh_update_tree_ms = 0;
  hipEvent_t mesh_update_event[2] = {nullptr, nullptr};   // start / stop of an update's frames on `stream`
  // pt_set_mesh_build: the options belong to the handle and outlive the scene
  int32_t mesh_builder = 0, mesh_on_pose = 0;        // PT_MESH_BUILDER_HOST, PT_MESH_POSE_REBUILD
  uint64_t mesh_host_builds = 0, mesh_device_builds = 0, mesh_refits = 0;
  int32_t mesh_last_kind = 0;
  double mesh_last_ms = 0;
  hipEvent_t mesh_event[2] = {nullptr, nullptr};     // start / stop of one mesh's device work on `stream`
  // pt_set_mesh_device_tree: which tree the device builder builds; belongs to the handle like the options above
  int32_t mesh_device_tree = 0;                      // PT_MESH_DEVICE_TREE_LINEAR
  uint64_t mesh_sah_builds = 0;
  uint32_t mesh_sah_last_levels = 0;
  double mesh_sah_last_ms = 0;

  // pt_get_trace_variant: what the selector picked at the last launch of each kernel family, written at the launch sites
  pt_trace_variant_launch variant_trace{-1, -1, -1, -1, 0}, variant_paths{-1, -1, -1, -1, 0}, variant_features{-1, -1, -1, -1, 0};

  // camera (pt_set_camera): the values as given, and the frame made from them once (ptmi_camera.h)
  pt_camera camera = ptcamera::default_camera();
  ptcamera::Basis camera_basis = ptcamera::basis(ptcamera::default_camera());

  // environment
  bool env_const = false;
  float env_rgb[3] = {0, 0, 0};
  // HDR environment map (pt_set_env_map, pt_envmap.h): the third kind; the last of the three calls wins
  bool env_map = false;
  DevBuf<float4> d_env_texels;       // [env_h][env_w] (B, G, R, 0), row-major
  uint32_t env_w = 0, env_h = 0;
  int32_t env_filter = 0;
  // environment guide (pt_set_env_guide, pt_env_guide.h): sampling, not light -- it outlives every change of environment
  bool guide_set = false;
  ptd::GuideParams guide{};          // device-visible: raw pointers into the two owners below (all zero without a guide)
  DevBuf<uint2> d_guide_alias;       // [rows * cols] {threshold, alias}
  DevBuf<float> d_guide_q;           // [rows * cols]
  float guide_alpha = 0.f;           // alpha as given (the sum check of pt_set_light_guide)
  // ... built from the environment in force (pt_set_env_guide_from_environment, pt_env_guide_build.h) instead of an image
  bool guide_from_env = false;       // the tables in force came from the environment
  uint32_t guide_supersample = 0;    // S of that build (0: from an image)
  bool guide_follow = false;         // rebuild when the environment is replaced
  bool guide_stale = false;          // the last such rebuild failed: the tables follow an earlier environment
  uint64_t guide_rebuilds = 0, guide_clamped = 0;
  double guide_build_ms = 0;
  // emitter guide (pt_set_light_guide, pt_light_guide.h): host data alone, rebuilt with the scene; it travels in the kernel arguments
  bool light_set = false;
  float light_beta = 0.f;            // beta as given
  uint32_t light_flags = 0;          // pt_set_light_guide_ex: PT_LIGHT_GUIDE_POLYGONS lists emissive polygons in the table
  ptlight::Table light{};
  bool nif_valid = false;
  int nif_hidden = 0, nif_emb = 0;   // PADDED hidden width / embedding dimension the kernels are instantiated for
  bool nif_gemm = false;  // layer-by-layer path (pt_nif_gemm.h)
  // float32 models (pt_nif_f32.h): padded row-major kernels and biases of all layers in one buffer, chunk buffers
  bool nif_f32 = false;
  struct F32Layer { size_t w_off, b_off; uint32_t k_act, k_in, ldw, relu, half_out, cast_half; };
  std::vector<F32Layer> f32_layers;
  DevBuf<float> d_f32_weights, d_f32_act[2], d_f32_feat;
  uint32_t f32_chunk = 0, f32_lda = 0, f32_ldf = 0;
  DevBuf<float4> d_head_partial;      // fused head: [2 FB][chunk samples] partial sums
  DevBuf<float4> d_head_in;           // head weights of the Fourier-feature inputs [4][E], if the head concatenates them
  float head_bias[3] = {0, 0, 0};
  uint32_t head_piece_base = 0;
  ptd::NifParams nif{};
  DevBuf<uint4> d_wpack, d_bpack;
  uint64_t nif_flops = 0;
  std::string nif_kernel;   // what launch_nif dispatched last (pt_nif_kernel_name): the bench line quotes the library, not a guess
  // layer-by-layer path of the wide networks (pt_nif_gemm.h): activation ping-pong and feature pieces of one chunk
  DevBuf<uint4> d_gemm_act[2], d_gemm_feat;
  DevBuf<uint32_t> d_tile_start;
  uint32_t gemm_chunk = 0;   // 32-sample tiles per chunk (multiple of 8); 0 = path not set up
  // The layer-by-layer paths run the chunks of a queue round-robin on the NIF stream and on extra ones (chunk_stream):
  // chunks are independent, so one chunk's layer launch fills the CUs another's is draining (the ramp / drain / gap of a
  // launch is ~3-4 % of a 240 us layer).  Every chunk buffer therefore exists kChunkSets times (set s at offset s x *_set).
  static constexpr int kChunkSets = 2;                  // chunks in flight (C5: 1 -> 2 streams +2.7 % on one box, 0 on another; 3: -1 %)
  hipStream_t chunk_stream[kChunkSets - 1] = {};        // sets 1.. (set 0 runs on the NIF stream itself)
  hipEvent_t chunk_fork = nullptr, chunk_join[kChunkSets - 1] = {};
  int chunk_sets = kChunkSets;                           // profiling build: PTMI_CHUNK_STREAMS lowers it for the A/B
  size_t gemm_act_set = 0, gemm_feat_set = 0, head_partial_set = 0;   // uint4 / uint4 / float4 elements per set
  size_t f32_act_set = 0, f32_feat_set = 0;                            // floats per set
  DevBuf<unsigned long long> d_stamps;      // profiling build: 256 phase stamps of the wide-NIF layer kernel
  int diag_fault_batch = -1;                // test build: batch whose NIF launch fails (pt_diag_inject_fault), -1 = none

  // NIF sharing and the memo (ptmi_nif_group.h; kernels: pt_nif_group.h, pt_nif_memo.h)
  struct NifGroup {
    // exact sharing of NIF evaluations (pt_set_nif_sharing).  No key survives a step: the table is cleared at the start
    // of every batch (PT_NIF_SHARE_BATCH) or, for PT_NIF_SHARE_STEP, at the end of the step before (share_clean_slots says
    // so) or else at the start of the step; the counts at every step.
    int32_t share_mode = 0;                    // requested: taken up by the next pt_path_trace
    bool share_mode_set = false;               // pt_set_nif_sharing or pt_set_nif_memo was called; until then the step chooses (auto_share_mode)
    bool share_auto_failed = false;            // the automatic default could not allocate: off until pt_set_nif_sharing
    int32_t share_mode_last = 0;               // what the last pt_path_trace ran with (0 also for a constant environment)
    DevBuf<unsigned long long> d_share_keys;
    DevBuf<uint32_t> d_share_vals;
    uint32_t share_slots = 0;                  // table capacity, a power of two
    uint32_t share_clean_slots = 0;            // the clean-table mark (ptmi_share_plan.h): slots at which the table is known to hold no key, 0 = not known
    uint32_t share_diag_slots = 0;             // test build: forced capacity (pt_diag_set_nif_share_capacity), 0 = sized from memory
    DevBuf<uint32_t> d_share_owner[kBatchSets];        // per batch-buffer set: [queue_cap] owner word of every entry (ptmi_share_plan.h)
    // the step's distinct queues and their decoded BGR, region-structured: batch b's at store region (b, or at batch scope its set) x queue_cap
    DevBuf<float> d_share_u, d_share_v, d_share_bgr;
    size_t share_regions = 0;
    DevBuf<uint32_t> d_share_count;            // [batch] distinct-queue length
    DevBuf<unsigned long long> d_share_over;
    PinnedBuf<uint32_t> h_share_count;         // pinned copies, written at the end of the step on `stream`
    PinnedBuf<unsigned long long> h_share_over;
    size_t share_count_cap = 0;
    uint64_t share_evals = 0, share_overflowed = 0;
    double share_ms = 0;

    // the class level of the NIF stage (pt_nif_group.h: ClassTable): whenever N(b) runs over a distinct queue of a NIF, it
    // evaluates one row per class of the kernels' encoder input.  The table and the class store live for one pt_path_trace,
    // whatever the sharing mode: cleared at the start of every step, batch b's class queue at region b.  If the buffers do
    // not fit (ptshare::class_fits) or an allocation fails, the handle runs without the level: the same bytes, no error.
    DevBuf<unsigned long long> d_class_keys;
    DevBuf<uint32_t> d_class_vals;
    uint32_t class_slots = 0;                  // table capacity, a power of two
    uint32_t class_diag_slots = 0;             // test build: forced capacity (pt_diag_set_nif_class_capacity), 0 = sized by the rule
    DevBuf<uint32_t> d_class_owner;            // [queue_cap]: class-store index of the owner of every entry of the distinct queue in flight (the memo's steps; a fused step keeps class-store indices in d_share_owner and the raw table's values)
    DevBuf<float> d_class_u, d_class_v, d_class_bgr;   // class queues and their decoded BGR: class_regions x queue_cap
    size_t class_regions = 0;
    DevBuf<uint32_t> d_class_count;            // [batch] class-queue length
    DevBuf<unsigned long long> d_class_over;   // rows evaluated alone
    PinnedBuf<uint32_t> h_class_count;         // pinned copies, written at the end of the step on `stream`
    PinnedBuf<unsigned long long> h_class_over;
    size_t class_count_cap = 0;
    bool class_failed = false;                 // an allocation failed: no class level on this handle from now on
    bool class_ran = false;                    // the last pt_path_trace ran the level
    uint64_t class_rows = 0, class_alone = 0;
    double class_ms = 0;
    // The class map of a mapped step (ptmi_share_plan.h; pt_nif_group.h: ClassMap): kClassMapWords words and the tail's values
    // behind them, and the tail's keys.  Allocated by the first step that may take it (ptshare::class_map_fits), set to kMapEmpty
    // once and released row by row at the end of every step that used it; class_map_clean is the mark of that (map_mark_after_step).
    DevBuf<uint32_t> d_class_map;
    DevBuf<unsigned long long> d_class_tail_keys;
    uint32_t class_tail_slots = 0;             // 0 = no map held
    bool class_map_clean = false;
    bool class_map_failed = false;             // its allocation failed: the hashed class table from now on
    bool class_map_ran = false;                // the last pt_path_trace was a mapped step
    uint32_t expand_launches = 0;              // E(b) launches of the last pt_path_trace (0 where A(b) expands: StepMode::expand_in_accumulate)

    // persistent memo of decoded NIF values (pt_set_nif_memo).  Unlike the sharing table it outlives the step:
    // it is cleared at allocation, on a new generation (pt_upload_nif, pt_clear_nif_memo, a failed pt_path_trace) and by the
    // retain pass.  With the memo on, every step uses the step-scope store above (d_share_u / _v / _bgr, d_share_count).
    DevBuf<ptd::MemoSlot> d_memo;
    uint32_t memo_slots = 0;                   // table capacity, a power of two; 0 = memo off
    DevBuf<ptd::MemoSlot> d_memo_list;         // retain list, memo_slots / 2 entries
    DevBuf<uint32_t> d_memo_slot;              // [store index]: slot the entry is published into (memo_slot_regions x queue_cap)
    size_t memo_slot_regions = 0;
    DevBuf<unsigned long long> d_memo_ctr;     // ptd::kMemoCounters counters of the memo passes
    PinnedBuf<unsigned long long> h_memo_ctr;  // pinned copy, written at the end of the step on `stream` (the step's one wait)
    bool memo_clear = false;                   // clear the table before the next lookup
    uint32_t memo_step = 0;                    // stamp of the last step that ran the memo passes
    bool memo_ran = false;                     // the last pt_path_trace ran them
    uint64_t memo_occupied = 0, memo_served = 0, memo_inserted = 0, memo_generation = 0, memo_retains = 0;
    double memo_ms = 0;
  } group;

  // stats.  The per-stage times are read lazily (pt_get_stats / pt_read_results): 3 hipEventElapsedTime calls per batch are
  // host time a step of a small image should not pay (BASELINE configs[0] is one millisecond of device work per step).
  pt_stats stats{};
  std::vector<hipEvent_t> events;
  enum SpanKind { kSpanNone = -1, kSpanTrace, kSpanNif, kSpanAccumulate, kSpanShare, kSpanMemo, kSpanClass };
  struct StageSpan { size_t a, b; int kind; };   // event pair (indices into `events`) around one stage of one batch
  std::vector<StageSpan> spans;
  size_t e_begin_i = 0, e_end_i = 0;
  bool spans_pending = false;

  // scratch for the standalone entry points
  DevBuf<char> d_scratch;   // grows on demand (ensure_scratch)

  // NIF trainer (pt_nif_train_begin .. pt_nif_train_end, ptmi_nif_train.h): null without one
  std::unique_ptr<NifTrainState> train;

  // first-hit feature cache and the denoiser's dense frames (pt_feature_buffers / pt_denoise; pt_features.h, pt_denoise.h):
  // allocated on first use, width x height float4 each (64 bytes per pixel in all)
  DevBuf<float4> d_feat[2];        // f0 = (normal, depth), f1 = (albedo BGR, object index bits)
  DevBuf<float4> d_dn_colour[2];   // colour ping-pong
  uint64_t feature_gen = 1;                      // bumped by pt_set_scene, pt_set_camera, pt_set_render_settings
  uint64_t feature_cached_gen = 0;               // generation d_feat holds (0: none)
  // A-trous iterations whose step is at most this stage their taps in LDS, the others read global memory (measured:
  // profiles/r11_denoise.txt); the profiling build can move it (pt_diag_denoise_bench)
  uint32_t denoise_tiled_max_step = 2;

  // multi-GPU film hand-off: RCCL communicator (one rank per handle) and the HDR tile buffers
  ncclComm_t comm = nullptr;
  std::shared_ptr<ptw::BoundedWorker> comm_worker;   // the long-lived thread that makes the handle's RCCL calls (ptmi_comm_worker.h): created with the first communicator call, dropped when a call never returns
  int comm_rank = 0, comm_world = 1;
  bool comm_broken = false;                  // the communicator was aborted (deadline, peer failure, pt_comm_abort): gathers fail until a new one is made
  std::atomic<bool> comm_abort_req{false};   // pt_comm_abort from another thread: the polling loops see it and abort
  uint32_t comm_timeout_ms = 120000;         // deadline of every communicator operation (pt_comm_set_timeout)
  size_t comm_slot_agreed = 0;               // slot_items value every rank of the communicator is known to use
  DevBuf<long long> d_slot_check;            // {slot, -slot} for the agreement all-reduce
  DevBuf<float> d_film;            // resident film: [capacity][3] BGR, sum over steps of the per-step means
  ptd::TileGrid tiles{};           // per-tile path-length sums for the balancer (pt_tile_costs_enable), n_tiles = 0: off
  DevBuf<unsigned long long> d_tile_cost;     // owns tiles.cost (the struct is device-visible: it keeps the raw pointer)
  DevBuf<unsigned long long> d_tile_tmp;      // tracked sums + current accumulators, staged for the copy to the host
  uint32_t film_steps = 0;
  DevBuf<float> d_hdr_stage;       // this rank's tile: [slot_items][3] mean BGR, zero padded
  DevBuf<float> d_hdr_gather;      // root only: [world][slot_items][3]
};

namespace {

inline int hip_status(hipError_t e);

#define PT_HIP(call)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      h->error = std::string(#call) + ": " + hipGetErrorString(e_);                          \
      return hip_status(e_);                                                                 \
    }                                                                                        \
  } while (0)

// A failed allocation is its own status (include/ptmi.h): the caller can retry with a smaller max_work_items.
inline int hip_status(hipError_t e) {
  if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return PT_ERR_OUT_OF_MEMORY; }   // not sticky: clear it for the next call
  return PT_ERR_HIP;
}

int fail(pt_handle h, int code, const std::string& msg) {
  h->error = msg;
  return code;
}

// The pt_get_*_info entry points' check of their output: null, or a struct of another size than this library's.
template <class Info>
int check_info(pt_handle h, const Info* out, const char* who) {
  if (out && out->struct_size == sizeof(Info)) return PT_OK;
  return fail(h, PT_ERR_INVALID_ARGUMENT, std::string(who) + ": struct_size must be " + std::to_string(sizeof(Info)));
}

// (a name for Buf::alloc that an error message quotes: PT_HIP(dev_alloc(h->d_film, n)) reads "dev_alloc(h->d_film, n): ...")
template <typename T, bool kPinned>
hipError_t dev_alloc(Buf<T, kPinned>& b, size_t count) { return b.alloc(count); }

int ensure_scratch(pt_handle h, size_t bytes) {
  if (bytes <= h->d_scratch.count()) return PT_OK;
  PT_HIP(dev_alloc(h->d_scratch, bytes));
  return PT_OK;
}
template <typename T>
T* scratch_as(pt_handle h) { return reinterpret_cast<T*>(static_cast<char*>(h->d_scratch)); }

// The built-in scene (src/codelets/codelets.cpp:111-144) as a pt_scene_object table: ONE source, the kernels' compile-time
// table pt_trace.h::scene_const.  A disc's normal (0, 1, 0) is already normalised (n / sqrtf(dot(n, n)) leaves it as it is).
static_assert(ptd::kMaxObjects == PT_MAX_SCENE_OBJECTS && ptd::MAT_EMISSIVE == PT_MATERIAL_EMISSIVE, "scene capacity / materials");
static_assert(sizeof(pt_scene_object) == 48, "pt_scene_object layout");
static_assert(sizeof(pt_scene_object_ex) == 84 && sizeof(ptd::PolyEdges) == 24 && ptd::SHAPE_TRIANGLE == PT_SHAPE_TRIANGLE &&
              ptd::SHAPE_PARALLELOGRAM == PT_SHAPE_PARALLELOGRAM, "pt_scene_object_ex layout / shape codes");
void builtin_scene(pt_scene_object (&out)[ptd::kBuiltinObjects]) {
  for (int i = 0; i < ptd::kBuiltinObjects; ++i) {
    const ptd::SceneConst S = ptd::scene_const(i);
    out[i] = pt_scene_object{S.disc ? PT_SHAPE_DISC : PT_SHAPE_SPHERE, S.type, {S.cx, S.cy, S.cz}, S.radius,
                             {S.nx, S.ny, S.nz}, {S.colr, S.colg, S.colb}};
  }
}

// Scene constants of a table of n objects (the built-in one or pt_set_scene's) into the kernel arguments: the SAME
// expressions for every table, so the built-in table passed through pt_set_scene is bit-identical to no call.
// The kernels trace in camera space: with a camera other than the built-in one (cam != nullptr) a centre enters as
// R^T (c - position) and a disc normal as R^T n, and the expressions below run on those values.  The built-in camera applies
// no transform at all (not a multiplication by the identity), so "no camera set" is the same bits by construction.
// A polygon (vertex != nullptr: the vertices of pt_set_scene_ex's table) enters with v0 as its centre, a point, and its edges
// e1, e2 (formed in world space in binary32, as the validation forms them) and stored normal as directions.
// A mesh row (mesh_row != nullptr: pt_set_scene_meshes) carries its shape code and, in its edges' slot, where its tree lies.
void fill_scene(ptd::TraceParams& P, const pt_scene_object* src, uint32_t n, const ptcamera::Basis* cam = nullptr,
                const float (*vertex)[3][3] = nullptr, const ptd::PolyEdges* mesh_row = nullptr) {
  P.n_objects = n;
  for (uint32_t i = 0; i < n; ++i) {
    ptd::SceneObject& o = P.obj[i];
    const bool disc = src[i].shape == PT_SHAPE_DISC;
    const bool poly = vertex && ptscene::is_polygon(src[i].shape);
    const bool mesh = mesh_row && src[i].shape == PT_SHAPE_MESH;
    if (mesh) P.poly[i] = mesh_row[i];
    float centre[3] = {src[i].centre[0], src[i].centre[1], src[i].centre[2]};
    float normal[3] = {src[i].normal[0], src[i].normal[1], src[i].normal[2]};
    if (cam) {
      ptcamera::to_camera_point(*cam, src[i].centre, centre);
      if (disc || poly) ptcamera::to_camera_direction(*cam, src[i].normal, normal);
    }
    if (poly) {
      const ptscene::PolyFrame f = ptscene::poly_frame(vertex[i]);
      float e1[3] = {f.e1[0], f.e1[1], f.e1[2]}, e2[3] = {f.e2[0], f.e2[1], f.e2[2]};
      if (cam) {
        ptcamera::to_camera_direction(*cam, f.e1, e1);
        ptcamera::to_camera_direction(*cam, f.e2, e2);
      }
      P.poly[i] = ptd::PolyEdges{e1[0], e1[1], e1[2], e2[0], e2[1], e2[2]};
    }
    o.cx = centre[0]; o.cy = centre[1]; o.cz = centre[2];
    // (a polygon: S = |e1 x e2| as formed in world space, for the polygon-lamp instances alone; r2 and c4 stay those of radius 0)
    o.radius = poly ? ptlight::poly_area_s(vertex[i]) : src[i].radius;
    o.r2 = src[i].radius * src[i].radius;
    o.nx = normal[0]; o.ny = normal[1]; o.nz = normal[2];
    o.colr = src[i].colour[0]; o.colg = src[i].colour[1]; o.colb = src[i].colour[2];
    o.type = src[i].material;
    o.is_disc = (poly || mesh) ? src[i].shape : (disc ? 1 : 0);   // the shape code
    // constants of a ray that starts at the origin, by the device's own expressions (this file is compiled with
    // -ffp-contract=off like the kernels; volatile keeps every intermediate a rounded binary32 whatever the host's FLT_EVAL_METHOD)
    volatile float ox = 0.f - o.cx, oy = 0.f - o.cy, oz = 0.f - o.cz;          // sub(o, c)
    volatile float xx = ox * ox, yy = oy * oy, zz = oz * oz;
    volatile float d0 = xx + yy, d1 = d0 + zz;                                 // dot(oc, oc), left to right
    volatile float cc = d1 - o.r2;
    o.ocx = ox; o.ocy = oy; o.ocz = oz;
    o.c4 = 4.0f * cc;
    volatile float kx = (o.cx - 0.f) * o.nx, ky = (o.cy - 0.f) * o.ny, kz = (o.cz - 0.f) * o.nz;   // dot(sub(c, o), n)
    volatile float k0 = kx + ky, k1 = k0 + kz;
    o.kdisc = k1;
    o.same_centre = (i > 0 && !disc && !poly && !mesh && src[i - 1].shape == PT_SHAPE_SPHERE && src[i].centre[0] == src[i - 1].centre[0] &&
                     src[i].centre[1] == src[i - 1].centre[1] && src[i].centre[2] == src[i - 1].centre[2]) ? 1 : 0;
  }
}

// ---- meshes (pt_set_scene_meshes): the trees on the device

void bind_meshes(pt_handle h, ptd::TraceParams& P) {
  P.mesh_nodes = h->mesh.d_nodes;
  P.mesh_tris = h->mesh.d_tris;
  P.mesh_orig = h->mesh.d_orig;
  P.mesh_normals = h->mesh.d_normals;
}
// The TEX instances' second argument (pt_set_mesh_texture): valid while h->mesh.textured()
ptd::TexParams tex_params(pt_handle h) { return ptd::TexParams{h->mesh.d_uvs, h->mesh.d_desc}; }

// The host copies of what pt_update_mesh_vertices wrote on the device (ptmi_mesh_update.h): a stale mesh's frames and corner
// normals come back with one copy each, before anything on the host reads them.
int refresh_mesh_host(pt_handle h, pt_context::MeshSet& M) {
  for (pt_context::MeshSet::One& m : M.mesh) {
    if (m.world_stale) {
      PT_HIP(hipMemcpy(M.world.data() + ptmesh::kFrameFloats * (size_t)m.tri_base, M.dev.world + ptmesh::kFrameFloats * (size_t)m.tri_base,
                       ptmesh::kFrameFloats * (size_t)m.n_triangles * sizeof(float), hipMemcpyDeviceToHost));
      m.world_stale = false;
    }
    if (m.normals_stale) {
      PT_HIP(hipMemcpy(m.normals.data(), M.dev.corner + 9 * (size_t)m.tri_base, m.normals.size() * sizeof(float), hipMemcpyDeviceToHost));
      m.normals_stale = false;
    }
  }
  return PT_OK;
}

// The host builder's scratch, kept over the meshes of one pass.
struct MeshHostScratch {
  std::vector<float> frames, uvs;
  std::vector<ptmesh::F4> normals;
  ptmesh::Built B;
};

// Mesh m of M into the frame of `cam`: its tree built on the host and copied, with its triangles, normals and uvs in the new slot
// order, into M's device buffers, which hold any tree of these triangles (2 T - 1 nodes): no allocation on the device.
int build_mesh_host(pt_handle h, pt_context::MeshSet& M, pt_context::MeshSet::One& m, const ptcamera::Basis* cam, MeshHostScratch& X) {
  ptmesh::Built& B = X.B;
  const auto t0 = std::chrono::steady_clock::now();
  X.frames.resize(ptmesh::kFrameFloats * (size_t)m.n_triangles);
  ptmesh::kernel_frames(M.world.data() + ptmesh::kFrameFloats * (size_t)m.tri_base, m.n_triangles, cam, X.frames.data());
  ptmesh::build(X.frames.data(), m.n_triangles, B);
  m.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  m.n_nodes = (uint32_t)B.nodes.size();
  m.max_leaf = B.max_leaf; m.depth = B.depth; m.pad = B.pad;
  if (B.nodes.size() > 2 * (size_t)m.n_triangles - 1 || B.orig.size() != m.n_triangles)
    return fail(h, PT_ERR_HIP, "mesh builder: a tree larger than its buffer");   // (cannot happen: a binary tree with non-empty leaves)
  PT_HIP(hipMemcpy(M.d_nodes + m.node_base, B.nodes.data(), B.nodes.size() * sizeof(ptmesh::Node), hipMemcpyHostToDevice));
  PT_HIP(hipMemcpy(M.d_tris + 3 * (size_t)m.tri_base, B.tris.data(), B.tris.size() * sizeof(ptmesh::F4), hipMemcpyHostToDevice));
  PT_HIP(hipMemcpy(M.d_orig + m.tri_base, B.orig.data(), B.orig.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  if (!m.normals.empty()) {   // the corner normals into the new slot order (the buffer exists: pt_set_mesh_normals)
    X.normals.resize(3 * (size_t)m.n_triangles);
    ptmesh::slot_normals(m.normals.data(), B.orig.data(), m.n_triangles, cam, X.normals.data());
    PT_HIP(hipMemcpy(M.d_normals + 3 * (size_t)m.tri_base, X.normals.data(), X.normals.size() * sizeof(ptmesh::F4), hipMemcpyHostToDevice));
  }
  if (!m.uvs.empty()) {   // the corner uvs into the new slot order, untransformed (the buffer exists: pt_set_mesh_texture)
    X.uvs.resize(6 * (size_t)m.n_triangles);
    ptmesh::slot_uvs(m.uvs.data(), B.orig.data(), m.n_triangles, X.uvs.data());
    PT_HIP(hipMemcpy(M.d_uvs + 6 * (size_t)m.tri_base, X.uvs.data(), X.uvs.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  const ptd::MeshRow row{m.node_base, m.tri_base, m.n_nodes, m.n_triangles, m.normals.empty() ? 0u : 1u, m.uvs.empty() ? 0u : 1u};
  memcpy(&M.row[m.object_index], &row, sizeof(row));
  return PT_OK;
}

// Transforms every mesh of M into the frame of `cam` (nullptr: the world frame, which is the built-in camera's), builds its tree
// and copies trees and triangles into M's device buffers.  The handle's streams are drained first: a step in flight may still
// read the buffers.
int build_meshes(pt_handle h, pt_context::MeshSet& M, const ptcamera::Basis* cam) try {
  PT_HIP(hipSetDevice(h->cfg.device));
  if (&M == &h->mesh)   // (a set that is not in force yet has no reader)
    for (hipStream_t s : {h->stream, h->trace_stream, h->acc_stream})
      if (s) PT_HIP(hipStreamSynchronize(s));
  M.built = false;
  M.topo_builder = -1;
  if (int rc = refresh_mesh_host(h, M)) return rc;
  MeshHostScratch X;
  double total_ms = 0;
  for (pt_context::MeshSet::One& m : M.mesh) {
    if (int rc = build_mesh_host(h, M, m, cam, X)) return rc;
    total_ms += m.build_ms;
  }
  M.built = true;
  M.built_world = cam == nullptr;
  if (cam) M.built_for = *cam;
  M.topo_builder = PT_MESH_BUILDER_HOST;
  h->mesh_host_builds += 1;
  h->mesh_last_kind = PT_MESH_LAST_HOST_BUILD;
  h->mesh_last_ms = total_ms;
  return PT_OK;
} catch (const std::bad_alloc&) {   // the builder's host arrays: the trees stay marked stale, the next call tries again
  return fail(h, PT_ERR_OUT_OF_MEMORY, "meshes: out of host memory while building the trees");
}

}  // (namespace: ptmi_mesh_build.h opens its own)
#include "ptmi_mesh_build.h"
namespace {

// The trees of M for the frame of `cam`, by the options in force (pt_set_mesh_build): a refit where trees of these triangles by
// the builder in force (and, on the device, of the kind in force) lie on the device and only the frame changes, else a build by
// that builder.
int update_meshes(pt_handle h, pt_context::MeshSet& M, const ptcamera::Basis* cam) {
  if (h->mesh_on_pose == PT_MESH_POSE_REFIT && mesh_topology_in_force(h, M) && M.dev.world) return refit_meshes(h, M, cam);
  if (h->mesh_builder == PT_MESH_BUILDER_DEVICE) return build_meshes_device(h, M, cam);
  return build_meshes(h, M, cam);
}

}  // (namespace: ptmi_mesh_update.h opens its own)
#include "ptmi_mesh_update.h"
namespace {

// Before anything traces a mesh scene: the trees follow the camera in force (world = true, pt_mesh_intersect: the world frame).
int ensure_meshes(pt_handle h, bool world = false) {
  if (!h->scene_n || !h->scene_mesh) return PT_OK;
  const ptcamera::Basis& cb = h->camera_basis;
  const ptcamera::Basis* cam = (world || cb.identity) ? nullptr : &cb;
  pt_context::MeshSet& M = h->mesh;
  const auto same = [](const ptcamera::Basis& a, const ptcamera::Basis& b) {
    return !memcmp(a.r, b.r, sizeof a.r) && !memcmp(a.u, b.u, sizeof a.u) && !memcmp(a.f, b.f, sizeof a.f) &&
           !memcmp(a.position, b.position, sizeof a.position);
  };
  if (M.built && (cam ? (!M.built_world && same(M.built_for, *cam)) : M.built_world)) return PT_OK;
  return update_meshes(h, M, cam);
}

// The emitter guide's table into the kernel arguments.  P.lights.n stays 0 -- no light-guided instance is launched -- unless a
// guide is set, has an emitter with mass and beta > 0 (beta = 0 is the mixture without the light branch: the other instances'
// arithmetic exactly).  The hooks (hook = true) take the table whatever beta is.
void fill_light_params(pt_handle h, ptd::TraceParams& P, bool hook = false) {
  const ptlight::Table& T = h->light;
  if (!h->light_set || !T.active() || (!hook && T.beta_thr == 0u)) return;
  ptd::LightParams& L = P.lights;
  L.n = T.n_draw;
  L.beta_thr = T.beta_thr;
  L.beta = (float)T.beta;
  L.one_minus = (float)(1.0 - ((double)P.guide.alpha_thr + (double)T.beta_thr) / ptlight::kTwo32);
  for (uint32_t k = 0; k < T.n_draw; ++k) {
    L.index[k] = T.object_index[k];
    L.threshold[k] = T.threshold[k];
    L.probability[k] = T.probability[k];
  }
}

void fill_trace_params(pt_handle h, ptd::TraceParams& P) {
  memset(&P, 0, sizeof(P));
  const ptcamera::Basis& cb = h->camera_basis;
  const ptcamera::Basis* cam = cb.identity ? nullptr : &cb;
  if (h->scene_n) {
    fill_scene(P, h->scene, h->scene_n, cam, h->scene_poly ? h->scene_vertex : nullptr, h->scene_mesh ? h->mesh.row : nullptr);
    if (h->scene_mesh) bind_meshes(h, P);
  } else {
    pt_scene_object builtin[ptd::kBuiltinObjects];
    builtin_scene(builtin);
    fill_scene(P, builtin, ptd::kBuiltinObjects, cam);
  }
  P.cam_pose = cam ? 1 : 0;
  for (int k = 0; k < 3; ++k) { P.cam_r[k] = cb.r[k]; P.cam_u[k] = cb.u[k]; P.cam_f[k] = cb.f[k]; }
  P.lens_a = h->camera.lens_radius;
  P.lens_f = h->camera.lens_radius > 0.f ? h->camera.focus_distance : 0.f;
  const pt_config& c = h->cfg;
  const float w = (float)c.width, hgt = (float)c.height;
  const float fov = host_hround(h->fov);        // field_of_view stream is half (PathTracerApp.cpp:591)
  P.width_f = w;
  P.height_f = hgt;
  P.width = c.width;
  P.height = c.height;
  P.tx = tanf(fov * 0.5f);                      // light::pixelToRay (INFERRED: DESIGN.md, camera model)
  P.ty = (hgt / w) * P.tx;
  P.aa_scale = host_hround(h->aa_scale);        // anti_alias_scale stream is half (:590)
  P.stop_prob = host_hround(c.stop_prob);       // IpuPathTraceJob.cpp:137
  P.rr_factor = 1.0f / (1.0f - P.stop_prob);
  P.ri = host_hround(c.refractive_index);       // IpuPathTraceJob.cpp:133
  P.azimuth = h->azimuth;
  P.seed_lo = (uint32_t)h->seed;
  P.seed_hi = (uint32_t)(h->seed >> 32);
  P.max_path_length = c.max_path_length;
  P.roulette_depth = c.roulette_depth;
  P.aa_type = c.aa_noise_type;
  P.samples_half = (c.sample_precision == PT_SAMPLES_HALF);
  P.env_const = h->env_const ? 1 : 0;
  P.env_r = h->env_rgb[0]; P.env_g = h->env_rgb[1]; P.env_b = h->env_rgb[2];
  P.pix = h->acc.pix;
  P.emitted = h->d_counters + 3;
  P.state_stride = h->queue_cap;
  P.guide = h->guide;
  fill_light_params(h, P);
  item_divider(h->n_items ? h->n_items : 1u, P.div_magic, P.div_shift);
}

void bind_batch(pt_handle h, ptd::TraceParams& P, const pt_context::BatchBuffers& B) {
  P.q_u = B.q_u; P.q_v = B.q_v; P.q_tr = B.q_tr; P.q_tg = B.q_tg; P.q_tb = B.q_tb; P.q_path = B.q_path;
  P.region_count = B.region_count;
  P.survivors = h->d_survivors;
  P.states = h->d_states;
  P.plen = B.plen;
  P.rad_r = B.rad_r; P.rad_g = B.rad_g; P.rad_b = B.rad_b;
}

}  // namespace
