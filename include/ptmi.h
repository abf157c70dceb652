/*
 * ptmi.h -- C-ABI of the MI355X path-trace hot path (libptmi.so).
 *
 * Drop-in boundary for markp-gc/ipu_path_trace: each entry point replaces one of the five
 * named Poplar programs / named data streams that PathTracerApp::execute() drives
 * (reference: src/PathTracerApp.cpp:479-483 registers the programs, src/ipu_utils.hpp:288-373
 * StreamableTensor is the stream mechanism).  Plain pointers and sizes only; no C++ or torch
 * types cross this boundary.  All functions return 0 on success and a negative pt_status
 * otherwise; pt_last_error() returns the message (the reference throws std::runtime_error /
 * std::logic_error which GraphManager::run catches once, src/ipu_utils.hpp:532-535 -- the C++
 * shim in ipu_path_trace_amd/host re-throws from these codes).
 *
 * Threading (as the reference, PathTracerApp.cpp:692-709): calls on one handle are made from one
 * thread, strictly setup -> path_trace -> read_results; the library copies from / to the host
 * buffers synchronously and retains no host pointer after returning.
 */
#ifndef PTMI_H
#define PTMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTMI_ABI_VERSION 5

typedef struct pt_context* pt_handle;

/* Wire format of the `trace_buffer` stream: src/codelets/TraceRecord.hpp:7-19
 * (20 bytes; offsets 0/2/4/8/12/16/18).  Padding items carry u = v = 65535
 * (src/LoadBalancer.cpp:66-71).  The reference's tiles trace them like any other item and the film skips them
 * (src/AccumulatedImage.cpp:66); here an item with u >= width or v >= height is NOT traced: its sampleCount advances, its
 * r, g, b and pathLength do not, and pt_stats counts image pixels only. */
typedef struct pt_trace_record {
  uint16_t u, v;
  float r, g, b;
  uint16_t sampleCount;
  uint16_t pathLength;
} pt_trace_record;

enum pt_status {
  PT_OK = 0,
  PT_ERR_INVALID_ARGUMENT = -1,
  PT_ERR_NO_DEVICE = -2,
  PT_ERR_HIP = -3,
  PT_ERR_UNSUPPORTED_MODEL = -4,
  PT_ERR_NOT_READY = -5,
  PT_ERR_OUT_OF_MEMORY = -6,
  PT_ERR_COMM = -7
};

enum { PT_AA_NORMAL = 0, PT_AA_UNIFORM = 1, PT_AA_TRUNCATED_NORMAL = 2 }; /* PathTracerApp.cpp:29-45 */
enum { PT_SAMPLES_HALF = 0, PT_SAMPLES_FLOAT = 1 };                        /* PathTracerApp.cpp:297 */
enum { PT_DTYPE_F16 = 0, PT_DTYPE_F32 = 1 };                                  /* Hdf5Model.cpp:109-133 */

/* Compile-time parameters of the reference graph: the CLI options consumed by
 * PathTracerApp::build() and IpuPathTraceJob::buildGraph() (PathTracerApp.cpp:799-817,
 * IpuPathTraceJob.cpp:95-138). */
typedef struct pt_config {
  uint32_t struct_size;          /* sizeof(pt_config) */
  uint32_t width, height;        /* --width/--height */
  uint32_t max_path_length;      /* --max-path-length (1..64) */
  uint32_t roulette_depth;       /* --roulette-depth (>= 1) */
  float stop_prob;               /* --stop-prob, rounded to half as on the IPU */
  float refractive_index;        /* --refractive-index, rounded to half as on the IPU */
  int32_t aa_noise_type;         /* --aa-noise-type */
  int32_t sample_precision;      /* PT_SAMPLES_HALF reproduces the IPU's half primary samples */
  int32_t device;                /* HIP device ordinal (the role of --ipus device selection) */
  uint32_t max_work_items;       /* capacity of the trace buffer (tiles x rays-per-tile) */
  uint32_t iterations_per_batch; /* sample iterations fused per kernel batch; 0 = auto */
  void* stream;                  /* hipStream_t to run on, or NULL for a private stream */
} pt_config;

/* One dense layer as NifModel streams it (src/neural_networks/DenseLayer.hpp:18-31,
 * NifModel.cpp:375-401): kernel row-major [rows = in][cols = out], bias [cols] or NULL,
 * raw fp16 or fp32 bytes as stored in the Keras H5 (Hdf5Model.cpp:109-133 accepts both; models with float32 layers are
 * slow: the fp32 matrix rate is 1/16 of the fp16 one).
 * Any Dense stack the reference's rule accepts is taken: first layer 4*embedding -> h0, every
 * later layer's input width either the previous width or that + 4*embedding (concat(x, input),
 * NifModel.cpp:305-308), head with 3 outputs; 2..16 layers, embedding 1..16, widths <= 2048. */
typedef struct pt_layer {
  uint32_t rows, cols;
  const void* kernel;
  const void* bias;
  int32_t dtype;                 /* PT_DTYPE_F16 or PT_DTYPE_F32.  A model ALL of whose layers share one type runs as the reference's
                                  * does: the matmul, bias add and ReLU in that type (NifModel.cpp:314-325).  A model that MIXES the two
                                  * is an EXTENSION of this library with cast points of its own: the reference ships no such model, never
                                  * casts x between layers and would most likely refuse one at graph construction.  Here every layer runs
                                  * in the type of its own kernel on the float path (fp32 matrix rate): a binary16 layer rounds its sum
                                  * to half, adds its bias in half and reads its input cast to half (RNE).  No reference fixture exists
                                  * for it: parity unpinned (checked against the oracle's restatement of the same rule only). */
  int32_t relu;                  /* activation == "relu" (NifModel.cpp:323-325) */
} pt_layer;

/* Replaces the three cycle-count streams (PathTracerApp.cpp:598-603) with per-stage device
 * times from HIP events, plus the counters the roofline accounting needs. */
typedef struct pt_stats {
  uint64_t paths;                /* path-samples traced by the last path_trace (work items that are not padding x samples) */
  uint64_t segments;             /* sum of pathLength (LoadBalancer.cpp:198-213 "totalRays") */
  uint64_t escaped;              /* paths that reached the environment light = NIF evaluations */
  uint64_t nif_flops_per_sample; /* NifModel::analyseModel formula (NifModel.cpp:129-133) */
  double path_trace_ms;          /* sum over trace-kernel launches  (path_trace_cycle_count) */
  double nif_ms;                 /* sum over NIF-kernel launches    (nif_cycle_count) */
  double accumulate_ms;          /* sum over accumulate launches (on the class map they expand too: pt_nif_class_stats) */
  double total_ms;               /* whole path_trace program        (iter_cycle_count x iterations) */
  uint32_t trace_launches, nif_launches, accumulate_launches;
  uint32_t first_sample;         /* absolute index of the step's first sample iteration (the RNG is keyed by pixel and this index) */
} pt_stats;

/* One traced path, for kernel-level parity checks: the information the reference keeps in the
 * per-ray contribution stack (PathTracerApp.cpp:301-308) reduced to what the deferred stages use. */
typedef struct pt_path_record {
  uint32_t length;               /* contribution-stack size incl. terminator (codelets.cpp:253) */
  uint32_t escaped;
  float dir[3];                  /* ESCAPED record direction (codelets.cpp:187) */
  float uv[2];                   /* PreProcessEscapedRays output (codelets.cpp:343-347) */
  float throughput[3];           /* product of clr*weight along the path incl. terminal weight */
  float cam[2];                  /* GenerateCameraRays output, half-rounded (codelets.cpp:74-75) */
} pt_path_record;

/* Construct the renderer: the work PathTracerApp::build() + GraphManager compile/load do
 * (PathTracerApp.cpp:310-484, ipu_utils.hpp:473-551).  Fails if no HIP device is usable. */
int pt_create(const pt_config* config, pt_handle* out);
int pt_destroy(pt_handle h);
/* Message for the last failure on `h` (or, with h == NULL, of the last failed pt_create). */
const char* pt_last_error(pt_handle h);
int pt_abi_version(void);
/* ABI 5.  Which shared objects this process really bound the library's HIP and RCCL imports to, and their versions, as one
 * JSON object: {"librccl": path, "libamdhip64": path, "rccl_version": ncclGetVersion() at run time, "rccl_compiled":
 * NCCL_VERSION_CODE of the headers libptmi.so was built against, "hip_runtime_version", "hip_driver_version"}.  libptmi.so
 * imports librccl.so.1 / libamdhip64.so.7 by SONAME: a process that has already loaded other copies under those names
 * (PyTorch ships its own) gets THOSE -- a process holds one HIP runtime, whichever was loaded first.  The reference has no
 * counterpart (its Poplar runtime is one library); the bench line and the tests record this so that nobody certifies one
 * RCCL and measures on another.  Needs no handle and no device.  Always NUL-terminated; PT_ERR_INVALID_ARGUMENT if the
 * buffer is too small (512 bytes are enough). */
int pt_runtime_info(char* buf, size_t n);

/* Program "init_nif_weights" (PathTracerApp.cpp:480; streams NifModel.cpp:375-401): all layer
 * kernels and biases, `max`, and `mean` with -eps already folded in (NifMetaData.cpp:48-53).
 * May be called again to hot-swap the environment (PathTracerApp.cpp:548-557). */
int pt_upload_nif(pt_handle h, const pt_layer* layers, uint32_t n_layers, uint32_t embedding_dim,
                  float max, const float mean[3], int32_t log_tonemap);
/* Constant-radiance environment instead of a NIF (BASELINE config C1; no reference program).  A third kind of environment,
 * an HDR image, is pt_set_env_map below. */
int pt_set_constant_env(pt_handle h, const float rgb[3]);

/* Program "init_render_settings" (PathTracerApp.cpp:479): streams seed u32[2], anti_alias_scale
 * (half), field_of_view (half, radians), hdri_azimuth (f32, radians), on_device_sample_limit.
 * A new seed restarts the sample-index sequence; the same seed continues it. */
int pt_set_render_settings(pt_handle h, uint64_t seed, float aa_noise_scale, float fov_radians,
                           float azimuth_radians, uint32_t samples_per_step);

/* Program "setup" (PathTracerApp.cpp:481): host -> device copy of the active worklist. */
int pt_setup(pt_handle h, const pt_trace_record* work, size_t n);
/* Program "path_trace" (PathTracerApp.cpp:482): samples_per_step iterations of
 * K2..K12 on the device (PathTracerApp.cpp:432-468).  Blocks until the device is done.
 * On failure every stream of the handle has been drained before the call returns (nothing is
 * left running on buffers the caller may free), the sample sequence has not advanced, and the
 * worklist's accumulators are undefined: call pt_setup again before the next path_trace. */
int pt_path_trace(pt_handle h);
/* Program "read_results" (PathTracerApp.cpp:483): device -> host copy of the worklist plus stats. */
int pt_read_results(pt_handle h, pt_trace_record* work, size_t n, pt_stats* stats);
/* Stats of the last path_trace without the device -> host copy. */
int pt_get_stats(pt_handle h, pt_stats* stats);
/* ABI 4.  Name of the NIF kernel(s) the library dispatched for the uploaded model at its last NIF launch (the reference
 * logs its model through NifModel::analyseModel, NifModel.cpp:122-144; here the kernel choice depends on the shape: fused
 * register-resident, layer by layer, or float32).  Empty before the first launch.  Always NUL-terminated. */
int pt_nif_kernel_name(pt_handle h, char* buf, size_t n);
/* ABI 4.  Calibration of the NIF stage, the counterpart of reading nif_cycle_count (PathTracerApp.cpp:449,598-603) with
 * nothing else on the device: runs the NIF stage of the largest batch of the LAST pt_path_trace again -- same kernel, same
 * compacted queue, which is still resident -- one untimed launch and then `launches` timed ones back to back, with no trace
 * or accumulate kernel beside it.  Returns the average milliseconds per launch (HIP events on the NIF stream) and the
 * number of NIF evaluations per launch (the queue length).  The worklist's accumulators are not touched.  Comparing this
 * rate with the one inside a step separates a slow device from a regression of the pipeline around the kernel. */
int pt_calibrate_nif(pt_handle h, uint32_t launches, double* ms_per_launch, uint64_t* evaluations);
/* With NIF sharing on (below), pt_calibrate_nif replays what that step really ran: the NIF stage over the batch's DISTINCT
 * queue, and `evaluations` is that queue's length. */

/* Exact sharing of NIF evaluations -- an EXTENSION: the reference evaluates the NIF on every escaped path
 * (PathTracerApp.cpp:147-198).  The NIF output of an escaped path depends on its (u, v) alone (the azimuth is folded in by
 * PreProcessEscapedRays, codelets.cpp:343-347; the path's throughput multiplies the decoded BGR afterwards, one fp32 multiply
 * per channel), and camera rays and primary samples are half, so many escaped paths carry bit-identical (u, v).
 *   PT_NIF_SHARE_OFF    every escaped path is one NIF row: the library runs exactly as without this API -- same kernels,
 *                       launches, streams and events.
 *   PT_NIF_SHARE_BATCH  paths of one kernel batch whose queue entries have bit-identical (u, v) share one NIF evaluation.
 *   PT_NIF_SHARE_STEP   the same across all batches of one pt_path_trace.
 * Exact: the key is the 64 raw bits of (u, v), with no tolerance; each distinct key is evaluated once by the unchanged NIF
 * kernels (every kernel family, float32 and mixed models included), and every path gets owner_bgr[k] * throughput[k], the
 * same single fp32 multiply the per-path NIF head does.  So every accumulator, record, resident-film value and HDR tile is
 * bit-identical to sharing off, for any option set and any table capacity.  A key that finds no table slot (full table, or
 * the key equals the table's empty marker) is evaluated on its own and counted in `overflowed`: never dropped.
 * THE DEFAULT IS AUTOMATIC.  A handle on which neither pt_set_nif_sharing nor pt_set_nif_memo was ever called runs PT_NIF_SHARE_STEP in every
 * pt_path_trace for which all of these hold, and PT_NIF_SHARE_OFF otherwise:
 *   - the environment is a NIF model (pt_upload_nif), not a constant and not an environment map;
 *   - the memo (pt_set_nif_memo) is off;
 *   - the step's distinct-queue store has fewer than 2^31 entries, and what the step has to allocate -- the table (12 bytes per
 *     slot), the store (20 bytes per queue slot of every batch) and the owner maps, less what the handle already holds -- is at
 *     most a quarter of the free device memory at that moment.
 * In automatic mode an allocation that fails all the same is no error: the buffers are given back and the handle runs off
 * from then on.  The result is the same bytes either way; `mode` of pt_nif_sharing_stats says what really ran.  The first
 * call of pt_set_nif_sharing, with any mode, ends the automatic choice for the handle: PT_NIF_SHARE_OFF then gives the
 * unshared step whatever the environment, and a sharing mode reports its errors as described below.
 * A valid pt_set_nif_memo call, with 0 too, ends it as well: a caller that manages the memo gets the sharing mode it set, which
 * is PT_NIF_SHARE_OFF until it says otherwise, so turning the memo off again gives the unshared step as before.
 * No table survives a step: every pt_path_trace starts empty, so hot-swapping the NIF (pt_upload_nif), a new azimuth
 * (pt_set_render_settings) and a mode switch between steps need no invalidation.
 * pt_set_nif_sharing takes effect at the next pt_path_trace.  The first explicit switch to a sharing mode allocates the device table
 * (sized from the batch capacity and the free memory) and the distinct-queue store: PT_ERR_OUT_OF_MEMORY leaves the mode
 * off.  A step-scope step with more batches than the store holds grows it (pt_path_trace may then return
 * PT_ERR_OUT_OF_MEMORY).  A bad mode or a NULL handle is PT_ERR_INVALID_ARGUMENT.
 * pt_stats keeps its meaning (escaped = escaped paths); pt_get_nif_sharing_stats reports the distinct lookups the last path_trace
 * handed to its NIF stage: evaluations == escaped with sharing off, 0 with a constant environment (no sharing pass runs then).  The caller
 * sets struct_size = sizeof(pt_nif_sharing_stats). */
enum { PT_NIF_SHARE_OFF = 0, PT_NIF_SHARE_BATCH = 1, PT_NIF_SHARE_STEP = 2 };
typedef struct pt_nif_sharing_stats {
  uint32_t struct_size;          /* sizeof(pt_nif_sharing_stats), set by the caller */
  int32_t mode;                  /* mode the last path_trace really ran with, chosen or automatic (PT_NIF_SHARE_OFF with a constant environment) */
  uint64_t escaped;              /* = pt_stats.escaped */
  uint64_t evaluations;          /* distinct (u, v) bit pairs the last path_trace handed to its NIF stage: the distinct queues' length (= escaped with sharing off); the rows the network ran are pt_nif_class_stats.mlp_rows */
  uint64_t overflowed;           /* entries evaluated alone because no table slot was free */
  uint64_t table_slots;          /* table capacity in use (0 with sharing off) */
  double share_ms;               /* device time of the sharing passes (HIP events, read lazily like the stage times); at step scope without the memo these claim the class too (pt_nif_class_stats), and their time is all here; on the class map with the expansion inside the accumulate passes: the class claim, the raw-pair pass and the release */
} pt_nif_sharing_stats;
int pt_set_nif_sharing(pt_handle h, int32_t mode);
int pt_get_nif_sharing_stats(pt_handle h, pt_nif_sharing_stats* out);

/* The class level of the NIF stage.  Every NIF inference kernel reads a coordinate as x = (coord - 1) * 2 and then only the
 * binary16 values half(x * 2^j), j < 16; for 2^-14 <= |x| <= 2 those are a function of half(x) alone, so two lookups whose u
 * and whose v round to the same half get the same BGR, bit for bit, although their fp32 (u, v) differ.  Whenever the NIF stage
 * runs over a distinct queue -- PT_NIF_SHARE_BATCH, PT_NIF_SHARE_STEP (chosen or automatic) and the memo, with a NIF as the
 * environment -- it therefore evaluates one row per such class and copies the result to the class's other entries; the class
 * table lives for one pt_path_trace.  Every output is the same bytes as without the level; the sharing key, the memo key and
 * pt_nif_sharing_stats.evaluations stay what they were.  If the level's buffers do not fit a quarter of the free device memory,
 * or their allocation fails, the step runs without it, and that is no error.  Sharing off launches nothing of it.
 * In a PT_NIF_SHARE_STEP step (chosen or automatic) without the memo the level has no passes of its own: the sharing passes
 * claim an entry's class where they claim its (u, v) pair and hand every path the BGR of its class's row.  class_ms is then 0
 * and pt_nif_sharing_stats.share_ms covers the claim of both levels, the resolve and the expand pass; with PT_NIF_SHARE_BATCH
 * and with the memo, class_ms is the level's own claim, resolve and spread passes.
 * Such a step keeps its classes in a CLASS MAP where it can: a coordinate of [0, 1) has one of 15361 classes, so a pair of them
 * is a number below 15361^2 and its class row is one 32-bit word of a 944 MB map -- no key, no probe; whatever else a queue may
 * hold (a coordinate of 1 or above, NaN) goes to a small hashed tail of 2^16 slots, and a full tail means rows evaluated alone.
 * The step claims an entry's class with that one word, counts the raw pairs in a pass of its own that nothing waits for
 * (evaluations and overflowed keep their values), runs no resolve pass, and gives the words it took back at its end, so the
 * map is cleared once in a handle's life.  The map is allocated by the first such step if it fits a quarter of the free device
 * memory; otherwise the step uses the hashed class table as before, and that is no error.  table_slots then reports the map's
 * words plus the tail's slots.
 * A step on the map over a worklist of a multiple of four items has no expand pass: its accumulate passes form the escaped
 * paths' radiance themselves, from the class rows.  pt_nif_sharing_stats.share_ms then covers the class claim, the raw-pair
 * pass and the release, and pt_stats.accumulate_ms the accumulate passes with the expansion inside.
 * The caller sets struct_size = sizeof(pt_nif_class_stats). */
typedef struct pt_nif_class_stats {
  uint32_t struct_size;          /* sizeof(pt_nif_class_stats), set by the caller */
  int32_t ran;                   /* the last path_trace ran the class level */
  uint64_t mlp_rows;             /* rows the NIF kernels executed in the last path_trace (= evaluations if the level did not run) */
  uint64_t alone;                /* rows evaluated alone because no slot of the class table was free */
  uint64_t table_slots;          /* class table capacity in use (0 if the level did not run); with the class map: its 15361^2 words + the tail's slots */
  double class_ms;               /* device time of the level's own claim, resolve and spread passes (batch scope, the memo); 0 where the sharing passes claim the class (step scope without the memo) (HIP events, read lazily) */
} pt_nif_class_stats;
int pt_get_nif_class_stats(pt_handle h, pt_nif_class_stats* out);

/* Persistent memo of NIF evaluations across steps -- an EXTENSION like sharing.  The decoded BGR of a key (the 64 raw bits of
 * (u, v), azimuth already folded in) depends on the uploaded model alone, so it stays valid from step to step until
 * pt_upload_nif.  pt_set_nif_memo(h, max_bytes) turns on a device table of at most max_bytes (48 bytes per slot: one 32-byte
 * slot -- key, state, last-hit step, decoded BGR -- and room to retain it; a power of two, at most 2^30 slots); 0 turns it off
 * (the default: the library then runs exactly as without this API).  Setting the capacity it already has keeps the entries.
 * Exact: a key found in the memo gets the fp32 BGR the NIF kernels' out_bgr mode wrote for it, times the path's throughput by
 * the heads' own single fp32 multiply per channel, so every record, accumulator, resident-film value and HDR tile is
 * bit-identical to memo off, for every option set, every kernel family (fused fp16, layer-by-layer wide, float32, mixed) and
 * any capacity.  Independent of the sharing mode: with the memo on every batch looks the memo up first, and the keys it does
 * not hold are shared as by PT_NIF_SHARE_STEP (in the step store) whatever pt_set_nif_sharing says.  Values of a step are
 * published into the memo once, at its end, so later batches of the same step reach them through the step store.  A key
 * that finds no slot within the probe limit is evaluated on its own and counted in `overflowed`: never dropped.  When more
 * than half of the slots are occupied after a step, the next step starts with a retain pass that keeps only the entries hit
 * in the last step (`retains` counts them).
 * Generation: pt_upload_nif, pt_set_env_map, pt_clear_nif_memo and a pt_path_trace that fails start a new generation (every
 * entry is forgotten).  Nothing else invalidates the memo: not pt_set_render_settings (seed, fov, azimuth, AA), not pt_setup, not
 * pt_set_scene, not pt_set_constant_env -- with a constant environment no memo pass runs.
 * Allocation: pt_set_nif_memo can return PT_ERR_OUT_OF_MEMORY and the memo is then left off; max_bytes between 1 and
 * 48 KiB - 1 is PT_ERR_INVALID_ARGUMENT.  The step store of step-scope sharing (not counted in max_bytes) is used and grown
 * as with PT_NIF_SHARE_STEP.
 * pt_nif_sharing_stats keeps its meaning: `evaluations` counts the entries of the distinct queues, so evaluations == escaped holds only
 * when both sharing and the memo are off; with the memo on its passes are timed in memo_ms, not share_ms.  The caller sets
 * struct_size = sizeof(pt_nif_memo_stats).  A NULL handle is PT_ERR_INVALID_ARGUMENT. */
typedef struct pt_nif_memo_stats {
  uint32_t struct_size;          /* sizeof(pt_nif_memo_stats), set by the caller */
  int32_t enabled;               /* the memo is on */
  uint64_t slots, occupied;      /* capacity in use; valid entries after the last step */
  uint64_t escaped, served;      /* escaped paths of the last step; of those, served from entries of EARLIER steps */
  uint64_t evaluations, inserted;/* distinct (u, v) bit pairs the last step handed to its NIF stage (pt_nif_sharing_stats.evaluations); new entries it published */
  uint64_t overflowed;           /* evaluated alone: no slot within the probe limit */
  uint64_t generation, retains;  /* bumped by upload / clear / failed step; retain passes so far */
  double memo_ms;                /* device time of the memo passes of the last step (HIP events, read lazily) */
} pt_nif_memo_stats;
int pt_set_nif_memo(pt_handle h, uint64_t max_bytes);
int pt_clear_nif_memo(pt_handle h);
int pt_get_nif_memo_stats(pt_handle h, pt_nif_memo_stats* out);

/* Runtime scene -- an EXTENSION: the reference's scene is compile-time, five spheres and a floor disc on the stack of
 * RayTraceKernel::compute ("For now the scene is hard coded", codelets.cpp:90,110-144).  pt_set_scene replaces it with up to
 * PT_MAX_SCENE_OBJECTS spheres and discs, tested for the nearest hit in the order given (Scene::intersect, codelets.cpp:183).
 *   shape     PT_SHAPE_SPHERE or PT_SHAPE_DISC (a disc is the set of points of its plane within `radius` of `centre`).
 *   material  PT_MATERIAL_DIFFUSE: colour is the factor the kernel multiplies by (the built-in scene's values include the
 *             reference's colourGain 2, codelets.cpp:127); PT_MATERIAL_SPECULAR: colour is kept but unused (the reference's
 *             tint is one); PT_MATERIAL_REFRACTIVE: colour is the tint of a refracted ray (the refractive index stays
 *             pt_config.refractive_index); PT_MATERIAL_EMISSIVE: colour is the emitted radiance.
 *   normal    disc only, normalised by the library once on the host as n / sqrtf(dot(n, n)) in binary32; stored as 0 for a sphere.
 * Validation: PT_ERR_INVALID_ARGUMENT, and pt_last_error names the object's index and the bad field, for n outside 1..32, a
 * shape or material out of range, any value that is not finite, radius <= 0, a negative colour component, a disc normal of
 * length zero, or a NULL table with n > 0.  After a rejection the previous scene stays in force.  (NULL, 0) restores the
 * built-in scene.  The built-in table passed through pt_set_scene renders bit-identically to no call.
 * A new scene takes effect at the next pt_path_trace / pt_trace_paths.  It does not touch the worklist, the accumulators, the
 * resident film, tile costs, NIF sharing or the NIF memo (memo keys depend on (u, v) and the model only).
 * Emitters: a hit on an emissive object ends the path with an EMIT entry (codelets.cpp:192-196; the material type is not
 * consulted), folded like an escape (:269-271): the path's radiance is emission * T per channel, T its throughput including
 * that segment's roulette factor, by one fp32 multiply as with a constant environment.  The EMIT entry counts in the path's
 * length (pt_stats.segments, TraceRecord pathLength).  pt_stats.escaped keeps its meaning -- paths that reached the
 * environment, = NIF evaluations -- and does not count emitter paths; a step in which no path escapes is valid in NIF mode.
 * pt_trace_paths reports an emitter path with escaped = 2, its throughput T and the direction of the ray that hit the emitter.
 * pt_get_scene copies the table in force (the stored, normalised values) into out[0 .. capacity) and its size into *n;
 * h == NULL gives the built-in table and needs no device.  out may be NULL with capacity 0 to ask for the size; a smaller
 * capacity is PT_ERR_INVALID_ARGUMENT.  A NULL handle given to pt_set_scene is PT_ERR_INVALID_ARGUMENT. */
enum { PT_SHAPE_SPHERE = 0, PT_SHAPE_DISC = 1 };
enum { PT_MATERIAL_DIFFUSE = 0, PT_MATERIAL_SPECULAR = 1, PT_MATERIAL_REFRACTIVE = 2, PT_MATERIAL_EMISSIVE = 3 };
#define PT_MAX_SCENE_OBJECTS 32
typedef struct pt_scene_object {     /* 48 bytes */
  int32_t shape, material;
  float centre[3];
  float radius;
  float normal[3];                   /* disc only; normalised by the library; 0 for spheres */
  float colour[3];                   /* diffuse: factor; refractive: tint; specular: unused; emissive: emitted radiance */
} pt_scene_object;
int pt_set_scene(pt_handle h, const pt_scene_object* objects, uint32_t n);
int pt_get_scene(pt_handle h, pt_scene_object* out, uint32_t capacity, uint32_t* n);

/* Polygons in a runtime scene -- an EXTENSION, opt-in and additive: PTMI_ABI_VERSION stays 5 and no existing struct moves; a
 * process that never calls pt_set_scene_ex launches the kernels it launched before and renders the same bits.  pt_set_scene_ex
 * takes the same table as pt_set_scene with nine more floats per object, and two more shapes, traced by the same object loop in
 * declaration order under the same cap of PT_MAX_SCENE_OBJECTS.
 * Geometry: e1 = v1 - v0, e2 = v2 - v0, both in binary32.  PT_SHAPE_TRIANGLE is the set v0 + a e1 + b e2 with a, b >= 0 and
 * a + b <= 1; PT_SHAPE_PARALLELOGRAM the same with a <= 1 and b <= 1 (its fourth corner is v1 + v2 - v0).  The stored normal is
 * n = c / sqrtf(dot(c, c)), c = cross(e1, e2), formed once on the host by the same volatile, left-to-right binary32 expressions
 * as a disc's normal.  pt_get_scene_ex returns a polygon with centre = v0, radius = 0 and normal = n, and a sphere or disc with
 * vertex = 0.
 * Intersection (device, every operation one rounded binary32, no contraction), in the kernel's frame, for a ray (o, d):
 *   pv = cross(d, e2); det = dot(e1, pv); det == 0 -> miss
 *   inv = 1 / det; tv = sub(o, v0)
 *   a = dot(tv, pv) * inv;  !(a >= 0) or a > 1 -> miss
 *   qv = cross(tv, e1); b = dot(d, qv) * inv;  !(b >= 0) -> miss
 *   triangle: a + b > 1 -> miss;  parallelogram: b > 1 -> miss
 *   t = dot(e2, qv) * inv;  t > 1e-5 else miss
 * and then the scene's own t > eps && t < tbest in declaration order, as for every object.  Polygons are two-sided: for a
 * diffuse or specular polygon the shading normal is dot(n, d) > 0 ? -n : n; the refractive branch flips the normal itself, as
 * it does for every object; an emissive polygon emits from both faces (the material is not consulted, as for every emitter).
 * Shared edges are NOT watertight in binary32: a ray can pass between two walls of a box that share an edge.
 * Camera: under a pose v0 enters the kernels as a point, R^T (v0 - position), and e1, e2 and the stored world n each as a
 * direction, R^T x, as centres and disc normals do; the built-in camera applies nothing.
 * Validation: PT_ERR_INVALID_ARGUMENT, pt_last_error naming the object's index and the field, checked in this order before any
 * device call: stride != sizeof(pt_scene_object_ex); n outside 1..32; a NULL table; then per object: a shape outside 0..3; a
 * material outside 0..3; a used field that is not finite (polygon: vertex and colour -- centre, radius and normal are ignored;
 * sphere, disc: centre, radius, normal, colour -- vertex is ignored); a negative colour component; a sphere's or disc's radius
 * <= 0 and a disc normal of length zero; a polygon whose e1, e2 or cross(e1, e2) is not finite or whose dot(c, c) is not > 0
 * ("vertices are collinear"); last, a NULL handle, whose message is pt_last_error(NULL)'s.  After a rejection the previous
 * scene stays in force.  (NULL, 0, stride) restores the built-in scene.  pt_get_scene_ex(NULL, ...) gives the built-in table and
 * needs no device; out may be NULL with capacity 0 to ask for the size.
 * Coexistence: pt_set_scene is unchanged and still refuses shapes above 1.  A table of spheres and discs given through
 * pt_set_scene_ex is the same scene bit for bit and runs the same kernels.  While a scene with a polygon is in force
 * pt_get_scene still reports the count in *n and answers PT_ERR_INVALID_ARGUMENT ("use pt_get_scene_ex") when asked to copy.
 * pt_stats, the escaped = 2 convention of pt_trace_paths, NIF sharing, the memo, the film and tile costs behave as for any
 * scene.  Feature buffers: object_id is the index, depth is t, normal is the stored normal flipped to face the ray and then
 * rotated to world space (the disc rule), albedo follows the material rule.  The environment guide applies to a diffuse hit on
 * a polygon as to any diffuse hit; eligibility and densities of the emitter guide at a polygon hit use n as the bounce forms
 * it, that is, flipped. */
enum { PT_SHAPE_TRIANGLE = 2, PT_SHAPE_PARALLELOGRAM = 3 };
typedef struct pt_scene_object_ex {   /* 84 bytes; the first 48 are pt_scene_object, field for field */
  int32_t shape, material;
  float centre[3];
  float radius;
  float normal[3];
  float colour[3];
  float vertex[3][3];                 /* polygons: v0, v1, v2 in world space */
} pt_scene_object_ex;
int pt_set_scene_ex(pt_handle h, const pt_scene_object_ex* objects, uint32_t n, uint32_t stride /* = sizeof(pt_scene_object_ex) */);
int pt_get_scene_ex(pt_handle h, pt_scene_object_ex* out, uint32_t capacity, uint32_t* n);

/* Triangle meshes in a runtime scene -- an EXTENSION, opt-in and additive: PTMI_ABI_VERSION stays 5 and no existing struct moves; a
 * process that never calls pt_set_scene_meshes launches the kernels it launched before and renders the same bits.
 *
 * Rows and meshes.  The table is pt_set_scene_ex's with one more shape, PT_SHAPE_MESH.  The k-th row of that shape, in declaration
 * order, takes meshes[k]; the number of such rows must equal n_meshes.  A mesh is ONE row of the table, whatever its size: n stays
 * 1..32.  Material and colour come from the row -- all four materials, one per mesh -- and a mesh row ignores centre, radius,
 * normal and vertex.  A table without a mesh row (n_meshes == 0) IS pt_set_scene_ex's scene, bit for bit, on the kernels that ran
 * before.  pt_set_scene and pt_set_scene_ex are unchanged and still refuse shape 4.  (NULL, 0, stride, NULL, 0) restores the
 * built-in scene.
 *
 * Copies.  The library copies everything and retains no host pointer.  It keeps a host copy of the triangles' world-space frames
 * (48 bytes per triangle), because a new camera needs them (below); the trees and the triangles the kernels read live in device
 * memory (pt_mesh_info.device_bytes), owned by the handle and freed by pt_destroy or by the next scene.
 *
 * Triangle j of a mesh.  v0, v1, v2 are vertices[indices[3 j + 0 .. 2]]; e1 = v1 - v0 and e2 = v2 - v0 in binary32, and the
 * stored normal is n = c / sqrtf(dot(c, c)), c = cross(e1, e2), exactly as for a PT_SHAPE_TRIANGLE object.  Shading is FLAT unless
 * normals are attached (pt_set_mesh_normals below), and a mesh has one colour unless a texture is attached (pt_set_mesh_texture).
 *
 * Intersection.  A triangle is tested by the expression sequence of a PT_SHAPE_TRIANGLE object, unchanged, then by the scene's
 * t > eps and t < tbest in declaration order, as every object is.  Ties inside one mesh: the smallest t wins and, among equal
 * t, the lowest triangle index, so the result does not depend on the tree and equals what the same triangles would give as
 * consecutive PT_SHAPE_TRIANGLE rows.  Across objects the rule stays declaration order, strict <.
 * NOT WATERTIGHT: the triangle test decides every triangle on its own, and its t > eps starts a bounce a little off the surface, so
 * a ray that meets the shared edge of two triangles, or leaves a hit point within about eps of such an edge, can pass between
 * them.  A closed unit box about the camera lets 8 of 6144 mirror paths and 22 of 6144 diffuse paths of six bounces out.  The
 * same triangles as PT_SHAPE_TRIANGLE rows let the identical paths out: it is the polygon test's property, and the tree adds none.
 *
 * The tree.  Each mesh gets a binary bounding-volume hierarchy, built on the host by binned SAH (or, opt-in, on the device:
 * pt_set_mesh_build below) with at most four triangles per
 * leaf and walked by the kernels without a stack (depth-first node order with skip links).  Node boxes are padded outward by one
 * value per mesh, pad = 2^-16 x the largest absolute coordinate of the mesh's box (pt_mesh_info.pad).  The pad is a safety margin,
 * not a proof: the triangle test's rounding grows at grazing incidence and with the distance of the ray's origin (from thousands
 * of box sizes away, where an ulp of t reaches the pad, ties between neighbouring triangles can fall the other way).  What is
 * promised is that the library's tests find no difference between the tree walk and a loop over all triangles
 * (PT_MESH_INTERSECT_BRUTE below is that loop).  The box test drops an axis whose slab products are NaN (0 x inf: the origin in a
 * slab plane, the direction parallel to it) and visits a node whose near distance EQUALS the best t so far.  With a positive pad
 * neither rule can change a result for rays from nearby -- a ray in a padded box's face is a pad away from that box's triangles
 * -- so nothing that runs the shipped pad, on the device or the host, can tell a wrong NaN rule from a right one: it is pinned on
 * the host alone, by a tree built with pad 0 (tests/mesh_bvh_main.cpp); the equality is also met on the device, by rays from far
 * above a flat mesh, where rounding absorbs the pad.
 *
 * Shading and other passes.  A mesh triangle is two-sided and follows the polygon rules word for word: the stored normal is
 * flipped to face the ray for diffuse and specular, glass flips its own normal, an emitter emits from both faces.  Feature
 * buffers: object_id is the ROW index; depth and normal are the hit triangle's (the disc / polygon rule); albedo follows the
 * material rule.  Emitter guide: an emissive mesh is SKIPPED by the table, whether or not polygon lamps are asked for; it is reached
 * by the hemisphere and environment branches, so the estimator stays unbiased (n_lights and object_index say what is listed).
 * The environment guide applies at a diffuse mesh hit as at any diffuse hit.
 *
 * Camera.  Under a pose v0 enters the kernels as a point and e1, e2 and n as directions through the camera's transform, from
 * the world values -- exactly what polygons do -- and the tree is built over the triangles as the kernel sees them.  A
 * pt_set_camera that changes the pose makes the meshes stale: they are transformed and rebuilt before the next pt_path_trace,
 * pt_trace_paths, pt_feature_buffers or pt_mesh_intersect.  Device buffers are sized once, at pt_set_scene_meshes (a tree of T
 * triangles has at most 2 T - 1 nodes): a rebuild allocates no device memory and cannot run out of it.  pt_mesh_info.build_ms
 * reports the last build.  (pt_set_mesh_build below: the build can run on the device, and a pose change can refit instead.)
 *
 * Validation returns PT_ERR_INVALID_ARGUMENT, and pt_last_error names the object, the mesh, the triangle and the field.  The
 * checks run in this order, before any device call: stride; n outside 1..32; a NULL table; per row the checks of
 * pt_set_scene_ex (a mesh row: material and colour only); the number of mesh rows against n_meshes (and a NULL mesh table); per
 * mesh struct_size, NULL vertices or indices, n_triangles == 0; the scene's total above PT_MAX_MESH_TRIANGLES; then per mesh
 * and triangle an index >= n_vertices, a referenced vertex that is not finite, and e1, e2 or their cross product not finite or
 * dot(c, c) not > 0 ("vertices are collinear"); last, a NULL handle (pt_last_error(NULL) then reports it).  After a rejection
 * or PT_ERR_OUT_OF_MEMORY the previous scene stays in force.
 *
 * Getters.  pt_get_scene_ex reports a mesh row with shape 4 and its geometric fields 0.  pt_get_scene answers as it does for a
 * polygon: the count, and PT_ERR_INVALID_ARGUMENT when asked to copy.  pt_get_mesh_info describes mesh k of the scene in force
 * (PT_ERR_INVALID_ARGUMENT when there is none). */
enum { PT_SHAPE_MESH = 4 };
#define PT_MAX_MESH_TRIANGLES (1u << 22)      /* per scene, all meshes together */
typedef struct pt_mesh {              /* 32 bytes */
  uint32_t struct_size;               /* sizeof(pt_mesh) */
  uint32_t n_vertices, n_triangles;
  const float* vertices;              /* [n_vertices][3], world space, host memory */
  const uint32_t* indices;            /* [n_triangles][3] */
} pt_mesh;
int pt_set_scene_meshes(pt_handle h, const pt_scene_object_ex* objects, uint32_t n, uint32_t stride /* = sizeof(pt_scene_object_ex) */,
                        const pt_mesh* meshes, uint32_t n_meshes);
typedef struct pt_mesh_info {         /* 48 bytes */
  uint32_t struct_size;               /* in: sizeof(pt_mesh_info) */
  uint32_t object_index;              /* the mesh's row in the table */
  uint32_t n_triangles, n_nodes;
  uint32_t max_leaf, depth;           /* most triangles in a leaf (<= 4); levels of the tree */
  uint64_t device_bytes;              /* this mesh's share of the device buffers, sized for 2 T - 1 nodes */
  double build_ms;                    /* host time of the last transform + build of this mesh (pt_set_mesh_build: device time under the device paths) */
  float pad;                          /* the outward pad of its node boxes, in the kernel's frame */
} pt_mesh_info;
int pt_get_mesh_info(pt_handle h, uint32_t mesh, pt_mesh_info* out);
/* Kernel-level hook, like pt_light_guide_sample and pt_env_map_lookup: the kernels' own mesh-aware nearest hit over n caller
 * rays, origin[n][3] and dir[n][3].  Origins and directions are WORLD space and the camera in force is IGNORED: the rays meet
 * the scene as the built-in camera sees it (under a pose the trees are rebuilt for this call and again for the next render).
 * out_t[i] is the hit distance (0 for a miss), out_object[i] the row index (-1 for a miss) and out_triangle[i] the triangle's
 * index in its mesh (-1 unless a mesh was hit).  PT_MESH_INTERSECT_BRUTE replaces the tree walk by a loop over all triangles
 * of each mesh with the same triangle function and the same tie rule: the yardstick for the tree.  PT_ERR_NOT_READY without a
 * mesh in force; n == 0 is a no-op. */
enum { PT_MESH_INTERSECT_BVH = 0, PT_MESH_INTERSECT_BRUTE = 1 };
int pt_mesh_intersect(pt_handle h, const float* origin, const float* dir, size_t n, int32_t mode,
                      float* out_t, int32_t* out_object, int32_t* out_triangle);

/* Vertex normals of a mesh (smooth shading) -- an EXTENSION, opt-in and additive: PTMI_ABI_VERSION stays 5, pt_mesh, pt_mesh_info
 * and every other struct and entry point keep layout and behaviour, and a process that never attaches normals launches the
 * kernels it launched before and renders the same bits.  The new code lives in kernel instances of its own (SMOOTH), launched only
 * while a mesh of the scene in force has normals.
 *
 * Attaching and removing.  pt_set_mesh_normals gives mesh `mesh` of the scene in force (counted as in pt_get_mesh_info) its
 * normals.  normal_indices == NULL: corner c of triangle j uses normals[indices[3 j + c]] -- per-vertex normals; n_normals must
 * equal the mesh's n_vertices.  Otherwise corner c uses normals[normal_indices[3 j + c]] -- per-corner normals, as OBJ's v//vn,
 * which allow creases.  (h, mesh, NULL, 0, NULL) removes the normals: the mesh is flat again and renders the flat bits.  Any
 * pt_set_scene* drops all normals with the scene.  A mesh WITHOUT normals beside one with normals takes none of the steps
 * below and renders its flat bits (a flag per mesh row).
 *
 * Copies and memory.  The library copies everything.  The handle keeps the world normals per corner in triangle order (36 bytes
 * per triangle of a mesh with normals; a pose change needs them), the mesh's own indices (12 bytes per triangle) and, for per-corner
 * normals, the caller's normal_indices (12 bytes per triangle; pt_update_mesh_vertices looks new normals up by them).  The device
 * holds three 16-byte vectors per triangle SLOT in leaf order, indexed by the global slot a hit carries: 48 bytes per triangle,
 * which pt_mesh_normals_info.device_bytes reports for a mesh with normals: THIS MESH'S SHARE.  The buffer itself spans the slots
 * of all meshes of the scene, the flat ones included (the slot of a hit indexes it directly), is allocated whole by the first call
 * that attaches normals and PERSISTS until the next scene or pt_destroy: removing the last normals does not free it, so that
 * attaching again, and every rebuild in between, allocates nothing.  The device memory held for normals is therefore
 * 48 x (the sum of pt_mesh_info.n_triangles over the scene's meshes) from the first attachment on, which the sum of device_bytes
 * under-reports by the flat meshes' slots and, after a removal, by the removed mesh's.  On PT_ERR_OUT_OF_MEMORY the mesh stays as
 * it was.
 *
 * Host preparation.  Each referenced normal is normalised once, n / sqrtf(dot(n, n)) in binary32, every intermediate rounded,
 * the sum left to right -- a disc normal's expressions.
 *
 * Validation returns PT_ERR_INVALID_ARGUMENT, and pt_last_error names the mesh, the triangle, the normal and the field: a NULL
 * handle (pt_last_error(NULL)); no mesh `mesh` in force; NULL normals with n_normals > 0 (or with indices); n_normals different
 * from n_vertices when normal_indices is NULL; then per triangle and corner an index >= n_normals, a referenced normal that is not
 * finite, or whose dot(n, n) is not > 0 and finite.  Unreferenced normals are not examined.  After a rejection the mesh keeps
 * what it had.
 *
 * Camera.  A normal is a direction: under a pose it enters the kernels as R^T n from the world value, as e1, e2 and the stored n
 * do.  The rebuild a pose change triggers re-expands the normals into the new slot order and allocates nothing on the device.
 *
 * The shading normal (csrc/pt_mesh.h: shading_normal, one function for the kernels and the host), at a hit of the ray (o, d) on a
 * triangle of a mesh with normals; every operation one rounded binary32, no contraction:
 *   1. a, b by the triangle test's own expressions on the winning triangle (formed again at the hit: the same bits), c = (1 - a) - b.
 *   2. m = ((c n0) + (a n1)) + (b n2) per component, l2 = dot(m, m); ns = m * (1 / sqrtf(l2)) -- the kernels' normalise -- when
 *      l2 > 1e-12, else ns = ng, the triangle's stored geometric normal.
 *   3. Orientation: dot(ns, ng) < 0 -> ns = -ns.  Normals wound against the triangle shade as if wound with it.
 *   4. Side: (dot(ns, d) > 0) != (dot(ng, d) > 0) -> ns = ng.  At grazing incidence a shading normal that would put the ray on the
 *      other side of the surface is dropped for this hit; glass therefore decides inside / outside exactly as the geometry does.
 *   5. n = ns and the bounce continues unchanged: the two-sided flip for diffuse and specular, glass's own flip, the hemisphere
 *      about n, cos = dot(d', n).  Both guides use this n.
 *   6. Specular only: after v = d - 2 dot(d, n) n, if dot(v, ng_f) <= 0 (ng_f: ng flipped to face the ray) v is formed again with
 *      ng_f in place of n.  A mirror never reflects into its own surface.
 *   7. Diffuse and glass get no such correction: a diffuse direction with dot(d', n) > 0 that points below the geometric surface
 *      is taken and meets the mesh again -- the usual shading-normal terminator, a documented limit like the non-watertight edges.
 * Emissive hits return before any normal is formed.  Feature buffers: `normal` is the shading normal after steps 1-4, flipped to
 * face the centre ray, then rotated to world space; object id, depth and albedo are unchanged. */
int pt_set_mesh_normals(pt_handle h, uint32_t mesh, const float* normals /* [n_normals][3], world space */, uint32_t n_normals,
                        const uint32_t* normal_indices /* [n_triangles][3], or NULL */);
typedef struct pt_mesh_normals_info {   /* 24 bytes */
  uint32_t struct_size;               /* in: sizeof(pt_mesh_normals_info) */
  uint32_t has_normals;               /* 1: the mesh shades smooth */
  uint32_t per_corner;                /* 1: given with normal_indices */
  uint32_t n_normals;                 /* as given */
  uint64_t device_bytes;              /* this mesh's share: 48 per triangle while it has normals, else 0 (the buffer: see above) */
} pt_mesh_normals_info;
int pt_get_mesh_normals_info(pt_handle h, uint32_t mesh, pt_mesh_normals_info* out);
/* Kernel-level hook, like pt_mesh_intersect: world-space rays, the camera IGNORED.  The smooth instances' own nearest hit and the
 * shading-normal function.  out_t, out_object, out_triangle as pt_mesh_intersect's; for a hit on a mesh triangle out_bary[i] is
 * (a, b) and out_normal[i] the normal after steps 1-5 with the two-sided flip (it faces the ray), in world space -- for a mesh
 * without normals the flipped stored normal.  For a miss or a hit on anything but a mesh triangle both are zero.
 * PT_ERR_NOT_READY without a mesh in force; n == 0 is a no-op. */
int pt_mesh_shade(pt_handle h, const float* origin, const float* dir, size_t n, float* out_t, int32_t* out_object,
                  int32_t* out_triangle, float* out_bary /* [n][2] */, float* out_normal /* [n][3] */);

/* Texture coordinates and an image texture for a mesh -- an EXTENSION, opt-in and additive: PTMI_ABI_VERSION stays 5, no existing
 * struct or entry point changes, and a process that never attaches a texture launches the kernels it launched before and renders
 * the same bits.  The new code lives in kernel instances of its own (TEX, which carry the SMOOTH code as well: a flag per mesh row
 * decides per hit), launched only while a mesh of the scene in force has a texture.
 *
 * Limits.  LINEAR FLOAT IMAGES ONLY: texels are linear radiometric factors in binary32; there is no 8-bit format and no sRGB
 * decoding.  ONE texture per mesh, each mesh with its own copy of its image (sharing one image between meshes is not built).
 * NO mip maps and no filtering by footprint: a lookup is one texel (nearest) or four (bilinear) whatever the distance.  An
 * emissive textured mesh is NOT in the emitter guide, as no emissive mesh is.
 *
 * The lookup (csrc/pt_mesh.h: tri_bary, blend_uv, tex_wrap, texel -- one set of functions for the kernels and the host), at a hit of
 * the ray (o, d) on triangle j of a textured mesh; every operation one rounded binary32, no contraction:
 *   1. Barycentrics.  a, b by the triangle test's own expressions on the ray that hit (the same bits the walk computed),
 *      c = (1 - a) - b.
 *   2. Interpolation.  s = ((c s0) + (a s1)) + (b s2), t likewise.  Corner k's (s, t) is uvs[uv_indices[3 j + k]], or
 *      uvs[indices[3 j + k]] when uv_indices == NULL (per-vertex uvs; n_uvs must equal the mesh's n_vertices).
 *   3. Wrap, x being s or t.  REPEAT: x' = x - floorf(x).  CLAMP: x' = fminf(fmaxf(x, 0), 1).  A value that is not >= 0 after that
 *      becomes 0.  x' lies in [0, 1], both ends included; no bit pattern reads outside the image.
 *   4. Texel position.  (s, t) = (0, 0) is the BOTTOM-LEFT corner of the image (OBJ's convention), s runs across a row, and rows
 *      are stored top to bottom, so the row coordinate uses 1 - t'.  Texel centres sit at half-integers.
 *      NEAREST: X = s' (float)width, Y = (1 - t') (float)height, c0 = (int)floorf(X), r0 = (int)floorf(Y); an index equal to the
 *      size wraps to 0 under REPEAT and becomes size - 1 under CLAMP.  The result is texel (r0, c0), bit for bit.
 *      BILINEAR: X = s' width - 0.5, Y = (1 - t') height - 0.5 (a product, then a difference); c0 = floorf(X), fx = X - c0,
 *      c1 = c0 + 1, rows the same way with fy.  Each index is wrapped (-1 becomes size - 1, size becomes 0) or clamped by the mode.
 *      Per channel top = fmaf(fx, t01 - t00, t00), bot = fmaf(fx, t11 - t10, t10), out = fmaf(fy, bot - top, top) with txy the
 *      texel of row ry, column cx: the environment map's lerp.
 *   5. Effect.  The texel multiplies the row's colour, one multiply per channel, before the material branch: the effective R is
 *      colour[0] x texel.R, G and B likewise.  Diffuse: the factor.  Refractive: the tint of a refracted ray.  Emissive: the
 *      emitted radiance (a textured emissive mesh forms the barycentrics before its early return).  Specular ignores it, as it
 *      ignores its colour.  So a texture of all ones renders the untextured bits, and a constant texture k renders the bits of the
 *      untextured scene with colour fl(colour x k).
 *   6. Feature buffers.  `albedo` of a diffuse or refractive hit on a textured mesh is that product at the centre ray's hit;
 *      everything else is unchanged.  pt_set_mesh_texture invalidates the feature cache.
 *   7. Independence and lifetime.  Textures are independent of normals: a mesh may have either, both or neither.  A mesh WITHOUT a
 *      texture beside a textured one takes none of the steps and renders its own bits.  (h, mesh, NULL) removes the texture.  Any
 *      pt_set_scene* drops all textures with the scene.  A pose change re-expands the uvs into the new slot order, untransformed,
 *      and allocates nothing on the device.  A texture touches neither the worklist, the film, the camera, NIF sharing, the memo
 *      nor the guides: both guides see the textured colour only through the throughput.
 *
 * Copies and memory.  The library copies everything.  The handle keeps the (s, t) per corner in triangle order, 24 bytes per
 * triangle of a textured mesh.  The device holds 24 bytes per triangle SLOT in leaf order, indexed by the global slot a hit
 * carries: one buffer over the slots of ALL meshes of the scene, allocated whole by the first call that attaches a texture,
 * together with a 1 KiB table of per-row descriptors, and kept until the next scene or pt_destroy (removing the last texture does
 * not free it).  It also holds 16 bytes per texel (B, G, R, 0), each mesh its own copy, freed when the texture is removed or
 * replaced.  pt_mesh_texture_info.device_bytes is THIS MESH'S SHARE: 24 per triangle + 16 per texel while it has a texture, else 0.
 * On PT_ERR_OUT_OF_MEMORY the mesh keeps what it had.
 *
 * Validation returns PT_ERR_INVALID_ARGUMENT, and pt_last_error names mesh, triangle, corner, texel and field.  The checks run in
 * this order, before any device call: a NULL handle (pt_last_error(NULL)); no mesh `mesh` in force; struct_size; width or height
 * outside 1..PT_MESH_TEXTURE_MAX_SIZE; filter, then wrap, out of range; NULL bgr, then NULL uvs; n_uvs different from n_vertices
 * when uv_indices is NULL; a texel that is not finite or is negative, naming row, column and channel, in storage order; then per
 * triangle and corner an index >= n_uvs or a referenced uv that is not finite.  Unreferenced uvs are not examined.  After a
 * rejection the mesh keeps what it had. */
enum { PT_TEX_FILTER_NEAREST = 0, PT_TEX_FILTER_BILINEAR = 1 };
enum { PT_TEX_WRAP_REPEAT = 0, PT_TEX_WRAP_CLAMP = 1 };
#define PT_MESH_TEXTURE_MAX_SIZE 8192
typedef struct pt_mesh_texture {      /* 56 bytes */
  uint32_t struct_size;               /* sizeof(pt_mesh_texture) */
  uint32_t width, height;             /* 1..PT_MESH_TEXTURE_MAX_SIZE */
  int32_t filter, wrap;
  const float* bgr;                   /* [height][width][3] float32, B,G,R, rows top to bottom, linear values, finite and >= 0 */
  const float* uvs;                   /* [n_uvs][2] (s, t), finite */
  uint32_t n_uvs;
  const uint32_t* uv_indices;         /* [n_triangles][3] per corner (OBJ's v/vt), or NULL: per vertex, n_uvs == n_vertices */
} pt_mesh_texture;
int pt_set_mesh_texture(pt_handle h, uint32_t mesh, const pt_mesh_texture* t);   /* NULL removes it */
typedef struct pt_mesh_texture_info { /* 40 bytes */
  uint32_t struct_size;               /* in: sizeof(pt_mesh_texture_info) */
  uint32_t has_texture;               /* 1: the mesh is textured */
  uint32_t per_corner;                /* 1: given with uv_indices */
  uint32_t width, height;
  int32_t filter, wrap;
  uint32_t n_uvs;                     /* as given */
  uint64_t device_bytes;              /* this mesh's share: 24 per triangle + 16 per texel while it has a texture, else 0 */
} pt_mesh_texture_info;
int pt_get_mesh_texture_info(pt_handle h, uint32_t mesh, pt_mesh_texture_info* out);
/* Kernel-level hook, like pt_mesh_shade: world-space rays, the camera IGNORED.  The textured instances' own nearest hit, uv
 * interpolation and lookup.  out_t, out_object, out_triangle as pt_mesh_intersect's.  For a hit on a triangle of a textured mesh
 * out_uv[i] is the interpolated (s, t) of rule 2 and out_bgr[i] the texel of rule 4, NOT multiplied by the row's colour; for a
 * mesh triangle without a texture uv is 0 and bgr is (1, 1, 1); for a miss or a hit on anything else both are 0.
 * PT_ERR_NOT_READY without a mesh in force; n == 0 is a no-op. */
int pt_mesh_texel(pt_handle h, const float* origin, const float* dir, size_t n, float* out_t, int32_t* out_object,
                  int32_t* out_triangle, float* out_uv /* [n][2] */, float* out_bgr /* [n][3] */);

/* Mesh trees built and refitted on the device -- an EXTENSION, opt-in and additive: PTMI_ABI_VERSION stays 5, no existing struct
 * moves, no trace kernel is added or changed, and a process that never calls pt_set_mesh_build runs the host builder and the
 * rebuild on every pose change that it ran before, call for call.
 *
 * Options.  builder says who builds a scene's trees: PT_MESH_BUILDER_HOST (binned SAH on one host thread, as above) or
 * PT_MESH_BUILDER_DEVICE (a linear BVH built by kernels on the handle's stream).  on_pose says what a change of frame does to
 * trees that exist: PT_MESH_POSE_REBUILD builds them again, PT_MESH_POSE_REFIT keeps topology and slot order and refits.  The
 * options belong to the handle and survive pt_set_scene*.  A change of builder makes the trees of the scene in force stale: they
 * are built again before whatever traces next; a change of on_pose alone makes nothing stale.  NULL options: the defaults,
 * HOST + REBUILD.  Validation, in this order, before any device call, pt_last_error naming the field: struct_size, builder,
 * on_pose, then a NULL handle (pt_last_error(NULL)).
 *
 * Memory.  While builder is DEVICE or on_pose is REFIT the handle holds, for the scene in force, the world frames on the device
 * (48 bytes per triangle), triangle-order copies of the corner normals (36) and uvs (24) once a mesh has them, and the builder's
 * arrays for the LARGEST mesh: keys and indices before and after the sort (24 per triangle), parents, ranges and counters (44),
 * 16 bytes per mesh, and the sort's histograms (1 KiB per 1024 triangles).  All of it is allocated by pt_set_mesh_build (for the scene in force), by
 * every pt_set_scene_meshes under such an option, and by pt_set_mesh_normals / pt_set_mesh_texture for what they add, so a build
 * or a refit allocates no device memory and, as above, cannot run out of it.  PT_ERR_OUT_OF_MEMORY leaves the previous options,
 * or the previous scene, in force.  pt_mesh_build_info.device_bytes reports the sum; it is given back with the scene.
 *
 * The device builder (csrc/pt_mesh_build.h states the rule; ONE set of functions for the kernels, the sequential reference
 * builder and the test program).  Triangles are ordered by the 63-bit Morton code of their boxes' centres (21 bits per axis over
 * the centres' bounds, ties by triangle index); a range of more than four keys splits at the highest differing bit of its first
 * and last key (equal codes: of their sorted positions), a range of at most four is a leaf.  Layout, boxes and pad are exactly the
 * host builder's.  The keys are sorted on the device by the library's own stable radix sort (sort_on_device = 1; a build that
 * had to sort them on the host would report 0: the same order, the same tree).  After pt_set_scene_meshes, pt_set_mesh_normals
 * and pt_set_mesh_texture have uploaded their triangle-order copies no per-triangle data crosses to or from the host.
 * TREE QUALITY IS BELOW SAH.  On the host walk over the test program's rays, box tests per ray rose from 47.4 to 53.6 (+13 %) on
 * icosphere4, 29.8 to 45.0 (+51 %) on grid and 60.8 to 69.9 (+15 %) on sliver; triangle tests rose by 4 %, 26 % and 4 %.  With
 * camera rays on icospheres of 82 k to 1.3 M triangles box tests moved by +5 %, +5 % and -1 %.  THE RESULT OF A TRACE DOES NOT
 * DEPEND ON THE TREE: the tie rule lives in the walk, so the device builder and the refit render the host tree's bits.  That
 * promise is as empirical as the one above: the pad is a margin, not a proof.
 *
 * Refit.  Under PT_MESH_POSE_REFIT, whenever trees of the same triangles by the builder in force lie on the device and only the
 * frame changes -- pt_set_camera, and the world-frame switch that pt_mesh_intersect, pt_mesh_shade and pt_mesh_texel force -- the
 * kernel frames are formed again from the device copy of the world frames and written into the unchanged slot order; every leaf
 * box is recomputed from its triangles' boxes and every inner box from its two children; the pad is computed from the new root
 * box and applied by the builder's own expressions.  n_nodes, depth, max_leaf, skips, leaf words and the slot -> triangle map do
 * not change; corner normals go through the direction transform into the same slots; uvs are not touched.  It serves host-built
 * (SAH) and device-built topology alike.  The first build of a scene, a build after a change of builder, and the build after
 * pt_set_mesh_normals or pt_set_mesh_texture are always builds.
 *
 * pt_mesh_info under the device paths: build_ms is the DEVICE time of that mesh's last build or refit (HIP events on the handle's
 * stream); n_nodes, depth, max_leaf and pad are read back from the device, four words per mesh.
 *
 * pt_mesh_tree is a kernel-level hook like pt_get_env_guide_tables: it brings the trees up to date for the camera in force,
 * exactly as a render would, then copies mesh `mesh`'s nodes as the kernels read them (padded boxes, skip, leaf word;
 * pt_mesh_info.n_nodes of them) and its slot -> triangle map (n_triangles words).  A NULL pointer with capacity 0 means "not
 * wanted"; a capacity that is too small (or a NULL pointer with a capacity) is PT_ERR_INVALID_ARGUMENT; without a mesh in force
 * it is PT_ERR_NOT_READY. */
enum { PT_MESH_BUILDER_HOST = 0, PT_MESH_BUILDER_DEVICE = 1 };
enum { PT_MESH_POSE_REBUILD = 0, PT_MESH_POSE_REFIT = 1 };
typedef struct pt_mesh_build_options { /* 12 bytes */
  uint32_t struct_size;               /* sizeof(pt_mesh_build_options) */
  int32_t builder;                    /* PT_MESH_BUILDER_* */
  int32_t on_pose;                    /* PT_MESH_POSE_* */
} pt_mesh_build_options;
int pt_set_mesh_build(pt_handle h, const pt_mesh_build_options* o);   /* NULL: the defaults, HOST + REBUILD */
enum { PT_MESH_LAST_NONE = 0, PT_MESH_LAST_HOST_BUILD = 1, PT_MESH_LAST_DEVICE_BUILD = 2, PT_MESH_LAST_REFIT = 3 };
typedef struct pt_mesh_build_info {   /* 64 bytes */
  uint32_t struct_size;               /* in: sizeof(pt_mesh_build_info) */
  int32_t builder, on_pose;           /* the options in force */
  uint32_t sort_on_device;            /* 1: the device builder sorts its keys on the device */
  uint64_t host_builds, device_builds, refits;   /* passes over the scene's meshes since pt_create */
  int32_t last_kind;                  /* PT_MESH_LAST_*: the last pass */
  uint32_t reserved;
  double last_ms;                     /* its time over all meshes: host time, or for device work HIP events on the handle's stream */
  uint64_t device_bytes;              /* held for the device paths (0 unless an option asked for them) */
} pt_mesh_build_info;
int pt_get_mesh_build_info(pt_handle h, pt_mesh_build_info* out);
typedef struct pt_mesh_node {         /* 32 bytes: a node as the kernels read it (csrc/pt_mesh.h) */
  float lo[3], hi[3];                 /* the padded box, in the kernel's frame */
  uint32_t skip;                      /* the node to continue at after a miss or a leaf; n_nodes ends the walk */
  uint32_t leaf;                      /* first slot << 3 | count; 0: an inner node, its left child at node + 1 */
} pt_mesh_node;
int pt_mesh_tree(pt_handle h, uint32_t mesh, pt_mesh_node* nodes, uint32_t node_capacity, uint32_t* orig, uint32_t orig_capacity);

/* SAH trees built on the device -- an EXTENSION, opt-in and additive: PTMI_ABI_VERSION stays 5, no existing struct or enum moves,
 * no trace kernel is added or changed, and a process that never calls pt_set_mesh_device_tree builds what it built before.
 *
 * The option.  kind says WHICH tree PT_MESH_BUILDER_DEVICE builds: PT_MESH_DEVICE_TREE_LINEAR (the default: the linear BVH above,
 * of which "tree quality is below SAH" stays true) or PT_MESH_DEVICE_TREE_SAH.  The kind belongs to the handle and survives
 * pt_set_scene*, as the build options do.  Under PT_MESH_BUILDER_HOST it is accepted and inert.  A change of kind while builder
 * is DEVICE makes the trees of the scene in force stale, exactly as a change of builder does: they are built again before
 * whatever traces next, and no refit keeps a tree of the other kind.  Validation, in this order, before any device call: kind
 * ("pt_set_mesh_device_tree: kind must be 0 (linear) or 1 (sah) (got N)"), then a NULL handle; both through pt_last_error(NULL)
 * when the handle is NULL.
 *
 * The rule.  The tree of PT_MESH_DEVICE_TREE_SAH IS the host builder's (ptmesh::build, csrc/ptmi_mesh.h) of the same kernel-frame
 * triangles, byte for byte: the nodes (padded boxes, skip, leaf word), the slot -> triangle map, n_nodes, depth, max_leaf and pad.
 * It can be, because the host builder's reductions are min / max and integer counts (exact in any order), its cost scan is a
 * fixed loop with strict <, its partition is stable, and library and test programs are compiled with -ffp-contract=off.
 * csrc/pt_mesh_sah.h states the rule and its parallel form -- breadth-first over the open ranges of one index array; per level:
 * centroid bounds and 3 x 16 bins per open range by integer atomics on order-preserving words, one thread per range for the two
 * scans, and a stable partition by a prefix sum of the goes-left flags -- ONE set of functions for the kernels and the test
 * program (tests/mesh_sah_main.cpp).  The host reads two words per level (the next level's range counts) and stops when no range
 * is open; last_levels reports how many levels the last build ran (the tree's depth - 1).  The depth cap of 48 is the host's;
 * 48 levels are out of reach of small valid fixtures in binary32, so the test program exercises the cap at 2 and 3.
 * Everything traced through such a tree is what the host builder's tree gives: they are the same bytes.
 *
 * Where it applies.  Every build PT_MESH_BUILDER_DEVICE runs: pt_set_scene_meshes, a pose change under PT_MESH_POSE_REBUILD, the
 * build after pt_set_mesh_normals / pt_set_mesh_texture, and pt_update_mesh_vertices(..., PT_MESH_UPDATE_REBUILD), which rebuilds
 * that one mesh.  Refits keep the SAH topology (the refit above serves any depth-first tree).
 *
 * Counters.  A SAH device build counts in pt_mesh_build_info.device_builds with last_kind == PT_MESH_LAST_DEVICE_BUILD, and in
 * sah_builds here; last_ms is that pass's device time.
 *
 * Memory.  While the kind is SAH under a device option (builder DEVICE or on_pose REFIT) the handle holds, beside the above, the
 * SAH builder's arrays for the LARGEST mesh: about 143 BYTES PER TRIANGLE -- boxes (24), two index arrays and two range maps (16),
 * the flags' prefix sums (4), six words per node for 2 T nodes (48), the open lists and splits of a level (44 per 5 triangles)
 * and a 1368-byte bin table per 33 triangles (42).  They are allocated by pt_set_mesh_device_tree for the scene in force, by
 * pt_set_mesh_build when it turns a device option on under the kind, and at every pt_set_scene_meshes under both; a build
 * allocates nothing.  PT_ERR_OUT_OF_MEMORY leaves the previous kind, or the previous scene, in force.  device_bytes reports the
 * addition (pt_mesh_build_info.device_bytes includes it); it is given back with the scene.  The builder is written for
 * meshes of at most PT_MAX_MESH_TRIANGLES (2^22) triangles, which is all a scene can hold. */
enum { PT_MESH_DEVICE_TREE_LINEAR = 0, PT_MESH_DEVICE_TREE_SAH = 1 };
int pt_set_mesh_device_tree(pt_handle h, int32_t kind);        /* which tree PT_MESH_BUILDER_DEVICE builds; default LINEAR */
typedef struct pt_mesh_device_tree_info { uint32_t struct_size; int32_t kind; uint64_t sah_builds;
  uint32_t last_levels, reserved; double last_ms; uint64_t device_bytes; } pt_mesh_device_tree_info;   /* 40 bytes */
int pt_get_mesh_device_tree_info(pt_handle h, pt_mesh_device_tree_info* out);

/* Animated meshes: one mesh's vertices replaced on the device and its tree refitted or rebuilt -- an EXTENSION, opt-in and
 * additive: PTMI_ABI_VERSION stays 5, no existing struct moves, no trace, NIF, sharing or accumulate kernel is added or changed,
 * and a process that never calls pt_update_mesh_vertices launches what it launched before, call for call.
 *
 * What it does.  pt_update_mesh_vertices gives mesh `mesh` of the scene in force new vertex positions (and, optionally, new
 * normals).  TOPOLOGY DOES NOT CHANGE: the indices, the triangle count and n_vertices are the mesh's own, and only whole-array
 * updates are supported.  The other meshes (nodes, slots, normals, uvs), this mesh's uvs and texture, the scene table and the
 * camera are not touched.  The mesh then renders, bit for bit, what a fresh handle renders after pt_set_scene_meshes with the
 * new vertices (plus pt_set_mesh_normals / pt_set_mesh_texture as attached): the result of a trace does not depend on the tree.
 *
 * On the device (csrc/pt_mesh_update.h states the rule; ONE set of functions for the kernels, the host and the test program).
 * One kernel forms every triangle's frame -- e1 = v1 - v0, e2 = v2 - v0, c = cross(e1, e2), n = c / sqrtf(dot(c, c)), every
 * operation one rounded binary32, the bytes pt_set_scene_meshes computes on the host -- and checks it by that call's rules in that
 * call's order: a referenced vertex that is not finite, then vertex differences or a cross product that are not finite, then
 * collinear vertices.  The LOWEST offending triangle is reported.  Only if there is none does a second kernel write the frames
 * (and the normalised corner normals) into the device copies the builder and the refit read.  A REJECTED UPDATE LEAVES EVERY BYTE
 * OF THE GEOMETRY IN FORCE AS IT WAS; pt_last_error names scene object, mesh, triangle and field exactly as pt_set_scene_meshes
 * (for normals: pt_set_mesh_normals) names the same data.
 *
 * The tree.  PT_MESH_UPDATE_REFIT keeps the mesh's topology, slot order, slot -> triangle map and uvs: the kernel frames are formed
 * again in the frame the trees are built for and the boxes and the pad follow, as under PT_MESH_POSE_REFIT.  It serves host-built
 * (SAH) and device-built topology.  A refit never changes what is rendered, but a tree refitted over a large deformation is a
 * worse tree: PT_MESH_UPDATE_REBUILD builds the mesh again by the builder in force (pt_set_mesh_build) -- on the device from the
 * device copy, or on the host from the host copy, which is first brought back from the device.  REFIT needs valid trees: where
 * the trees of the scene are stale (nothing traced since pt_set_mesh_normals, pt_set_mesh_texture or a change of builder) the
 * scene's trees are built instead, as the next trace would have, and pt_mesh_update_info counts a fallback.
 *
 * Normals.  normals != NULL: the mesh must have normals attached and n_normals must equal the attached count; the attached layout
 * (per vertex, or per corner through the normal_indices given to pt_set_mesh_normals, which the handle keeps) is reused, and the
 * new normals are checked and normalised by pt_set_mesh_normals' rules.  normals == NULL (n_normals must be 0) on a mesh with
 * normals KEEPS THE ATTACHED NORMALS AS THEY ARE: whether they still suit the moved surface is the caller's business.
 *
 * Memory.  PT_MESH_UPDATE_HOST_MEMORY: vertices and normals are host arrays, copied before the call returns.
 * PT_MESH_UPDATE_DEVICE_MEMORY: they are device memory on the handle's device; the caller guarantees that every write to them is
 * complete before the call and that they are untouched until it returns; the library copies them device to device into its own
 * staging buffers on the handle's stream and never keeps the pointer.  The first update of a scene allocates, once, and holds until
 * the next pt_set_scene*: the device paths' storage of pt_set_mesh_build if no option asked for it yet, the scene's triangle
 * indices (12 bytes per triangle), a vertex staging buffer for the mesh with the most vertices (12 per vertex) and, for meshes
 * with normals, a normal staging buffer and the per-corner normal indices (12 per triangle).  Later updates allocate nothing
 * (pt_set_mesh_normals in between has the normal buffers sized again at the next update).  PT_ERR_OUT_OF_MEMORY leaves everything
 * as it was.  The handle's streams are drained first; the work runs on the handle's stream and is complete when the call returns.
 *
 * Validation returns PT_ERR_INVALID_ARGUMENT before any device call, in this order, pt_last_error naming the field: struct_size
 * (or a NULL struct), mode, memory, NULL vertices, normals NULL with n_normals > 0 or not NULL with n_normals == 0, then a NULL
 * handle (pt_last_error(NULL)), no mesh `mesh` in force, n_vertices different from the mesh's, normals for a mesh without normals
 * or n_normals different from the attached count; then the device check above.
 *
 * pt_mesh_build_info counts an update's tree pass as a pass (a pass over one mesh is a pass). */
enum { PT_MESH_UPDATE_REFIT = 0, PT_MESH_UPDATE_REBUILD = 1 };
enum { PT_MESH_UPDATE_HOST_MEMORY = 0, PT_MESH_UPDATE_DEVICE_MEMORY = 1 };
typedef struct pt_mesh_update {       /* 40 bytes */
  uint32_t struct_size;               /* sizeof(pt_mesh_update) */
  int32_t mode;                       /* PT_MESH_UPDATE_REFIT / _REBUILD */
  int32_t memory;                     /* PT_MESH_UPDATE_HOST_MEMORY / _DEVICE_MEMORY: where vertices and normals lie */
  uint32_t n_vertices;                /* must equal the mesh's */
  const float* vertices;              /* [n_vertices][3], world space */
  uint32_t n_normals;                 /* 0: keep what is attached (four bytes of padding follow) */
  const float* normals;              /* [n_normals][3] or NULL; indexed as the attached normals are */
} pt_mesh_update;
int pt_update_mesh_vertices(pt_handle h, uint32_t mesh, const pt_mesh_update* u);
typedef struct pt_mesh_update_info {  /* 64 bytes */
  uint32_t struct_size;               /* in: sizeof(pt_mesh_update_info) */
  int32_t last_kind;                  /* PT_MESH_LAST_*: the last update's tree pass */
  uint64_t updates;                   /* accepted updates since pt_create ... */
  uint64_t refits, rebuilds;          /* ... whose tree pass was a refit / a build (updates = refits + rebuilds) */
  uint64_t fallbacks;                 /* of the rebuilds, those that were asked for as PT_MESH_UPDATE_REFIT */
  double last_frames_ms;              /* the last update's copy, check and commit: HIP events on the handle's stream */
  double last_tree_ms;                /* its tree pass (pt_mesh_build_info.last_ms) */
  uint64_t device_bytes;              /* added by the update path for the scene in force (0 before its first update) */
} pt_mesh_update_info;
int pt_get_mesh_update_info(pt_handle h, pt_mesh_update_info* out);

/* Which instance of the trace kernels a launch took -- an EXTENSION, read-only and additive: PTMI_ABI_VERSION stays 5, no existing
 * struct moves and nothing that is launched changes.  The trace kernel, the pt_trace_paths kernel and the feature kernel are each
 * one template instantiated per (camera, bounce, geometry) (csrc/ptmi_trace_variant.h: 57, 19 and 5 instances); the camera, the
 * guides and the scene in force pick the instance at every launch.  pt_get_trace_variant reports what the most recent launch of
 * each family picked, as pt_nif_kernel_name does for the NIF: `trace` the last trace launch of pt_path_trace, `paths` the last
 * pt_trace_paths, `features` the last computation of the feature buffers (pt_feature_buffers, pt_denoise; they are cached, so a
 * call that finds them valid launches nothing and counts nothing).  camera, bounce and geometry are the coordinates the selector
 * computed for that launch (PT_TRACE_CAMERA_*, PT_TRACE_BOUNCE_*, PT_TRACE_GEOMETRY_*: the values of ptvariant::Camera, Bounce and
 * Geometry).  index is the instance's dense number in its family: geometry major, then bounce, then camera, the one invalid pair
 * (LIGHT_GUIDE_PLAMPS, SPHERES) left out -- 0..56 for `trace`; 0..18 for `paths`, whose kernels read the camera at run time;
 * 0..4, the geometry, for `features`, whose kernels ignore the bounce and the lens.  launches counts the family's launches since
 * pt_create.  Before the first launch of a family its camera, bounce, geometry and index are -1 and its count is 0.
 * Validation, in this order: a NULL out, struct_size, then a NULL handle (pt_last_error(NULL)); PT_ERR_INVALID_ARGUMENT each. */
enum { PT_TRACE_CAMERA_BUILTIN = 0, PT_TRACE_CAMERA_POSE = 1, PT_TRACE_CAMERA_LENS = 2 };
enum { PT_TRACE_BOUNCE_PLAIN = 0, PT_TRACE_BOUNCE_ENV_GUIDE = 1, PT_TRACE_BOUNCE_LIGHT_GUIDE = 2, PT_TRACE_BOUNCE_LIGHT_GUIDE_PLAMPS = 3 };
enum { PT_TRACE_GEOMETRY_SPHERES = 0, PT_TRACE_GEOMETRY_POLY = 1, PT_TRACE_GEOMETRY_MESH = 2, PT_TRACE_GEOMETRY_SMOOTH = 3, PT_TRACE_GEOMETRY_TEX = 4 };
typedef struct pt_trace_variant_launch { /* 24 bytes */
  int32_t camera, bounce, geometry;   /* PT_TRACE_CAMERA_*, PT_TRACE_BOUNCE_*, PT_TRACE_GEOMETRY_*; -1 before the first launch */
  int32_t index;                      /* the instance's dense number in its family; -1 before the first launch */
  uint64_t launches;                  /* launches of the family since pt_create */
} pt_trace_variant_launch;
typedef struct pt_trace_variant_info { /* 80 bytes */
  uint32_t struct_size;               /* in: sizeof(pt_trace_variant_info) */
  uint32_t reserved;
  pt_trace_variant_launch trace, paths, features;
} pt_trace_variant_info;
int pt_get_trace_variant(pt_handle h, pt_trace_variant_info* out);

/* Runtime camera -- an EXTENSION: the reference's camera is compile-time, a pinhole at the origin looking down -z with +y up
 * (codelets.cpp:68-75,162-163); only the field of view is a setting.  pt_set_camera gives it a position, an orientation and an
 * optional thin lens.  Additive: PTMI_ABI_VERSION stays 5 and no existing struct moves.
 * Basis, computed once on the host, every intermediate a rounded binary32:
 *   f = normalise(look_at - position), r = normalise(cross(f, up)), u = cross(r, f)    (normalise(v) = v / sqrtf(dot(v, v)))
 * look_at - position and up are first scaled by the power of two that brings their largest component into [0.5, 1): exact, the
 * same bits as without it, and any finite non-zero length is accepted (no overflow or underflow in the squares).
 * A camera-space vector (x, y, z) is the world vector x r + y u - z f; the default camera gives the identity.  The field of
 * view, the AA noise and the half-rounded (camx, camy) are exactly as before (fov and azimuth stay in pt_set_render_settings;
 * the azimuth is added after the direction is in world space).  A camera whose basis is exactly (+x, +y, -z) at position 0
 * IS the built-in one: no transform is applied at all, so it renders bit-identically to no call.
 * Every quantity the ABI reports is in world space: pt_path_record.dir is the world direction of the escaping ray (or of the
 * ray that hit an emitter), uv is PreProcessEscapedRays of that world direction, cam is unchanged (camera space).
 * Thin lens (lens_radius = a > 0, focus_distance = F), in camera space: the focus point is F (camx, camy, -1) -- the focal
 * plane is perpendicular to the view axis --, the lens point is a (sqrt(x1) cos 2 pi x2, sqrt(x1) sin 2 pi x2, 0), and the ray
 * goes from the lens point towards the focus point with weight 1 (throughput starts at (1, 1, 1) as for the pinhole).
 * x1, x2 are words 0 and 1 of Philox block 65 of the path (counter (pixel, sample, 65, 0x5054); AA noise draws block 0 and
 * bounce d block 1 + d <= 64), on the primary-sample grid of pt_config.sample_precision.  With a == 0 no lens block is drawn
 * and F is ignored.
 * Validation: PT_ERR_INVALID_ARGUMENT, the previous camera stays in force and pt_last_error names the field, for a wrong
 * struct_size, any value that is not finite (look_at - position included), look_at == position, up of length zero or parallel to the view direction
 * (|cross(f, up / |up|)| < 1e-3), lens_radius < 0, lens_radius > 0 with focus_distance <= 0, and a NULL handle.  A NULL camera
 * restores the built-in one.
 * A new camera takes effect at the next pt_path_trace / pt_trace_paths.  It does not touch the worklist, the accumulators,
 * the resident film, tile costs, the scene, NIF sharing or the NIF memo: sharing and memo keys are the (u, v) bits after
 * rotation and azimuth, so both stay exact and need no invalidation.
 * pt_get_camera copies the camera in force, values as given (struct_size = sizeof(pt_camera)); h == NULL gives the default
 * and needs no device. */
typedef struct pt_camera {        /* 48 bytes */
  uint32_t struct_size;           /* sizeof(pt_camera), set by the caller */
  float position[3];              /* default (0, 0, 0) */
  float look_at[3];               /* default (0, 0, -1) */
  float up[3];                    /* default (0, 1, 0); need not be unit or orthogonal */
  float lens_radius;              /* 0 = pinhole (default) */
  float focus_distance;           /* distance of the focal plane along the view axis; used when lens_radius > 0 */
} pt_camera;
int pt_set_camera(pt_handle h, const pt_camera* cam);   /* NULL restores the built-in camera */
int pt_get_camera(pt_handle h, pt_camera* out);          /* values as given; h == NULL: the default, needs no device */

/* HDR environment map -- an EXTENSION: an equirectangular image as the environment light, the third kind next to the NIF and
 * the constant radiance.  The reference renders with a NIF trained on such an image (its README: "source an
 * equirectangular-projection HDRI image"); here the image itself can be the light.  Additive: PTMI_ABI_VERSION stays 5.
 * `bgr` is [height][width][3] float32 in host memory, B, G, R order, rows top to bottom (what the NIF decodes to and what
 * AccumulatedImage holds).  The library keeps a device copy of one float4 (B, G, R, 0) per texel (16 bytes per texel: 128 MiB
 * for 4096 x 2048) and retains no host pointer.
 * Mapping: u runs down the image and v across it (PreProcessEscapedRays, codelets.cpp:333-347; the azimuth is folded into v),
 * and texel (row r, column c) sits at u = r / height, v = c / width with no half-texel offset (NifModel::makeGridCoordsUV,
 * NifModel.cpp:474-490): the map is the image a NIF would be trained to reproduce.  Per lookup, in binary32:
 *   u, v are clamped with fminf(fmaxf(., 0), 1) (NaN becomes 0; no bit pattern reads outside the image);
 *   y = u * (float)height, x = v * (float)width;
 *   r0 = (int)floorf(y), fy = y - r0, then r0 = min(r0, height - 1), r1 = min(r0 + 1, height - 1)   (rows clamp at the pole);
 *   c0 = (int)floorf(x), fx = x - c0, then c0 = c0 mod width, c1 = (c0 + 1) mod width              (columns wrap; v == 1 is column 0).
 *   PT_ENV_FILTER_NEAREST   texel (r0, c0), bit for bit.
 *   PT_ENV_FILTER_BILINEAR  per channel top = fmaf(fx, t01 - t00, t00), bot = fmaf(fx, t11 - t10, t10),
 *                           out = fmaf(fy, bot - top, top).
 * A path's radiance is out * throughput, the NIF heads' own single fp32 multiply per channel.
 * pt_set_env_map makes the map the environment; a later pt_upload_nif or pt_set_constant_env replaces it (the last of the three
 * calls wins) and frees the device copy, as does pt_destroy.  It takes effect at the next pt_path_trace and touches neither the
 * worklist, the film, the scene nor the camera.  A step with a map runs the NIF-mode schedule with the map kernel in the NIF
 * stage, so NIF sharing and the NIF memo apply to a map exactly as to a NIF (keys are the (u, v) bits); pt_set_env_map starts a
 * new memo generation.  pt_stats: escaped keeps its meaning, nif_ms / nif_launches count that stage whichever kernel ran it,
 * nif_flops_per_sample is 0; pt_nif_kernel_name reports "envmap_nearest" or "envmap_bilinear"; pt_calibrate_nif answers
 * PT_ERR_NOT_READY as with a constant environment; pt_nif_infer still evaluates the last uploaded NIF.
 * PT_ERR_INVALID_ARGUMENT for a NULL handle or image, width or height outside 1..PT_ENV_MAP_MAX_SIZE, a filter out of range, or
 * a texel that is not finite or is negative (pt_last_error names row, column and channel).  After that or
 * PT_ERR_OUT_OF_MEMORY the previous environment stays in force.
 * pt_env_map_lookup runs the same kernel over n host (u, v) pairs and returns the BGR it looks up, float32 [n][3]:
 * PT_ERR_NOT_READY when no map is the environment; n == 0 is a no-op. */
enum { PT_ENV_FILTER_NEAREST = 0, PT_ENV_FILTER_BILINEAR = 1 };
#define PT_ENV_MAP_MAX_SIZE 16384
int pt_set_env_map(pt_handle h, const float* bgr, uint32_t width, uint32_t height, int32_t filter);
int pt_env_map_lookup(pt_handle h, const float* u, const float* v, size_t n, float* bgr);

/* Environment-guided diffuse sampling -- an EXTENSION, opt-in: a diffuse bounce draws its next direction, with probability
 * alpha, from a distribution that follows the luminance of an HDR image, and otherwise uniformly over the hemisphere as the
 * reference does (codelets.cpp:199-204).  Additive: PTMI_ABI_VERSION stays 5 and no existing struct moves; a process that never
 * calls pt_set_env_guide launches the kernels it launched before and renders the same bits.
 * The guide describes SAMPLING, not light: the estimator stays unbiased for any environment (NIF, map or constant), because the
 * guide only enters as a density that is mixed with the hemisphere's and is therefore positive wherever the integrand is.  A
 * NIF render is typically guided by the image the NIF was trained from.
 * Tables (host, binary64; csrc/ptmi_env_guide.h): the image bgr[height][width][3] (layout and validity rules of pt_set_env_map)
 * is reduced to a grid of rows x cols cells -- both powers of two, rows <= PT_ENV_GUIDE_MAX_ROWS and height, cols <=
 * PT_ENV_GUIDE_MAX_COLS and width.  Cell (i, j) covers u in [i / rows, (i + 1) / rows), v in [j / cols, (j + 1) / cols) (u down the
 * image, v across it); texel (r, c) belongs to cell (floor(r rows / height), floor(c cols / width)) and adds
 * (0.0722 B + 0.7152 G + 0.2126 R) sin(pi (r + 0.5) / height) to its mass.  One alias table (Vose) over the n = rows cols cells,
 * entries {uint32 threshold, uint32 alias}: cell k is kept when a 32-bit word is < threshold[k].  The density table is made from
 * the quantised table: P(cell) = (threshold[cell] + sum over k with alias[k] = cell of (2^32 - threshold[k])) / (n 2^32),
 * q[cell] = P(cell) n / pi (float32), so that g(w) = q[cell(w)] / sin(theta) is 2 pi times the solid-angle density the kernel
 * really draws from.  alpha is used as alpha_thr / 2^32 with alpha_thr = (uint32)(alpha 2^32).
 * A guided diffuse bounce at depth d (first bounce: d = 0) draws Philox block 66 + d of the path, words g0..g3 (blocks 0..64 are
 * the AA noise and the bounces, 65 the lens).  g0 < alpha_thr: k = g1 >> (32 - log2 n), cell = g2 < threshold[k] ? k : alias[k],
 * (i, j) = (cell / cols, cell mod cols), u = (i + ((g3 >> 16) + 0.5) / 65536) / rows, v = (j + ((g3 & 0xffff) + 0.5) / 65536) / cols,
 * theta = pi u, phi = 2 pi v - azimuth, world direction (sin theta cos phi, cos theta, sin theta sin phi) -- the inverse of the
 * escape's direction-to-(u, v) map -- rotated into camera space when a pose is set.  Otherwise: the reference's hemisphere
 * direction from words 1 and 2 of the bounce's own block, unchanged.  Whichever branch gave the direction w: cos = dot(w, n), the
 * cell of w is (min((int)(u rows), rows - 1), (int)(v cols) mod cols) of its (u, v), sin theta = max(sqrtf(1 - y^2), 1e-30f) with y
 * the world y, g = q[cell] / sin theta, and T = T (.) colour x (cos x rr / ((1 - alpha) + alpha g)).  With alpha = 0 the factor is
 * cos x rr / 1: the unguided bits.
 * A guide-branch direction with cos <= 0 ends the path with no contribution.  Length rule: such a path has length d + 1 -- the
 * bounce's own record stands, exactly the length of a path whose contribution stack fills at that bounce -- and it counts in
 * pt_stats.paths, in pt_stats.segments and in TraceRecord pathLength with that length, not in pt_stats.escaped; pt_trace_paths
 * reports it with escaped = 0 and throughput 0.  Mirror, glass, emitters, roulette and the escape are untouched.
 * pt_set_env_guide takes effect at the next pt_path_trace / pt_trace_paths and touches neither the environment, the worklist,
 * the film, the scene, the camera, NIF sharing nor the memo (their keys are (u, v) bits); it survives pt_upload_nif,
 * pt_set_env_map and pt_set_constant_env.  g == NULL clears the guide.  The library keeps the two tables on the device (12 bytes
 * per cell) and retains no host pointer.  PT_ERR_INVALID_ARGUMENT, pt_last_error naming the field, for a NULL handle, a wrong
 * struct_size, a NULL image, a size outside 1..PT_ENV_MAP_MAX_SIZE, a grid that is not powers of two within the caps and the
 * image, alpha outside [0, PT_ENV_GUIDE_MAX_ALPHA], a texel that is not finite or is negative, or an image whose total mass is 0;
 * after that or PT_ERR_OUT_OF_MEMORY the previous guide stays in force.
 * pt_env_guide_sample runs the kernels' own sampling function over n caller word triples: out_uv float32 [n][2], out_cell
 * uint32 [n].  pt_env_guide_eval runs the kernels' own density function over n caller world directions (float32 [n][3], unit
 * length, with the azimuth of pt_set_render_settings): out_cell uint32 [n], out_g float32 [n].  Both: PT_ERR_NOT_READY without
 * a guide; n == 0 is a no-op. */
#define PT_ENV_GUIDE_MAX_ROWS 1024
#define PT_ENV_GUIDE_MAX_COLS 2048
#define PT_ENV_GUIDE_MAX_ALPHA 0.9f
typedef struct pt_env_guide {
  uint32_t struct_size;          /* = sizeof(pt_env_guide) */
  uint32_t width, height;        /* of the image */
  uint32_t rows, cols;           /* of the grid */
  float alpha;                   /* probability of the guide branch, 0 .. PT_ENV_GUIDE_MAX_ALPHA */
  const float* bgr;              /* [height][width][3], host memory */
} pt_env_guide;
int pt_set_env_guide(pt_handle h, const pt_env_guide* g);   /* NULL clears the guide */
int pt_env_guide_sample(pt_handle h, const uint32_t* g1, const uint32_t* g2, const uint32_t* g3, size_t n, float* out_uv,
                        uint32_t* out_cell);
int pt_env_guide_eval(pt_handle h, const float* dir_world, size_t n, uint32_t* out_cell, float* out_g);

/* The environment guide built from the environment in force -- the NIF, the map or the constant -- with no image in host memory:
 * a render from shipped NIF assets, from a NIF made by pt_nif_train_install or after a hot swap can be guided.  Additive:
 * PTMI_ABI_VERSION stays 5, no existing struct moves, no trace, NIF or accumulate kernel changes and the tables keep their format.
 * DEFINITION (the contract).  With S = supersample, the guide is pt_set_env_guide of the image I of height rows S and width
 * cols S, same rows, cols and alpha, where
 *   I[r][c] = the environment in force looked up at u = ((float)r + 0.5f) / (float)(rows S), v = ((float)c + 0.5f) / (float)(cols S)
 * (both exact in binary32: the divisors are powers of two; the guide's cells live in the post-azimuth (u, v) square the
 * environment is defined on, so the azimuth does not enter).  The lookup is the NIF stage's own: for a NIF the value
 * pt_nif_infer gives, whichever kernel family the model dispatches to; for a map the value pt_env_map_lookup gives with the
 * filter in force; for a constant the rgb of pt_set_constant_env as (B, G, R) = (rgb[2], rgb[1], rgb[0]).  Each channel x of the
 * result is then clamped, x' = x >= 0 ? fminf(x, FLT_MAX) : 0 -- NaN and negative values become 0, +inf becomes FLT_MAX (a
 * NIF's decode can give any of them) -- and `clamped` counts the channel values this replaced.
 * Masses, the total, the alias table, P and q follow from I by the rules of pt_set_env_guide (csrc/ptmi_env_guide.h) in the same
 * binary64 arithmetic in the same order: a sample adds ((0.0722 B + 0.7152 G) + 0.2126 R) sin(pi (r + 0.5) / (rows S)) -- the
 * sine table comes from the host --, a cell adds its S^2 samples one after the other in row-major order, the total adds the
 * cells in cell order.  Host and device are compiled without contraction, so the two routes agree BIT FOR BIT in threshold,
 * alias and q.  The masses are summed on the device (csrc/pt_env_guide_build.h), one sub-sample plane at a time: S^2 launches of
 * the NIF stage over dense queues of rows cols entries, device memory bounded by one plane.
 * Validation: PT_ERR_INVALID_ARGUMENT, pt_last_error naming the field, checked in this order before any device call: a NULL
 * struct, struct_size, rows, cols (powers of two within the caps), supersample (1, 2 or 4), alpha (0 .. PT_ENV_GUIDE_MAX_ALPHA),
 * follow (0 or 1), a NULL handle (the message is then pt_last_error(NULL)'s), alpha + beta against a light guide already set.
 * PT_ERR_NOT_READY: no environment has ever been set (none of pt_upload_nif, pt_set_env_map, pt_set_constant_env).
 * PT_ERR_INVALID_ARGUMENT naming the total: the environment's total mass is 0.  After any failure, PT_ERR_OUT_OF_MEMORY
 * included, the previous guide stays in force.
 * The call changes nothing else: not the worklist, the film or the feature cache; it bypasses NIF sharing and the memo (their
 * stats do not move, no new memo generation); pt_get_stats, pt_nif_kernel_name and the replay state of pt_calibrate_nif stay as
 * they were.  pt_set_env_guide(image) replaces such a guide and turns follow off; pt_set_env_guide(NULL) clears it.
 * follow = 1: every successful pt_upload_nif, pt_set_env_map, pt_set_constant_env and pt_nif_train_install rebuilds the tables
 * from the new environment before it returns, with the same rows, cols, S and alpha; its own return value is unaffected.  If
 * the rebuild fails (a black constant, out of memory) the old tables stay and `stale` is 1 -- a stale guide is still unbiased --
 * until the next successful build.  With follow = 0, or a guide set from an image, those calls do what they always did.
 * pt_get_env_guide_info reports the guide in force (struct_size set by the caller; supersample is 0 for a guide from an image).
 * pt_get_env_guide_tables copies the tables the device holds: PT_ERR_NOT_READY without a guide, PT_ERR_INVALID_ARGUMENT unless
 * n == rows cols. */
typedef struct pt_env_guide_auto {
  uint32_t struct_size;   /* sizeof(pt_env_guide_auto) */
  uint32_t rows, cols;    /* powers of two, <= PT_ENV_GUIDE_MAX_ROWS / _COLS */
  uint32_t supersample;   /* S: 1, 2 or 4 samples per cell edge */
  float    alpha;         /* 0 .. PT_ENV_GUIDE_MAX_ALPHA */
  int32_t  follow;        /* 0 | 1: rebuild when the environment is replaced */
} pt_env_guide_auto;
int pt_set_env_guide_from_environment(pt_handle h, const pt_env_guide_auto* a);

typedef struct pt_env_guide_info {
  uint32_t struct_size;          /* sizeof(pt_env_guide_info), set by the caller */
  int32_t  set, source;          /* source: 0 = image (pt_set_env_guide), 1 = environment */
  uint32_t rows, cols, supersample;
  float    alpha;                /* alpha_thr / 2^32 */
  int32_t  follow, stale;
  uint64_t rebuilds, clamped;    /* builds from the environment so far; channel values replaced in the last one */
  double   build_ms;             /* device time of the last build from the environment (HIP events) */
} pt_env_guide_info;
int pt_get_env_guide_info(pt_handle h, pt_env_guide_info* out);
/* threshold, alias uint32 [n], q float32 [n], n = rows * cols; any pointer may be NULL */
int pt_get_env_guide_tables(pt_handle h, uint32_t* threshold, uint32_t* alias, float* q, size_t n);

/* Emitter-guided diffuse sampling -- an EXTENSION, opt-in: a diffuse bounce draws its next direction, with probability beta,
 * towards an emissive sphere or disc of the scene (the visible cone of a sphere, a uniform point of a disc), and divides by the
 * mixture density at the direction it took.  No shadow ray and no second contribution: an occluded lamp direction hits the
 * occluder and the path goes on, so the estimator is unbiased for any scene and environment.  Additive: PTMI_ABI_VERSION stays 5
 * and no existing struct moves; a process that never calls pt_set_light_guide launches the kernels it launched before and
 * renders the same bits, and so does one whose guide is inert (below) or has beta = 0.
 * Table (host, binary64; csrc/ptmi_light_guide.h): the emitters are the objects of the scene in force with
 * PT_MATERIAL_EMISSIVE, in declaration order, rank k = 0 .. K - 1.  Mass m_k = Y(colour_k) a_k, Y = 0.2126 R + 0.7152 G + 0.0722 B,
 * a_k = 4 r^2 (sphere) or 2 r^2 (disc).  Thresholds c_k = floor(2^32 sum_{j<=k} m_j / sum m) (uint32) before the last emitter of
 * positive mass; that one takes the rest (from it on the reported threshold is 0xffffffff).  A 32-bit word g1 selects the first k
 * with g1 < c_k, else that last emitter.  p_k = (c_k - c_{k-1}) / 2^32 from the integers (the last: (2^32 - c_{k-1}) / 2^32),
 * rounded to float32 once: sum p_k = 1, and an emitter with p_k = 0 is never selected and adds nothing to the density.  If the
 * scene has no emitter, or none of positive mass, the guide is accepted but INERT: the library launches what it would launch
 * without it.  The table is rebuilt by pt_set_light_guide and by every pt_set_scene while a guide is set; the camera does not
 * change it.  beta is used as beta_thr / 2^32, beta_thr = (uint32)(beta 2^32).
 * An emissive polygon (pt_set_scene_ex) is skipped by the table unless pt_set_light_guide_ex asks for polygons (n_lights and
 * object_index say so): it is still reached by the hemisphere and environment branches, and the estimator stays unbiased because
 * the guide is only a density mixed with the hemisphere's.
 * Estimator (device, binary32, every operation rounded once, no contraction; csrc/pt_light_guide.h), in the kernel's frame, at
 * the hit point x with the normal n as the bounce forms them (a disc's stored normal is not flipped):
 *   eligible(k), sphere (c, r): v = c - x, D2 = v.v; D2 > r^2 and v.n + r > 0.
 *   eligible(k), disc (c, m, R): v = c - x, hgt = v.m; |hgt| > 1e-5 and v.n + R sqrtf(fmaxf(0, 1 - (n.m)(n.m))) > 0.
 *   P_E = sum of p_k over the eligible k, in declaration order.
 *   x1 = ((float)(g2 >> 8) + 0.5f) 2^-24, x2 = (float)(g3 >> 8) 2^-24, (sn, cs) = sincos(2 pi x2).
 *   sphere draw: s2 = r^2 / D2, cm = sqrtf(1 - s2), a = v (1 / sqrtf(D2)), (rx, ry) the hemisphere draw's basis about a,
 *     ct = 1 - (x1 s2) / (1 + cm), st = sqrtf(fmaxf(0, 1 - ct ct)), w = rx (cs st) + ry (sn st) + a ct (per component the dot
 *     product ((rx, ry, a) . (cs st, sn st, ct)) left to right); own term g_k = (1 + cm) / s2.
 *   sphere density of any w: (1 + cm) / s2 if w.a >= cm, else 0.
 *   disc draw: (t1, t2) that basis about m, rho = R sqrtf(x1), y = c + (t1 (rho cs) + t2 (rho sn)), e = y - x, l2 = e.e,
 *     l = sqrtf(l2), w = e (1 / l); own term g_k = (2 (l2 l)) / (|hgt| R^2).
 *   disc density of any w: dn = m.w; if dn != 0, t = hgt / dn > 1e-5 and not (|x + t w - c|^2 > R^2): (2 (t t)) / (|dn| R^2), else 0.
 * THE RIM RULE: a direction drawn from emitter k takes k's own term by construction and does not run k's inside test; the test
 * is used for every other emitter, and for all of them when the direction came from the hemisphere or the environment guide.
 * A guided diffuse bounce at depth d draws Philox block 66 + d, words g0..g3 -- the environment guide's block: the branches are
 * exclusive and share the words.  alpha_thr is the environment guide's (0 without one).  g0 < alpha_thr: the environment branch,
 * exactly as pt_set_env_guide states it.  Else g0 < alpha_thr + beta_thr: the light branch; k selected by g1; if k is eligible
 * w is drawn from it, else w is the hemisphere direction from words 1 and 2 of the bounce's own block (the fallback).  Else
 * that hemisphere direction.  Whichever gave w: cos = w.n,
 *   den = (one_minus + alpha g_env(w)) + beta ((1 - P_E) + sum over eligible k, in declaration order, of p_k g_k(w)),
 *   T = T (.) colour x ((cos x rr) / den),
 * one_minus = (float)(1 - (alpha_thr + beta_thr) / 2^32), the environment term present only with an environment guide.
 * A direction drawn from an emitter (not a fallback) or from the environment guide with cos <= 0 ends the path with no
 * contribution, under the environment guide's length rule: length d + 1, counted in paths, segments and pathLength, not in
 * escaped; pt_trace_paths reports escaped = 0 and throughput 0.
 * pt_set_light_guide takes effect at the next pt_path_trace / pt_trace_paths; it survives pt_upload_nif, pt_set_env_map,
 * pt_set_constant_env and pt_set_camera, follows pt_set_scene, and touches neither the worklist, the film, the features, NIF
 * sharing nor the memo.  g == NULL clears it.  PT_ERR_INVALID_ARGUMENT, pt_last_error naming the field, checked in this order
 * before any device call: a wrong struct_size; beta not finite or outside [0, PT_LIGHT_GUIDE_MAX_BETA]; alpha + beta >
 * PT_LIGHT_GUIDE_MAX_BETA (+ 1e-6 for the rounding of the two floats) against an environment guide already set (pt_set_env_guide checks the same sum from its side while a
 * light guide is set); a NULL handle.  After a rejection the previous guide stays in force.
 * pt_get_light_guide_info: set, active (set and not inert), beta as used, and the table over all K emitters.
 * pt_light_guide_sample runs the kernels' own selection and draw over n caller items in WORLD space against the world-space
 * scene table: origin, normal float32 [n][3], words g1, g2, g3; out_dir float32 [n][3] and out_light the rank drawn from, or -1
 * (and direction 0) where the selected emitter is not eligible.  pt_light_guide_eval runs the kernels' own density over caller
 * (origin, normal, unit direction) triples with the inside test for every emitter: out_sum = sum over eligible k of p_k g_k,
 * out_pe = P_E.  Both: PT_ERR_NOT_READY without an active guide; n == 0 is a no-op. */
#define PT_LIGHT_GUIDE_MAX_BETA 0.9f
typedef struct pt_light_guide {
  uint32_t struct_size;          /* = sizeof(pt_light_guide) */
  float beta;                    /* probability of the light branch, 0 .. PT_LIGHT_GUIDE_MAX_BETA */
} pt_light_guide;
int pt_set_light_guide(pt_handle h, const pt_light_guide* g);   /* NULL clears the guide */
/* Polygon lamps -- an EXTENSION of the emitter guide, opt-in: pt_set_light_guide_ex with PT_LIGHT_GUIDE_POLYGONS lists emissive
 * triangles and parallelograms (pt_set_scene_ex) in the table too, in declaration order together with spheres and discs, and
 * guided bounces draw a uniform point of their area.  Additive: PTMI_ABI_VERSION stays 5 and no existing struct moves;
 * pt_set_light_guide(h, g) is pt_set_light_guide_ex with flags = 0, an emissive polygon is then still skipped, and a process
 * that never sets the flag launches the kernels it launched before and renders the same bits.  So does one that sets it over a
 * scene whose emitters are all spheres and discs (the flag survives such a scene and applies again when polygons return).
 * Table: a polygon v0 + a e1 + b e2, e1 = v1 - v0, e2 = v2 - v0, has S = sqrtf(dot(c, c)), c = cross(e1, e2), the binary32
 * value its stored normal was divided by (world space), area A_p = S (parallelogram) or 0.5 S (triangle) and the binary64 mass
 * m_k = Y(colour_k) 2 A_p / pi: two faces, and the pi the masses 4 r^2 and 2 r^2 dropped.  Thresholds and p_k follow as above.
 * Estimator, with m the stored normal, kTwoPi = 2 kPi in binary32, every operation one rounded binary32, left to right:
 *   eligible(k), polygon: v = v0 - x, hgt = v.m, d0 = v.n, d1 = e1.n, d2 = e2.n; reach = fmaxf(0, fmaxf(d1, d2)) (triangle) or
 *     fmaxf(0, d1) + fmaxf(0, d2) (parallelogram); |hgt| > 1e-5 and d0 + reach > 0: some corner is above the horizon.
 *   polygon draw: a = x1, b = x2; triangle only: if a + b > 1 then a = 1 - a, b = 1 - b; y = v0 + (e1 a + e2 b), e = y - x,
 *     l2 = e.e, l = sqrtf(l2), w = e (1 / l); own term g_k = (kTwoPi (l2 l)) / (|hgt| A_p).
 *   polygon density of any w: t = the tracer's own polygon intersection of the ray (x, w), epsilon included; t == 0 -> 0;
 *     dn = m.w; dn == 0 -> 0; else (kTwoPi (t t)) / (|dn| A_p): positive exactly where a ray would hit.
 * The rim rule, the denominator, the cos <= 0 rule and its length rule, the fallback of an ineligible selection and the
 * combination with the environment guide are those of pt_set_light_guide; at a diffuse polygon hit n is the flipped normal.
 * S is not recomputed under a camera (a rotation would change its bits): the kernels receive the world-space value.
 * PT_ERR_INVALID_ARGUMENT, pt_last_error naming the field, checked in this order before any device call: a wrong struct_size;
 * beta not finite or outside [0, PT_LIGHT_GUIDE_MAX_BETA]; a flags bit other than PT_LIGHT_GUIDE_POLYGONS; alpha + beta against
 * an environment guide already set (the rule and slack above); a NULL handle.  After a rejection the previous guide and its
 * flags stay in force.  pt_get_light_guide_info, pt_light_guide_sample and pt_light_guide_eval cover the polygon ranks while
 * the flag is set.  pt_get_light_guide_flags: the flags of the guide in force, 0 without one. */
enum { PT_LIGHT_GUIDE_POLYGONS = 1 };          /* flags of pt_light_guide_ex */
typedef struct pt_light_guide_ex {             /* 12 bytes */
  uint32_t struct_size;                        /* = sizeof(pt_light_guide_ex) */
  float    beta;                               /* as pt_light_guide.beta */
  uint32_t flags;                              /* 0 or PT_LIGHT_GUIDE_POLYGONS */
} pt_light_guide_ex;
int pt_set_light_guide_ex(pt_handle h, const pt_light_guide_ex* g);   /* NULL clears the guide */
int pt_get_light_guide_flags(pt_handle h, uint32_t* flags);           /* flags of the guide in force, 0 without one */
typedef struct pt_light_guide_info {
  uint32_t struct_size;          /* = sizeof(pt_light_guide_info), set by the caller */
  int32_t set, active;
  float beta;                    /* beta_thr / 2^32 */
  uint32_t n_lights;             /* K */
  uint32_t object_index[32];     /* rank -> index into the scene in force (pt_get_scene) */
  uint32_t threshold[32];
  float probability[32];
} pt_light_guide_info;
int pt_get_light_guide_info(pt_handle h, pt_light_guide_info* out);
int pt_light_guide_sample(pt_handle h, const float* origin, const float* normal, const uint32_t* g1, const uint32_t* g2,
                          const uint32_t* g3, size_t n, float* out_dir, int32_t* out_light);
int pt_light_guide_eval(pt_handle h, const float* origin, const float* normal, const float* dir, size_t n, float* out_sum,
                        float* out_pe);

/* First-hit feature buffers -- an EXTENSION: what the centre ray of every pixel sees, noise free, for masks, compositing, the
 * debugging of runtime scenes and as the guide of pt_denoise.  Additive: PTMI_ABI_VERSION stays 5 and no existing struct moves;
 * a process that never calls it runs exactly as before.
 * The ray, for every pixel (u, v) of width x height (all pixels, whatever the worklist holds), is the production camera ray with
 * zero AA noise and no lens: c = (float)u, r = (float)v, px = ((2 c - width) / width) tx, py = -(((2 r - height) / height) ty),
 * camx = half(px), camy = half(py), d = normalise((camx, camy, -1)), origin 0 in camera space -- the expressions of the trace
 * kernels with both noise terms 0.  The hit is the production kernels' nearest hit over the scene in force (pt_set_scene, seen
 * by the camera of pt_set_camera), so with aa_noise_scale = 0 and no lens object_id is the object the trace kernels hit, bit
 * for bit.  The thin lens is ignored on purpose: a guide image must be sharp.
 *   object_id  index into the scene in force (pt_get_scene), -1 for a miss.
 *   depth      hit distance t along the unit ray, 0 for a miss.
 *   normal     sphere: (hit - centre) / |hit - centre| (= (hit - centre) / radius but for the rounding of the hit point; unit to
 *              rounding); disc: its stored normal.  Flipped to face the ray (dot(n, d) > 0 -> -n), then rotated to WORLD space
 *              (x r + y u - z f, as every quantity the ABI reports) and normalised again when a camera pose is set.  0 for a miss.
 *   albedo     the object's colour for diffuse and refractive objects; (1, 1, 1) for specular and emissive objects and for a
 *              miss (the usual demodulation convention).  Stored B, G, R like every other image of the ABI.
 * The buffers stay on the device as the handle's feature cache, two float4 per pixel, allocated at the first call and freed by
 * pt_destroy; pt_set_scene, pt_set_camera and pt_set_render_settings (the field of view) make the next call recompute them,
 * and a call without such a change copies the cache.  Nothing else is touched: not the worklist, the accumulators or the film.
 * Any pointer of pt_features may be NULL (= not wanted).  PT_ERR_INVALID_ARGUMENT for a NULL handle, a NULL `out` or a wrong
 * struct_size; PT_ERR_NOT_READY before pt_set_render_settings (no worklist is needed); PT_ERR_OUT_OF_MEMORY if the cache cannot
 * be allocated, and nothing else changes. */
typedef struct pt_features {        /* all host pointers, any may be NULL (= not wanted) */
  uint32_t struct_size;             /* sizeof(pt_features), set by the caller */
  int32_t* object_id;               /* [height][width]      index into the scene in force, -1 = miss */
  float*   depth;                   /* [height][width]      hit distance t along the unit ray, 0 for a miss */
  float*   normal;                  /* [height][width][3]   WORLD-space unit normal facing the camera, 0 for a miss */
  float*   albedo;                  /* [height][width][3]   B,G,R */
} pt_features;
int pt_feature_buffers(pt_handle h, pt_features* out);

/* Film denoiser -- an EXTENSION: an edge-avoiding A-trous wavelet filter (Dammertz et al., HPG 2010) over a finished image, on
 * the device, steered by the feature buffers above (computed on demand).  It runs after the sampling loop: no trace, NIF or
 * accumulate kernel is involved and nothing a render produces moves.  Additive: PTMI_ABI_VERSION stays 5.
 * Source.  PT_DENOISE_HOST_IMAGE: host_bgr_in, [height][width][3] float32 B, G, R (what rank 0 holds after pt_gather_hdr).
 * The other two scatter THIS handle's work items into a dense image by their (u, v): PT_DENOISE_ACCUMULATORS the mean radiance
 * (b, g, r) * (1 / sampleCount) as pt_export_hdr_device forms it (0 samples -> 0), PT_DENOISE_FILM the resident film's running
 * sum times 1 / film_steps (one binary32 multiply by the binary32 reciprocal of the number of pt_film_accumulate calls since
 * pt_setup).  Pixels the worklist does not hold, and padding items, are 0; a pixel it holds twice gets one of the two values.
 * Definition, every operation binary32.  Let c_0[p] be the source; with `demodulate`, c_0[p] /= max(albedo[p], 1e-3) per channel
 * and the result is multiplied by the same factor at the end.  Iteration i = 0 .. iterations - 1 has the step s = 2^i and the
 * taps q = p + s (dx, dy), dx, dy in {-2 .. 2}; a tap outside the image is skipped (no clamping, no wrap).
 *   h(dx, dy) = k[|dx|] k[|dy|], k = (3/8, 1/4, 1/16)                                      (the B3 spline)
 *   w = w_c w_n w_d w_id, a disabled stop being 1:
 *     w_c  = exp(-|c_i[p] - c_i[q]|^2 / sc_i^2), sc_i = sigma_colour 2^-i                  (the halving of Dammertz et al.)
 *     w_n  = exp(-|n[p] - n[q]|^2 / sigma_normal^2)
 *     w_d  = exp(-(d[p] - d[q])^2 / (sigma_depth max(d[p], 1e-6))^2)
 *     w_id = 1 when the object ids are equal, else 0 -- a hard zero: that tap contributes nothing and its colour is not even
 *            multiplied, so a non-finite neighbour on another object cannot leak.
 *   c_{i+1}[p] = sum h w c_i[q] / sum h w.  The centre tap has w = 1 exactly (it is not computed through exp), so the
 *   denominator is >= 9/64 and the result is a convex combination of the inputs.
 * As evaluated: the three exponentials are one, expf(-(x_c + x_n + x_d)) with x = squared difference times the binary32
 * reciprocal of the squared sigma; a stop whose squared difference is exactly 0 adds 0 without forming the product.
 * Non-finite input colours are not validated and propagate (to every pixel whose taps reach them with a non-zero weight).
 * pt_denoise_default_params fills the defaults (and struct_size); it needs no handle and no device.  params == NULL means the
 * defaults.  The dense frames (2 colour + 2 feature float4 per pixel, 64 bytes per pixel) are allocated on first use and freed
 * by pt_destroy.  The result is host_bgr_out, [height][width][3] float32 B, G, R.  Blocking.
 * PT_ERR_INVALID_ARGUMENT, pt_last_error naming the field, for a wrong struct_size, iterations outside 1..6, a sigma that is
 * not finite, a source out of range, a NULL host_bgr_out, a NULL host_bgr_in with PT_DENOISE_HOST_IMAGE, and a NULL handle;
 * these are checked in this order before anything touches a device, and with h == NULL the message is pt_last_error(NULL)'s.
 * PT_ERR_NOT_READY before pt_set_render_settings, without a worklist for the two device sources, and with no
 * pt_film_accumulate since pt_setup for PT_DENOISE_FILM; PT_ERR_OUT_OF_MEMORY if the frames cannot be allocated.
 * Multi-GPU: every rank's handle sees the whole scene, so the rank that holds the gathered image (rank 0) denoises it with
 * PT_DENOISE_HOST_IMAGE; the device sources of one rank cover that rank's pixels only. */
enum { PT_DENOISE_HOST_IMAGE = 0, PT_DENOISE_ACCUMULATORS = 1, PT_DENOISE_FILM = 2 };
typedef struct pt_denoise_params {
  uint32_t struct_size;     /* sizeof(pt_denoise_params), set by the caller (pt_denoise_default_params sets it) */
  uint32_t iterations;      /* 1..6, default 5: step 1, 2, 4, ... */
  float sigma_colour;       /* default 4;  <= 0 disables the colour stop */
  float sigma_normal;       /* default 0.5; <= 0 disables */
  float sigma_depth;        /* default 0.1 (relative); <= 0 disables */
  int32_t object_stop;      /* default 1: a tap on another object id gets weight 0 */
  int32_t demodulate;       /* default 1: divide by albedo before, multiply after */
} pt_denoise_params;
int pt_denoise_default_params(pt_denoise_params* p);     /* needs no handle and no device */
int pt_denoise(pt_handle h, const pt_denoise_params* p /* NULL = defaults */, int32_t source,
               const float* host_bgr_in /* [h][w][3], PT_DENOISE_HOST_IMAGE only */, float* host_bgr_out /* [h][w][3] */);

/* NIF trainer -- an EXTENSION: an HDR environment map in, a NIF out, on the device.  The reference sends its users to an external
 * TensorFlow script ("Train your own Environment Lighting Network"); here the library makes its own assets from the map
 * pt_set_env_map holds.  It runs beside the sampling loop on the handle's stream: no trace, NIF or accumulate kernel is involved
 * and nothing a render produces moves.  Additive: PTMI_ABI_VERSION stays 5.  Everything is binary32 (the matrix products on
 * v_mfma_f32_32x32x2_f32) unless pt_nif_train_set_precision asks for PT_NIF_TRAIN_MIXED_F16 (below).
 * Model: layer_count ReLU layers of width hidden, the first on the 4 E Fourier features [sin u, sin v, cos u, cos v] x E
 * (E = embedding_dim), layer layer_count / 2 (when that is not layer 0) on concat(x, features), and a linear head of 3
 * outputs: layer_count + 1 layers in pt_layer layout, kernel row-major [in][out].  A feature is half(sin(a)) / half(cos(a)) of
 * a = half((coord - 1) 2 2^j), the sine correctly rounded to binary32 first: the oracle's orc_nif_encode bit for bit.
 * pt_nif_train_begin needs a map on the handle (PT_ERR_NOT_READY otherwise).  With L = log(texel + eps) in log mode and the
 * texel itself otherwise (binary64 from the binary32 texel and eps) it computes mean[c] = the per-channel mean of L, rounded to
 * binary32, and max = the largest |L - mean[c]|, rounded to binary32, by per-block partial sums added in block order; a
 * constant image (max = 0) is PT_ERR_INVALID_ARGUMENT.  It keeps the image as targets t = (L - mean) / max (binary64 from the
 * binary32 mean and max, rounded once) in device memory of its own, 16 bytes per texel, so training goes on after the map is
 * replaced.  It allocates master weights, Adam moments, activations and gradients for `batch` samples, draws the kernels
 * Glorot-uniform -- w[i] = (2 x - 1) sqrt(6 / (in + out)), x = ((word 0 >> 8) + 1/2) 2^-24 of Philox4x32-10 block
 * (i, layer, 0, "NIFW") keyed by seed -- and zeroes the biases.  PT_ERR_INVALID_ARGUMENT, pt_last_error naming the field, for a
 * wrong struct_size, embedding_dim outside 1..15 (with 16 the argument of the highest
 * frequency is half(-2 x 2^15) = -inf at u = 0 or v = 0 and its sine NaN), hidden not a multiple of 32 in 32..1024, layer_count outside 1..15, batch not
 * a multiple of 256 in 256..2^20, a learning_rate, adam_eps or eps that is not finite or not positive (eps may be 0 without
 * log_tone_map), a beta outside [0, 1), log_tone_map other than 0 or 1, and a NULL handle; these are checked in this order
 * before anything touches a device, and with h == NULL the message is pt_last_error(NULL)'s.  After a rejection or
 * PT_ERR_OUT_OF_MEMORY an earlier trainer of the handle stays in force; a successful begin replaces it.
 * pt_nif_train_steps runs n Adam steps and returns the loss of the last one (before its update) in *last_loss (may be NULL).
 * Step t = 0, 1, ... (counted since begin or pt_nif_train_set_weights):
 *   sample i < batch: texel index floor(word 0 x H W / 2^32) of Philox block (i, t low, t high, "NIFB") keyed by seed,
 *   r = index / W, c = index mod W, u = (float)r / (float)H, v = (float)c / (float)W (one binary32 division each: the map's
 *   own mapping), target = t[r][c];
 *   forward pass y, loss = mean over batch x 3 of (y - target)^2 (summed in binary64), backward pass, then for every weight
 *   and bias  m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g^2,  w -= lr (m c1) / (sqrt(v c2) + adam_eps),
 *   c1 = 1 / (1 - b1^(t+1)), c2 = 1 / (1 - b2^(t+1)) (the bias-corrected Adam of Kingma and Ba).
 * Deterministic: sums over the batch are per-slab partials added in slab order, there is no float atomic, and two runs with one
 * seed on one device give the same bits.
 * pt_nif_train_get_weights / _set_weights / _export / _gradients take an array of pt_layer whose kernel and bias point to CALLER
 * buffers of rows x cols and cols elements (the getters write through them; bias may be NULL = not wanted, or for set_weights
 * = zeros); n_layers must be layer_count + 1 and every rows, cols must be the model's -- pt_nif_train_layer_shapes fills rows,
 * cols, dtype (PT_DTYPE_F32) and relu and touches no pointer.  get / set move the binary32 master weights (dtype PT_DTYPE_F32);
 * set_weights resets the Adam moments and the step counter.  pt_nif_train_export gives the layers rounded to binary16 (round
 * to nearest even) as PT_DTYPE_F16; a finite weight that rounds to infinity is PT_ERR_UNSUPPORTED_MODEL naming the layer.
 * pt_nif_train_get_encode_params returns max and mean as computed; the -eps fold stays where it is, in the metadata loaders.
 * pt_nif_train_install is pt_upload_nif of exactly the exported layers with max, the folded mean (float)(mean - eps) in log
 * mode and log_tone_map: the NIF is the environment from then on, the memo generation advances and the map is dropped as any
 * pt_upload_nif drops it; the trainer stays and can go on.  pt_nif_train_end frees everything, as does pt_destroy; every
 * call but begin answers PT_ERR_NOT_READY without a trainer.
 * Two kernel-level hooks: pt_nif_train_batch copies out the batch step `step` would draw (u, v [batch], target [batch][3]) and
 * changes nothing; pt_nif_train_gradients runs the forward and backward pass on n <= batch caller samples with the current
 * weights and returns the loss and every dW, db in binary32 -- neither weights, moments nor the step counter move. */
typedef struct pt_nif_train_params {
  uint32_t struct_size;          /* sizeof(pt_nif_train_params), set by the caller (pt_nif_train_default_params sets it) */
  uint32_t embedding_dim;        /* 1..15, default 12 */
  uint32_t hidden;               /* a multiple of 32 in 32..1024, default 320 */
  uint32_t layer_count;          /* hidden ReLU layers, 1..15, default 6 */
  uint32_t batch;                /* samples per step, a multiple of 256, default 65536 */
  float learning_rate;           /* default 1e-3 */
  float beta1, beta2;            /* default 0.9, 0.999 */
  float adam_eps;                /* default 1e-7 */
  uint64_t seed;                 /* default 1 */
  int32_t log_tone_map;          /* default 1 */
  float eps;                     /* default 1e-8 */
} pt_nif_train_params;
int pt_nif_train_default_params(pt_nif_train_params* p);     /* needs no handle and no device */
int pt_nif_train_begin(pt_handle h, const pt_nif_train_params* p);
int pt_nif_train_layer_shapes(pt_handle h, pt_layer* layers, uint32_t n_layers);
int pt_nif_train_steps(pt_handle h, uint32_t n, float* last_loss);
int pt_nif_train_get_weights(pt_handle h, pt_layer* layers, uint32_t n_layers);
int pt_nif_train_set_weights(pt_handle h, const pt_layer* layers, uint32_t n_layers);
int pt_nif_train_get_encode_params(pt_handle h, float* max, float mean[3]);
int pt_nif_train_export(pt_handle h, pt_layer* layers, uint32_t n_layers);
int pt_nif_train_install(pt_handle h);
int pt_nif_train_end(pt_handle h);
int pt_nif_train_batch(pt_handle h, uint64_t step, float* u, float* v, float* target);
int pt_nif_train_gradients(pt_handle h, const float* u, const float* v, const float* target, uint32_t n, float* loss,
                           pt_layer* gradients, uint32_t n_layers);

/* Mixed precision for the trainer -- opt-in: binary16 inputs to the matrix products (v_mfma_f32_32x32x16_f16, exact products,
 * binary32 sums), a loss scale S, binary32 master weights.  A successful pt_nif_train_begin always starts in PT_NIF_TRAIN_F32,
 * and a process that never calls pt_nif_train_set_precision runs exactly what it ran before this call existed.  Additive:
 * PTMI_ABI_VERSION stays 5 and pt_nif_train_params stays as it is.
 * pt_nif_train_set_precision may be called at any time between steps (PT_ERR_NOT_READY without a trainer).  It keeps the master
 * weights, the Adam moments and applied_steps, allocates (mixed) or frees (f32) the half buffers, and resets S to loss_scale,
 * good_steps and skipped_steps to 0; the step counter that draws the batches continues at applied_steps.  PT_ERR_INVALID_ARGUMENT,
 * pt_last_error naming the field, in this order and before any device call: NULL struct, wrong struct_size, mode other than 0 or
 * 1, loss_scale not a power of two in 1 .. 2^30, dynamic other than 0 or 1, growth_interval outside 1 .. 2^31, NULL handle (the
 * message is pt_last_error(NULL)'s then).  After a rejection or PT_ERR_OUT_OF_MEMORY the previous mode stays in force.
 * A mixed step:
 *   weights: the masters w, b stay binary32; w16 = half(w) (round to nearest even) is refreshed by the Adam kernel and by
 *   set_weights / set_precision; biases are used in binary32.
 *   forward, hidden layer: z = the binary32-accumulated sum over the half inputs times w16, plus b in binary32; the stored
 *   activation is a = half(max(z, 0)), one rounding; features are half values already.  The head gives y = sum + b in binary32,
 *   not rounded.  loss = mean of (y - t)^2 summed in binary64, unscaled: what last_loss returns, also for a skipped step.
 *   backward: head dZ = half((y - t) c), c = (float)(2 S / (3 n)); dW = X^T dZ and db = the column sums of dZ accumulate in
 *   binary32 over the half values, in the 32 batch slabs, added in slab order; dZ below = half((dZ w16^T)[:, :cols below] (a > 0))
 *   on the stored half activation; feature columns carry no gradient.
 *   unscale: g = g_scaled (1 / S), exact.  If any element of any dW or db is not finite the step is SKIPPED: weights, w16 and
 *   moments keep their bits, skipped_steps advances and, with dynamic, S halves (floor 1) and good_steps returns to 0.
 *   Otherwise Adam applies as above with t + 1 = applied_steps + 1, applied_steps and good_steps advance and, with dynamic, S
 *   doubles (cap 2^30) and good_steps returns to 0 when good_steps reaches growth_interval.
 *   The batch drawn is that of step applied_steps + skipped_steps since begin / set_weights / set_precision: a skipped step
 *   draws the next batch.  S, 1 / S, c, the counters and Adam's c1, c2 (binary64 on the device) live in a device control block
 *   that one single-thread kernel updates per step; pt_nif_train_steps still waits once, at its end.  Deterministic as above.
 * In mixed mode pt_nif_train_gradients runs this pass with the current S and returns the unscaled binary32 gradients (an
 * overflow shows as non-finite values); S, counters, weights and moments do not move.  export / install are unchanged (the
 * export equals w16 bit for bit); get_weights / set_weights move the masters, and set_weights also zeroes applied_steps and
 * skipped_steps.  In PT_NIF_TRAIN_F32 pt_nif_train_get_precision_state reports loss_scale 1, good_steps 0, skipped_steps 0. */
#define PT_NIF_TRAIN_F32        0
#define PT_NIF_TRAIN_MIXED_F16  1
typedef struct pt_nif_train_precision {
  uint32_t struct_size;      /* sizeof(pt_nif_train_precision), set by the caller (pt_nif_train_default_precision sets it) */
  int32_t  mode;             /* PT_NIF_TRAIN_F32 | PT_NIF_TRAIN_MIXED_F16, default PT_NIF_TRAIN_F32 */
  float    loss_scale;       /* initial scale S, a power of two in 1 .. 2^30, default 65536 */
  int32_t  dynamic;          /* 0 | 1, default 1 */
  uint32_t growth_interval;  /* applied steps without overflow before S doubles, 1 .. 2^31, default 2000 */
} pt_nif_train_precision;
typedef struct pt_nif_train_precision_state {
  uint32_t struct_size;      /* sizeof(pt_nif_train_precision_state), set by the caller */
  int32_t  mode;
  float    loss_scale;       /* the current S */
  uint32_t good_steps;       /* applied steps since S last changed */
  uint64_t applied_steps, skipped_steps;
} pt_nif_train_precision_state;
int pt_nif_train_default_precision(pt_nif_train_precision* p);          /* needs no handle and no device */
int pt_nif_train_set_precision(pt_handle h, const pt_nif_train_precision* p);
int pt_nif_train_get_precision_state(pt_handle h, pt_nif_train_precision_state* s);

/* Multi-GPU film hand-off.  The path shards over pixels with no exchange of ray data (reference: one NIF
 * replica per IPU, "no inter-ipu exchange of ray data", PathTracerApp.cpp:205-252, shard_utils.cpp:28-38);
 * the only exchange is the film: mean radiance per work item, BGR float32 [n][3] -- the value
 * AccumulatedImage::accumulate adds, AccumulatedImage.cpp:59-74: (b,g,r)/sampleCount, with the device's
 * 32-bit sample count (0 samples -> 0).
 *
 * pt_export_hdr_device writes this rank's tile into a caller-owned DEVICE buffer on the handle's stream.
 *
 * pt_film_accumulate keeps the film on the device between save intervals: it is AccumulatedImage::accumulate
 * (AccumulatedImage.cpp:59-74: film += (b,g,r) * (1/sampleCount)) followed by
 * LoadBalancer::clearInactiveAccumulators (LoadBalancer.cpp:198-213) for every work item, with the host's fp32
 * expressions, so the resident film equals the host film bit for bit.  pt_setup starts a new (zero) film.
 *
 * pt_gather_hdr is the whole hand-off as one call, made by every rank of the communicator: take this rank's
 * tile -- PT_HDR_ACCUMULATORS: mean radiance of the current accumulators (as pt_export_hdr_device);
 * PT_HDR_FILM: the resident film's running sum (the host divides by the step count when it saves,
 * AccumulatedImage.cpp:24,54) -- into a slot of `slot_items` items (>= this rank's item count, equal on all
 * ranks, zero padded), ONE RCCL gather to rank 0 (grouped ncclSend/ncclRecv: every peer sends directly to the
 * root over its own xGMI link), and on rank 0 a copy of all tiles [world][slot_items][3] into `root_host_bgr`
 * (ignored on the other ranks; may be NULL).  Blocking.  Without a communicator it degenerates to export +
 * copy of one tile.
 *
 * Communicators: one rank per handle.  One process per GPU: rank 0 calls pt_comm_get_unique_id, hands the
 * PT_COMM_ID_BYTES bytes to the other processes by any means (MPI, torch.distributed, a file), everyone calls
 * pt_comm_init_rank.  One process driving several GPUs (ipu_trace --ipus N): pt_comm_init_all on the list of
 * handles; pt_gather_hdr is then called from one thread per handle.  pt_destroy releases the communicator.
 *
 * No communicator call blocks for ever (the reference's Poplar engine has no such failure mode: its IPUs are one
 * device, PathTracerApp.cpp:205-252).  Communicators are asked to be non-blocking and their progress is polled against a
 * deadline (pt_comm_set_timeout, default 120000 ms); because the RCCL of ROCm 7.2 (2.27.7) does not honour that for set-up
 * and abort, every RCCL call that may need a peer additionally runs on a worker thread of the handle and is WAITED FOR
 * against the same deadline: a call that never returns is abandoned.  slot_items is checked for
 * agreement between the ranks once per communicator and slot size (PT_ERR_INVALID_ARGUMENT on every rank if it differs).
 * If a peer never joins an exchange (it failed a local check and returned early, crashed, or was never started), if RCCL
 * reports an asynchronous error, or if another thread calls pt_comm_abort(h), the waiting rank aborts its communicator
 * (ncclCommAbort, itself bounded), drains its stream and returns PT_ERR_COMM; the handle then has no communicator and
 * pt_gather_hdr keeps returning PT_ERR_COMM until pt_comm_init_rank / pt_comm_init_all gives it a new one.  CONTRACT for
 * callers that drive several ranks: when one rank's call fails, abort the others (pt_comm_abort -- the only pt_* function
 * that may be called from another thread while a call on the same handle is in progress) or let them time out.
 * pt_comm_init_rank / pt_comm_init_all ask the RCCL they are bound to for its version first (ncclGetVersion): older than
 * 2.14 (no ncclCommInitRankConfig) is refused with PT_ERR_COMM; older than the headers libptmi.so was compiled against,
 * the ncclConfig_t is stamped with the RUNNING library's version, so that library reads exactly the fields it knows
 * (pt_runtime_info and DESIGN.md section 6 say which RCCL a process runs on).
 * Multi-rank exchanges have not been run on hardware yet (no multi-GPU box was available): DESIGN.md section 6. */
enum { PT_HDR_ACCUMULATORS = 0, PT_HDR_FILM = 1 };
#define PT_COMM_ID_BYTES 128
int pt_comm_get_unique_id(void* id_out);
int pt_comm_init_rank(pt_handle h, const void* id, int rank, int world);
int pt_comm_init_all(pt_handle* handles, int n);
int pt_comm_info(pt_handle h, int* rank, int* world);
int pt_comm_set_timeout(pt_handle h, uint32_t milliseconds);
int pt_comm_abort(pt_handle h);
int pt_film_accumulate(pt_handle h);
/* Path-length balancing without the worklist leaving the device.  The reference re-deals work by the pathLength every
 * step returns per work item (LoadBalancer::allocateWorkByPathLength, LoadBalancer.cpp:141-192), which costs the whole
 * trace buffer both ways per step; across GPUs the unit of re-dealing is an image tile, so what the balancer needs is
 * kilobytes: per tile of tile_w x tile_h pixels (row-major grid over width x height) the sum of pathLength of this
 * handle's work items.  pt_tile_costs_enable starts the bookkeeping (what pt_film_accumulate clears from the
 * accumulators is folded into the per-tile sums first); pt_tile_costs copies, for all n_tiles = ceil(width / tile_w) x
 * ceil(height / tile_h) tiles, tracked sums + the current accumulators' pathLength to the host (uint64 each; padding
 * items, u = v = 65535, belong to no tile).  pt_setup starts the sums afresh. */
/* pt_film_seed: after a re-deal the film has to follow its pixels.  Sets the resident film of the n = current work
 * items from host values (BGR float32 [n][3], the running sums pt_gather_hdr(PT_HDR_FILM) returned for those pixels),
 * so that every pixel's fp32 sum continues in step order whichever handle owns it: a balanced render equals the
 * unbalanced one bit for bit.  Called after pt_setup (which zeroes the film), at save intervals only. */
int pt_film_seed(pt_handle h, const float* host_bgr, size_t n);
int pt_tile_costs_enable(pt_handle h, uint32_t tile_w, uint32_t tile_h);
int pt_tile_costs(pt_handle h, uint64_t* host_costs, size_t n_tiles);
int pt_gather_hdr(pt_handle h, int32_t source, size_t slot_items, float* root_host_bgr);
int pt_export_hdr_device(pt_handle h, void* device_bgr, size_t n);
/* Clear r,g,b,sampleCount,pathLength on the device worklist
 * (LoadBalancer::clearInactiveAccumulators, LoadBalancer.cpp:198-213) without a host round trip. */
int pt_clear_accumulators(pt_handle h);
int pt_synchronize(pt_handle h);

/* Standalone NIF inference, host buffers: u, v in [0,1) -> decoded BGR float32 [n][3]
 * (NifModel's streamed-IO mode, NifModel.cpp:268-278,338-350). */
int pt_nif_infer(pt_handle h, const float* u, const float* v, size_t n, float* bgr);
/* Trace individual paths (pixel u,v; absolute sample index) and return their records. */
int pt_trace_paths(pt_handle h, const uint16_t* u, const uint16_t* v, const uint32_t* sample_index,
                   size_t n, pt_path_record* out);

#ifdef __cplusplus
}
#endif
#endif /* PTMI_H */
