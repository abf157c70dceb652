"""ctypes binding of include/ptmi.h (libptmi.so) plus a thin Renderer that sequences the calls the
way PathTracerApp::execute does (reference: src/PathTracerApp.cpp:612-614, :692-694)."""
import ctypes as C
import os

import numpy as np

from .build import library_path

TRACE_DTYPE = np.dtype([("u", "<u2"), ("v", "<u2"), ("r", "<f4"), ("g", "<f4"), ("b", "<f4"),
                        ("sampleCount", "<u2"), ("pathLength", "<u2")], align=True)
assert TRACE_DTYPE.itemsize == 20  # src/codelets/TraceRecord.hpp:7-19

PATH_DTYPE = np.dtype([("length", "<u4"), ("escaped", "<u4"), ("dir", "<f4", 3), ("uv", "<f4", 2),
                       ("throughput", "<f4", 3), ("cam", "<f4", 2)])
assert PATH_DTYPE.itemsize == 48

SCENE_DTYPE = np.dtype([("shape", "<i4"), ("material", "<i4"), ("centre", "<f4", 3), ("radius", "<f4"),
                        ("normal", "<f4", 3), ("colour", "<f4", 3)])
assert SCENE_DTYPE.itemsize == 48   # pt_scene_object
SCENE_EX_DTYPE = np.dtype(SCENE_DTYPE.descr + [("vertex", "<f4", (3, 3))])
assert SCENE_EX_DTYPE.itemsize == 84   # pt_scene_object_ex
MAX_SCENE_OBJECTS = 32
SHAPE_SPHERE, SHAPE_DISC = 0, 1
SHAPE_TRIANGLE, SHAPE_PARALLELOGRAM = 2, 3
SHAPE_MESH = 4
MAX_MESH_TRIANGLES = 1 << 22      # PT_MAX_MESH_TRIANGLES: per scene, all meshes together
MESH_INTERSECT_BVH, MESH_INTERSECT_BRUTE = 0, 1
SHAPES_EX = {"sphere": SHAPE_SPHERE, "disc": SHAPE_DISC, "triangle": SHAPE_TRIANGLE, "parallelogram": SHAPE_PARALLELOGRAM}
MATERIAL_DIFFUSE, MATERIAL_SPECULAR, MATERIAL_REFRACTIVE, MATERIAL_EMISSIVE = 0, 1, 2, 3
SHAPES = {"sphere": SHAPE_SPHERE, "disc": SHAPE_DISC}
MATERIALS = {"diffuse": MATERIAL_DIFFUSE, "specular": MATERIAL_SPECULAR, "refractive": MATERIAL_REFRACTIVE,
             "emissive": MATERIAL_EMISSIVE}

AA_NORMAL, AA_UNIFORM, AA_TRUNCATED_NORMAL = 0, 1, 2
SAMPLES_HALF, SAMPLES_FLOAT = 0, 1
DTYPE_F16, DTYPE_F32 = 0, 1

ABI_VERSION = 5          # PTMI_ABI_VERSION of include/ptmi.h this binding was written against
EXPORTS = ["pt_abi_version", "pt_create", "pt_destroy", "pt_last_error", "pt_upload_nif", "pt_set_constant_env",
           "pt_set_render_settings", "pt_setup", "pt_path_trace", "pt_read_results", "pt_get_stats",
           "pt_export_hdr_device", "pt_clear_accumulators", "pt_synchronize", "pt_nif_infer", "pt_trace_paths",
           "pt_comm_get_unique_id", "pt_comm_init_rank", "pt_comm_init_all", "pt_comm_info", "pt_comm_set_timeout", "pt_comm_abort",
           "pt_gather_hdr", "pt_film_accumulate", "pt_tile_costs_enable", "pt_tile_costs", "pt_film_seed",
           "pt_nif_kernel_name", "pt_calibrate_nif", "pt_runtime_info", "pt_set_nif_sharing", "pt_get_nif_sharing_stats",
           "pt_get_nif_class_stats",
           "pt_set_nif_memo", "pt_clear_nif_memo", "pt_get_nif_memo_stats", "pt_set_scene", "pt_get_scene",
           "pt_set_camera", "pt_get_camera", "pt_set_env_map", "pt_env_map_lookup", "pt_feature_buffers",
           "pt_denoise_default_params", "pt_denoise", "pt_nif_train_default_params", "pt_nif_train_begin",
           "pt_nif_train_layer_shapes", "pt_nif_train_steps", "pt_nif_train_get_weights", "pt_nif_train_set_weights",
           "pt_nif_train_get_encode_params", "pt_nif_train_export", "pt_nif_train_install", "pt_nif_train_end",
           "pt_nif_train_batch", "pt_nif_train_gradients", "pt_nif_train_default_precision", "pt_nif_train_set_precision",
           "pt_nif_train_get_precision_state", "pt_set_env_guide", "pt_env_guide_sample", "pt_env_guide_eval",
           "pt_set_light_guide", "pt_set_light_guide_ex", "pt_get_light_guide_flags", "pt_get_light_guide_info", "pt_light_guide_sample", "pt_light_guide_eval",
           "pt_set_env_guide_from_environment", "pt_get_env_guide_info", "pt_get_env_guide_tables", "pt_set_scene_ex",
           "pt_get_scene_ex", "pt_set_scene_meshes", "pt_get_mesh_info", "pt_mesh_intersect", "pt_set_mesh_normals",
           "pt_get_mesh_normals_info", "pt_mesh_shade", "pt_set_mesh_texture", "pt_get_mesh_texture_info", "pt_mesh_texel",
           "pt_set_mesh_build", "pt_get_mesh_build_info", "pt_mesh_tree", "pt_update_mesh_vertices", "pt_get_mesh_update_info",
           "pt_get_trace_variant", "pt_set_mesh_device_tree", "pt_get_mesh_device_tree_info"]
# pt_get_trace_variant: the values of ptvariant::Camera, Bounce and Geometry (csrc/ptmi_trace_variant.h), and the three families' sizes
TRACE_CAMERA_BUILTIN, TRACE_CAMERA_POSE, TRACE_CAMERA_LENS = 0, 1, 2
TRACE_BOUNCE_PLAIN, TRACE_BOUNCE_ENV_GUIDE, TRACE_BOUNCE_LIGHT_GUIDE, TRACE_BOUNCE_LIGHT_GUIDE_PLAMPS = 0, 1, 2, 3
TRACE_GEOMETRY_SPHERES, TRACE_GEOMETRY_POLY, TRACE_GEOMETRY_MESH, TRACE_GEOMETRY_SMOOTH, TRACE_GEOMETRY_TEX = 0, 1, 2, 3, 4
TRACE_CAMERAS = ("BUILTIN", "POSE", "LENS")
TRACE_BOUNCES = ("PLAIN", "ENV_GUIDE", "LIGHT_GUIDE", "LIGHT_GUIDE_PLAMPS")
TRACE_GEOMETRIES = ("SPHERES", "POLY", "MESH", "SMOOTH", "TEX")
TRACE_INSTANCES, TRACE_PATHS_INSTANCES, TRACE_FEATURE_INSTANCES = 57, 19, 5
MESH_UPDATE_REFIT, MESH_UPDATE_REBUILD = 0, 1
MESH_UPDATE_MODES = {"refit": MESH_UPDATE_REFIT, "rebuild": MESH_UPDATE_REBUILD}
MESH_UPDATE_HOST_MEMORY, MESH_UPDATE_DEVICE_MEMORY = 0, 1
MESH_BUILDER_HOST, MESH_BUILDER_DEVICE = 0, 1
MESH_BUILDERS = {"host": MESH_BUILDER_HOST, "device": MESH_BUILDER_DEVICE}
MESH_POSE_REBUILD, MESH_POSE_REFIT = 0, 1
MESH_POSES = {"rebuild": MESH_POSE_REBUILD, "refit": MESH_POSE_REFIT}
MESH_LAST_NONE, MESH_LAST_HOST_BUILD, MESH_LAST_DEVICE_BUILD, MESH_LAST_REFIT = 0, 1, 2, 3
MESH_DEVICE_TREE_LINEAR, MESH_DEVICE_TREE_SAH = 0, 1
MESH_DEVICE_TREES = {"linear": MESH_DEVICE_TREE_LINEAR, "sah": MESH_DEVICE_TREE_SAH}
MESH_NODE_DTYPE = np.dtype([("lo", np.float32, 3), ("hi", np.float32, 3), ("skip", np.uint32), ("leaf", np.uint32)])   # pt_mesh_node
TEX_FILTER_NEAREST, TEX_FILTER_BILINEAR = 0, 1
TEX_FILTERS = {"nearest": TEX_FILTER_NEAREST, "bilinear": TEX_FILTER_BILINEAR}
TEX_WRAP_REPEAT, TEX_WRAP_CLAMP = 0, 1
TEX_WRAPS = {"repeat": TEX_WRAP_REPEAT, "clamp": TEX_WRAP_CLAMP}
MESH_TEXTURE_MAX_SIZE = 8192
NIF_SHARE_OFF, NIF_SHARE_BATCH, NIF_SHARE_STEP = 0, 1, 2
NIF_SHARE_MODES = {"off": NIF_SHARE_OFF, "batch": NIF_SHARE_BATCH, "step": NIF_SHARE_STEP}
ENV_FILTER_NEAREST, ENV_FILTER_BILINEAR = 0, 1
ENV_FILTERS = {"nearest": ENV_FILTER_NEAREST, "bilinear": ENV_FILTER_BILINEAR}
ENV_GUIDE_MAX_ROWS, ENV_GUIDE_MAX_COLS, ENV_GUIDE_MAX_ALPHA = 1024, 2048, 0.9
LIGHT_GUIDE_MAX_BETA = 0.9
LIGHT_GUIDE_POLYGONS = 1          # PT_LIGHT_GUIDE_POLYGONS: flags of pt_light_guide_ex
COMM_ID_BYTES = 128
HDR_ACCUMULATORS, HDR_FILM = 0, 1
DENOISE_HOST_IMAGE, DENOISE_ACCUMULATORS, DENOISE_FILM = 0, 1, 2
DENOISE_SOURCES = {"accumulators": DENOISE_ACCUMULATORS, "film": DENOISE_FILM}


class PtError(RuntimeError):
    """Mirrors the std::runtime_error the reference throws (src/ipu_utils.hpp:532-535)."""

    def __init__(self, code, message):
        super().__init__("ptmi error %d: %s" % (code, message))
        self.code = code


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
                ("max_path_length", C.c_uint32), ("roulette_depth", C.c_uint32), ("stop_prob", C.c_float),
                ("refractive_index", C.c_float), ("aa_noise_type", C.c_int32), ("sample_precision", C.c_int32),
                ("device", C.c_int32), ("max_work_items", C.c_uint32), ("iterations_per_batch", C.c_uint32),
                ("stream", C.c_void_p)]


class Layer(C.Structure):
    _fields_ = [("rows", C.c_uint32), ("cols", C.c_uint32), ("kernel", C.c_void_p), ("bias", C.c_void_p),
                ("dtype", C.c_int32), ("relu", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("escaped", C.c_uint64),
                ("nif_flops_per_sample", C.c_uint64), ("path_trace_ms", C.c_double), ("nif_ms", C.c_double),
                ("accumulate_ms", C.c_double), ("total_ms", C.c_double), ("trace_launches", C.c_uint32),
                ("nif_launches", C.c_uint32), ("accumulate_launches", C.c_uint32), ("first_sample", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SceneObject(C.Structure):
    """pt_scene_object (include/ptmi.h): one sphere or disc of a runtime scene."""
    _fields_ = [("shape", C.c_int32), ("material", C.c_int32), ("centre", C.c_float * 3), ("radius", C.c_float),
                ("normal", C.c_float * 3), ("colour", C.c_float * 3)]


class Camera(C.Structure):
    """pt_camera (include/ptmi.h): position, orientation and thin lens of the runtime camera."""
    _fields_ = [("struct_size", C.c_uint32), ("position", C.c_float * 3), ("look_at", C.c_float * 3), ("up", C.c_float * 3),
                ("lens_radius", C.c_float), ("focus_distance", C.c_float)]

    def as_dict(self):
        return {"position": tuple(self.position), "look_at": tuple(self.look_at), "up": tuple(self.up),
                "lens_radius": self.lens_radius, "focus_distance": self.focus_distance}


assert C.sizeof(Camera) == 48   # pt_camera


class EnvGuide(C.Structure):
    """pt_env_guide (include/ptmi.h): the image, the grid and alpha of an environment guide."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("rows", C.c_uint32),
                ("cols", C.c_uint32), ("alpha", C.c_float), ("bgr", C.c_void_p)]


assert C.sizeof(EnvGuide) == 32   # pt_env_guide


class EnvGuideAuto(C.Structure):
    """pt_env_guide_auto (include/ptmi.h): grid, supersampling, alpha and follow of a guide built from the environment in force."""
    _fields_ = [("struct_size", C.c_uint32), ("rows", C.c_uint32), ("cols", C.c_uint32), ("supersample", C.c_uint32),
                ("alpha", C.c_float), ("follow", C.c_int32)]


class EnvGuideInfo(C.Structure):
    """pt_env_guide_info (include/ptmi.h): the environment guide in force and how it was built."""
    _fields_ = [("struct_size", C.c_uint32), ("set", C.c_int32), ("source", C.c_int32), ("rows", C.c_uint32), ("cols", C.c_uint32),
                ("supersample", C.c_uint32), ("alpha", C.c_float), ("follow", C.c_int32), ("stale", C.c_int32),
                ("rebuilds", C.c_uint64), ("clamped", C.c_uint64), ("build_ms", C.c_double)]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}
        d.update(set=bool(self.set), source="environment" if self.source else "image", follow=bool(self.follow), stale=bool(self.stale))
        return d


assert C.sizeof(EnvGuideAuto) == 24 and C.sizeof(EnvGuideInfo) == 64   # pt_env_guide_auto, pt_env_guide_info


class LightGuide(C.Structure):
    """pt_light_guide (include/ptmi.h): the probability beta of drawing a diffuse bounce towards an emitter."""
    _fields_ = [("struct_size", C.c_uint32), ("beta", C.c_float)]


class LightGuideEx(C.Structure):
    """pt_light_guide_ex (include/ptmi.h): pt_light_guide with flags (LIGHT_GUIDE_POLYGONS: draw from emissive polygons too)."""
    _fields_ = [("struct_size", C.c_uint32), ("beta", C.c_float), ("flags", C.c_uint32)]


class LightGuideInfo(C.Structure):
    """pt_light_guide_info (include/ptmi.h): the emitter guide in force and its table."""
    _fields_ = [("struct_size", C.c_uint32), ("set", C.c_int32), ("active", C.c_int32), ("beta", C.c_float),
                ("n_lights", C.c_uint32), ("object_index", C.c_uint32 * 32), ("threshold", C.c_uint32 * 32),
                ("probability", C.c_float * 32)]


assert C.sizeof(LightGuideEx) == 12
assert C.sizeof(LightGuide) == 8 and C.sizeof(LightGuideInfo) == 404   # pt_light_guide, pt_light_guide_info


def default_env_guide_grid(width, height):
    """(rows, cols): the largest powers of two not above the image size or the caps."""
    rows = cols = 1
    while rows * 2 <= min(height, ENV_GUIDE_MAX_ROWS):
        rows *= 2
    while cols * 2 <= min(width, ENV_GUIDE_MAX_COLS):
        cols *= 2
    return rows, cols


def make_camera(position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), lens_radius=0.0, focus_distance=1.0):
    """A Camera with struct_size set; the defaults are the built-in camera."""
    cam = Camera()
    cam.struct_size = C.sizeof(Camera)
    cam.position = (C.c_float * 3)(*[float(x) for x in position])
    cam.look_at = (C.c_float * 3)(*[float(x) for x in look_at])
    cam.up = (C.c_float * 3)(*[float(x) for x in up])
    cam.lens_radius = float(lens_radius)
    cam.focus_distance = float(focus_distance)
    return cam


def default_camera():
    """The built-in camera as the library reports it (pt_get_camera with no handle); needs no GPU."""
    cam = Camera()
    rc = load_library().pt_get_camera(None, C.byref(cam))
    if rc:
        raise PtError(rc, "pt_get_camera failed")
    return cam


def scene_array(objects):
    """A SCENE_DTYPE array from a SCENE_DTYPE array or a list of dicts with the keys shape, material, centre, radius, normal,
    colour ("emission" is accepted for colour); shape and material may be names ("sphere", "disc"; "diffuse", "specular",
    "refractive", "emissive") or their numbers.  normal may be left out for a sphere, colour for a specular object."""
    if isinstance(objects, np.ndarray) and objects.dtype == SCENE_DTYPE:
        return np.ascontiguousarray(objects)
    out = np.zeros(len(objects), dtype=SCENE_DTYPE)
    for i, o in enumerate(objects):
        unknown = set(o) - {"shape", "material", "centre", "radius", "normal", "colour", "emission"}
        if unknown:
            raise ValueError("scene object %d: unknown key(s) %s" % (i, sorted(unknown)))
        shape, mat = o["shape"], o["material"]
        out[i]["shape"] = SHAPES[shape] if isinstance(shape, str) else int(shape)
        out[i]["material"] = MATERIALS[mat] if isinstance(mat, str) else int(mat)
        out[i]["centre"] = o["centre"]
        out[i]["radius"] = o["radius"]
        out[i]["normal"] = o.get("normal", (0.0, 0.0, 0.0))
        out[i]["colour"] = o.get("colour", o.get("emission", (1.0, 1.0, 1.0)))
    return out


def _is_polygon_shape(shape):
    return shape in ("triangle", "parallelogram") or (not isinstance(shape, str) and int(shape) in (SHAPE_TRIANGLE, SHAPE_PARALLELOGRAM))


def has_polygon(objects):
    """Does a scene (a SCENE_DTYPE / SCENE_EX_DTYPE array or a list of dicts) hold a triangle or a parallelogram?"""
    if isinstance(objects, np.ndarray):
        return bool(np.any(objects["shape"] >= SHAPE_TRIANGLE))
    return any(_is_polygon_shape(o["shape"]) for o in objects)


def scene_array_ex(objects):
    """A SCENE_EX_DTYPE array (pt_scene_object_ex) from a SCENE_EX_DTYPE or SCENE_DTYPE array or a list of dicts: the keys of
    scene_array, the shape names "triangle" and "parallelogram", and for those "vertices", three points v0, v1, v2 (a polygon
    takes no centre, radius or normal)."""
    if isinstance(objects, np.ndarray) and objects.dtype == SCENE_EX_DTYPE:
        return np.ascontiguousarray(objects)
    if isinstance(objects, np.ndarray) and objects.dtype == SCENE_DTYPE:
        out = np.zeros(len(objects), dtype=SCENE_EX_DTYPE)
        for name in SCENE_DTYPE.names:
            out[name] = objects[name]
        return out
    out = np.zeros(len(objects), dtype=SCENE_EX_DTYPE)
    for i, o in enumerate(objects):
        poly = _is_polygon_shape(o["shape"])
        allowed = {"shape", "material", "vertices", "colour", "emission"} if poly else \
            {"shape", "material", "centre", "radius", "normal", "colour", "emission"}
        unknown = set(o) - allowed
        if unknown:
            raise ValueError("scene object %d: unknown key(s) %s" % (i, sorted(unknown)))
        shape, mat = o["shape"], o["material"]
        out[i]["shape"] = SHAPES_EX[shape] if isinstance(shape, str) else int(shape)
        out[i]["material"] = MATERIALS[mat] if isinstance(mat, str) else int(mat)
        if poly:
            vertices = np.asarray(o["vertices"], dtype=np.float32)
            if vertices.shape != (3, 3):
                raise ValueError("scene object %d: vertices must be three points of three coordinates" % i)
            out[i]["vertex"] = vertices
        else:
            out[i]["centre"] = o["centre"]
            out[i]["radius"] = o["radius"]
            out[i]["normal"] = o.get("normal", (0.0, 0.0, 0.0))
        out[i]["colour"] = o.get("colour", o.get("emission", (1.0, 1.0, 1.0)))
    return out


def _is_mesh_shape(shape):
    return shape == "mesh" or (not isinstance(shape, str) and int(shape) == SHAPE_MESH)


def has_mesh(objects):
    """Does a scene given as a list of dicts hold a mesh?  (An array cannot: a mesh's vertices and triangles travel beside it.)"""
    return not isinstance(objects, np.ndarray) and any(_is_mesh_shape(o["shape"]) for o in objects)


def scene_meshes(objects):
    """(table, meshes) for pt_set_scene_meshes from a list of dicts: the keys of scene_array_ex, and for a mesh
    {"shape": "mesh", "material": ..., "colour": ..., "vertices": (V, 3), "triangles": (T, 3)} -- world-space points and, per
    triangle, three indices into them.  table is a SCENE_EX_DTYPE array whose mesh rows hold shape 4, material and colour;
    meshes is the list of (vertices float32 (V, 3), triangles uint32 (T, 3)) in the order of those rows.  Shapes and index range
    are checked here, everything else by the library."""
    rows, meshes = [], []
    for i, o in enumerate(objects):
        if not _is_mesh_shape(o["shape"]):
            rows.append(o)
            continue
        unknown = set(o) - {"shape", "material", "vertices", "triangles", "colour", "emission", "normals", "normal_indices",
                            "texture", "uvs", "uv_indices", "texture_filter", "texture_wrap"}
        if unknown:
            raise ValueError("scene object %d: unknown key(s) %s" % (i, sorted(unknown)))
        vertices = np.ascontiguousarray(o["vertices"], dtype=np.float32)
        if vertices.ndim != 2 or vertices.shape[1] != 3 or len(vertices) == 0:
            raise ValueError("scene object %d: vertices must be an array of shape (V, 3), V >= 1" % i)
        tri = np.asarray(o["triangles"])
        if tri.ndim != 2 or tri.shape[1] != 3 or len(tri) == 0:
            raise ValueError("scene object %d: triangles must be an array of shape (T, 3), T >= 1" % i)
        if not np.issubdtype(tri.dtype, np.integer) or tri.min() < 0 or tri.max() > 0xffffffff:
            raise ValueError("scene object %d: triangles must hold unsigned 32-bit indices" % i)
        meshes.append((vertices, np.ascontiguousarray(tri, dtype=np.uint32)))
        rows.append({"shape": SHAPE_SPHERE, "material": o["material"], "centre": (0.0, 0.0, 0.0), "radius": 0.0,
                     "colour": o.get("colour", o.get("emission", (1.0, 1.0, 1.0)))})
    table = scene_array_ex(rows)
    for i, o in enumerate(objects):
        if _is_mesh_shape(o["shape"]):
            table[i]["shape"] = SHAPE_MESH
    return table, meshes


def mesh_normals(objects):
    """[(k, normals, normal_indices or None)] for the meshes of a list of dicts that carry "normals" (N, 3), optionally with
    "normal_indices" (T, 3): k counts the mesh rows in order, as pt_set_mesh_normals does."""
    out, k = [], 0
    for i, o in enumerate(objects):
        if not _is_mesh_shape(o["shape"]):
            continue
        if o.get("normals") is not None:
            out.append((k, o["normals"], o.get("normal_indices")))
        elif o.get("normal_indices") is not None:
            raise ValueError("scene object %d: normal_indices without normals" % i)
        k += 1
    return out


def mesh_textures(objects):
    """[(k, image, uvs, uv_indices or None, filter, wrap)] for the meshes of a list of dicts that carry "texture" (H, W, 3 B,G,R)
    and "uvs" (N, 2), optionally with "uv_indices" (T, 3), "texture_filter" and "texture_wrap": k counts the mesh rows in order,
    as pt_set_mesh_texture does."""
    out, k = [], 0
    for i, o in enumerate(objects):
        if not _is_mesh_shape(o["shape"]):
            continue
        if o.get("texture") is not None:
            if o.get("uvs") is None:
                raise ValueError("scene object %d: texture without uvs" % i)
            out.append((k, o["texture"], o["uvs"], o.get("uv_indices"), o.get("texture_filter", "bilinear"), o.get("texture_wrap", "repeat")))
        else:
            for key in ("uvs", "uv_indices", "texture_filter", "texture_wrap"):
                if o.get(key) is not None:
                    raise ValueError("scene object %d: %s without texture" % (i, key))
        k += 1
    return out


def vertex_normals(vertices, triangles):
    """Angle-weighted vertex normals of a mesh that comes without any: for every vertex the sum over its triangles of the
    triangle's unit normal times the corner's angle, normalised.  Computed in float64, returned as float32 (V, 3).  A vertex no
    triangle uses, or whose sum vanishes, gets (0, 0, 0): pt_set_mesh_normals refuses it if a triangle refers to it."""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles, dtype=np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError("vertices must have shape (V, 3) and triangles (T, 3)")
    if len(t) and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("triangles must index vertices")
    p = v[t]                                              # (T, 3, 3)
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    fl = np.linalg.norm(fn, axis=1, keepdims=True)
    fn = np.divide(fn, fl, out=np.zeros_like(fn), where=fl > 0)
    acc = np.zeros_like(v)
    for c in range(3):
        e0 = p[:, (c + 1) % 3] - p[:, c]
        e1 = p[:, (c + 2) % 3] - p[:, c]
        l0 = np.linalg.norm(e0, axis=1)
        l1 = np.linalg.norm(e1, axis=1)
        den = l0 * l1
        cosang = np.divide(np.einsum("ij,ij->i", e0, e1), den, out=np.ones_like(den), where=den > 0)
        ang = np.arccos(np.clip(cosang, -1.0, 1.0))
        np.add.at(acc, t[:, c], fn * ang[:, None])
    ln = np.linalg.norm(acc, axis=1, keepdims=True)
    return np.divide(acc, ln, out=np.zeros_like(acc), where=ln > 0).astype(np.float32)


def builtin_scene_ex():
    """The built-in scene as a SCENE_EX_DTYPE array (pt_get_scene_ex with no handle: vertices 0); needs no GPU."""
    lib = load_library()
    n = C.c_uint32()
    out = np.zeros(MAX_SCENE_OBJECTS, dtype=SCENE_EX_DTYPE)
    rc = lib.pt_get_scene_ex(None, out.ctypes.data, MAX_SCENE_OBJECTS, C.byref(n))
    if rc:
        raise PtError(rc, "pt_get_scene_ex failed")
    return out[:n.value].copy()


def builtin_scene():
    """The built-in scene (the reference's five spheres and floor disc) as a SCENE_DTYPE array; needs no GPU."""
    lib = load_library()
    n = C.c_uint32()
    out = np.zeros(MAX_SCENE_OBJECTS, dtype=SCENE_DTYPE)
    rc = lib.pt_get_scene(None, out.ctypes.data, MAX_SCENE_OBJECTS, C.byref(n))
    if rc:
        raise PtError(rc, "pt_get_scene failed")
    return out[:n.value].copy()


class Mesh(C.Structure):
    """pt_mesh"""
    _fields_ = [("struct_size", C.c_uint32), ("n_vertices", C.c_uint32), ("n_triangles", C.c_uint32),
                ("vertices", C.c_void_p), ("indices", C.c_void_p)]


class MeshInfo(C.Structure):
    """pt_mesh_info"""
    _fields_ = [("struct_size", C.c_uint32), ("object_index", C.c_uint32), ("n_triangles", C.c_uint32), ("n_nodes", C.c_uint32),
                ("max_leaf", C.c_uint32), ("depth", C.c_uint32), ("device_bytes", C.c_uint64), ("build_ms", C.c_double),
                ("pad", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


class MeshBuildOptions(C.Structure):
    """pt_mesh_build_options"""
    _fields_ = [("struct_size", C.c_uint32), ("builder", C.c_int32), ("on_pose", C.c_int32)]


class MeshBuildInfo(C.Structure):
    """pt_mesh_build_info"""
    _fields_ = [("struct_size", C.c_uint32), ("builder", C.c_int32), ("on_pose", C.c_int32), ("sort_on_device", C.c_uint32),
                ("host_builds", C.c_uint64), ("device_builds", C.c_uint64), ("refits", C.c_uint64), ("last_kind", C.c_int32),
                ("reserved", C.c_uint32), ("last_ms", C.c_double), ("device_bytes", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name not in ("struct_size", "reserved")}


class MeshDeviceTreeInfo(C.Structure):
    """pt_mesh_device_tree_info"""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("sah_builds", C.c_uint64), ("last_levels", C.c_uint32),
                ("reserved", C.c_uint32), ("last_ms", C.c_double), ("device_bytes", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name not in ("struct_size", "reserved")}


class MeshUpdate(C.Structure):
    """pt_mesh_update"""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("memory", C.c_int32), ("n_vertices", C.c_uint32),
                ("vertices", C.c_void_p), ("n_normals", C.c_uint32), ("normals", C.c_void_p)]


class MeshUpdateInfo(C.Structure):
    """pt_mesh_update_info"""
    _fields_ = [("struct_size", C.c_uint32), ("last_kind", C.c_int32), ("updates", C.c_uint64), ("refits", C.c_uint64),
                ("rebuilds", C.c_uint64), ("fallbacks", C.c_uint64), ("last_frames_ms", C.c_double), ("last_tree_ms", C.c_double),
                ("device_bytes", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


class TraceVariantLaunch(C.Structure):
    """pt_trace_variant_launch"""
    _fields_ = [("camera", C.c_int32), ("bounce", C.c_int32), ("geometry", C.c_int32), ("index", C.c_int32), ("launches", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class TraceVariantInfo(C.Structure):
    """pt_trace_variant_info"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("trace", TraceVariantLaunch), ("paths", TraceVariantLaunch),
                ("features", TraceVariantLaunch)]


class MeshNormalsInfo(C.Structure):
    """pt_mesh_normals_info"""
    _fields_ = [("struct_size", C.c_uint32), ("has_normals", C.c_uint32), ("per_corner", C.c_uint32), ("n_normals", C.c_uint32),
                ("device_bytes", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


class MeshTexture(C.Structure):
    """pt_mesh_texture"""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("filter", C.c_int32), ("wrap", C.c_int32),
                ("bgr", C.c_void_p), ("uvs", C.c_void_p), ("n_uvs", C.c_uint32), ("uv_indices", C.c_void_p)]


class MeshTextureInfo(C.Structure):
    """pt_mesh_texture_info"""
    _fields_ = [("struct_size", C.c_uint32), ("has_texture", C.c_uint32), ("per_corner", C.c_uint32), ("width", C.c_uint32),
                ("height", C.c_uint32), ("filter", C.c_int32), ("wrap", C.c_int32), ("n_uvs", C.c_uint32), ("device_bytes", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


assert C.sizeof(Mesh) == 32 and C.sizeof(MeshInfo) == 48 and C.sizeof(MeshNormalsInfo) == 24
assert C.sizeof(MeshTexture) == 56 and C.sizeof(MeshTextureInfo) == 40


class Features(C.Structure):
    """pt_features (include/ptmi.h): host pointers of the first-hit feature buffers, any may be NULL."""
    _fields_ = [("struct_size", C.c_uint32), ("object_id", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p),
                ("albedo", C.c_void_p)]


class DenoiseParams(C.Structure):
    """pt_denoise_params (include/ptmi.h): the A-trous filter's settings; default_denoise_params() fills the defaults."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_uint32), ("sigma_colour", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("object_stop", C.c_int32), ("demodulate", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


assert C.sizeof(Features) == 40 and C.sizeof(DenoiseParams) == 28   # pt_features, pt_denoise_params


def default_denoise_params(**overrides):
    """The library's default DenoiseParams (pt_denoise_default_params; needs no GPU), with any field overridden by keyword."""
    p = DenoiseParams()
    rc = load_library().pt_denoise_default_params(C.byref(p))
    if rc:
        raise PtError(rc, "pt_denoise_default_params failed")
    for k, v in overrides.items():
        if k not in p.as_dict():
            raise ValueError("unknown denoise parameter %r (known: %s)" % (k, sorted(p.as_dict())))
        setattr(p, k, v)
    return p


class NifTrainParams(C.Structure):
    """pt_nif_train_params (include/ptmi.h): model, batch, Adam constants, seed and encode mode of the NIF trainer;
    default_nif_train_params() fills the defaults."""
    _fields_ = [("struct_size", C.c_uint32), ("embedding_dim", C.c_uint32), ("hidden", C.c_uint32), ("layer_count", C.c_uint32),
                ("batch", C.c_uint32), ("learning_rate", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("adam_eps", C.c_float), ("seed", C.c_uint64), ("log_tone_map", C.c_int32), ("eps", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


assert C.sizeof(NifTrainParams) == 56   # pt_nif_train_params


NIF_TRAIN_MODES = {"f32": 0, "mixed": 1}   # PT_NIF_TRAIN_F32, PT_NIF_TRAIN_MIXED_F16


class NifTrainPrecision(C.Structure):
    """pt_nif_train_precision (include/ptmi.h): the trainer's precision mode and its loss scaling."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("loss_scale", C.c_float), ("dynamic", C.c_int32),
                ("growth_interval", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class NifTrainPrecisionState(C.Structure):
    """pt_nif_train_precision_state (include/ptmi.h): the mode in force, the current scale and the step counts."""
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("loss_scale", C.c_float), ("good_steps", C.c_uint32),
                ("applied_steps", C.c_uint64), ("skipped_steps", C.c_uint64)]


assert C.sizeof(NifTrainPrecision) == 20 and C.sizeof(NifTrainPrecisionState) == 32


def default_nif_train_precision(**overrides):
    """The library's default NifTrainPrecision (pt_nif_train_default_precision; needs no GPU), with any field overridden by
    keyword; mode may be "f32" / "mixed" or the header's constant."""
    p = NifTrainPrecision()
    rc = load_library().pt_nif_train_default_precision(C.byref(p))
    if rc:
        raise PtError(rc, "pt_nif_train_default_precision failed")
    for k, v in overrides.items():
        if k not in p.as_dict():
            raise ValueError("unknown NIF training precision field %r (known: %s)" % (k, sorted(p.as_dict())))
        if k == "mode" and isinstance(v, str):
            if v not in NIF_TRAIN_MODES:
                raise ValueError("unknown NIF training precision mode %r (known: %s)" % (v, sorted(NIF_TRAIN_MODES)))
            v = NIF_TRAIN_MODES[v]
        setattr(p, k, v)
    return p


def default_nif_train_params(**overrides):
    """The library's default NifTrainParams (pt_nif_train_default_params; needs no GPU), with any field overridden by keyword."""
    p = NifTrainParams()
    rc = load_library().pt_nif_train_default_params(C.byref(p))
    if rc:
        raise PtError(rc, "pt_nif_train_default_params failed")
    for k, v in overrides.items():
        if k not in p.as_dict():
            raise ValueError("unknown NIF training parameter %r (known: %s)" % (k, sorted(p.as_dict())))
        setattr(p, k, v)
    return p


class NifSharingStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("escaped", C.c_uint64), ("evaluations", C.c_uint64),
                ("overflowed", C.c_uint64), ("table_slots", C.c_uint64), ("share_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class NifClassStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("ran", C.c_int32), ("mlp_rows", C.c_uint64), ("alone", C.c_uint64),
                ("table_slots", C.c_uint64), ("class_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class NifMemoStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("enabled", C.c_int32), ("slots", C.c_uint64), ("occupied", C.c_uint64),
                ("escaped", C.c_uint64), ("served", C.c_uint64), ("evaluations", C.c_uint64), ("inserted", C.c_uint64),
                ("overflowed", C.c_uint64), ("generation", C.c_uint64), ("retains", C.c_uint64), ("memo_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


_libs = {}


def load_library(diag=False):
    """Load libptmi.so (the product).  Raises if it has not been built: the product path has no fallback.
    diag=True loads libptmi_diag.so, the profiling / test build (only tests/ and scripts/ ask for it)."""
    if diag in _libs:
        return _libs[diag]
    path = library_path(diag)
    if not os.path.exists(path):
        raise FileNotFoundError(
            "%s not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')" % path)
    try:
        # torch bundles its own HIP runtime: when both live in one process it has to be loaded first, or torch later
        # finds "No HIP GPUs" (two copies of libamdhip64 with one SONAME).  No torch, no problem.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    L.pt_abi_version.restype = C.c_int
    if L.pt_abi_version() != ABI_VERSION:   # a stale in-tree build: the structs below would not match the library's
        raise RuntimeError("%s has ABI version %d, this binding needs %d: rebuild it (python -c 'import __graft_entry__ as g; "
                           "g.build()')" % (path, L.pt_abi_version(), ABI_VERSION))
    for sym in EXPORTS:   # same ABI version, fewer entry points: an in-tree build from before they were added
        if not hasattr(L, sym):
            raise RuntimeError("%s does not export %s: rebuild it (python -c 'import __graft_entry__ as g; g.build()')" % (path, sym))
    L.pt_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
    L.pt_destroy.argtypes = [C.c_void_p]
    L.pt_last_error.restype = C.c_char_p
    L.pt_last_error.argtypes = [C.c_void_p]
    L.pt_upload_nif.argtypes = [C.c_void_p, C.POINTER(Layer), C.c_uint32, C.c_uint32, C.c_float,
                                C.POINTER(C.c_float), C.c_int32]
    L.pt_set_constant_env.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.pt_set_render_settings.argtypes = [C.c_void_p, C.c_uint64, C.c_float, C.c_float, C.c_float, C.c_uint32]
    L.pt_setup.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.pt_path_trace.argtypes = [C.c_void_p]
    L.pt_read_results.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(Stats)]
    L.pt_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.pt_export_hdr_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.pt_comm_get_unique_id.argtypes = [C.c_void_p]
    L.pt_comm_init_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.pt_comm_init_all.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.pt_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.pt_comm_set_timeout.argtypes = [C.c_void_p, C.c_uint32]
    L.pt_comm_abort.argtypes = [C.c_void_p]
    L.pt_gather_hdr.argtypes = [C.c_void_p, C.c_int32, C.c_size_t, C.c_void_p]
    L.pt_film_accumulate.argtypes = [C.c_void_p]
    L.pt_film_seed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.pt_tile_costs_enable.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.pt_tile_costs.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.pt_clear_accumulators.argtypes = [C.c_void_p]
    L.pt_synchronize.argtypes = [C.c_void_p]
    L.pt_nif_infer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.pt_trace_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.pt_nif_kernel_name.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.pt_calibrate_nif.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.pt_runtime_info.argtypes = [C.c_char_p, C.c_size_t]
    L.pt_set_nif_sharing.argtypes = [C.c_void_p, C.c_int32]
    L.pt_get_nif_sharing_stats.argtypes = [C.c_void_p, C.POINTER(NifSharingStats)]
    L.pt_get_nif_class_stats.argtypes = [C.c_void_p, C.POINTER(NifClassStats)]
    L.pt_set_nif_memo.argtypes = [C.c_void_p, C.c_uint64]
    L.pt_clear_nif_memo.argtypes = [C.c_void_p]
    L.pt_get_nif_memo_stats.argtypes = [C.c_void_p, C.POINTER(NifMemoStats)]
    L.pt_set_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    L.pt_get_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.pt_set_scene_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
    L.pt_get_scene_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.pt_set_scene_meshes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Mesh), C.c_uint32]
    L.pt_get_mesh_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(MeshInfo)]
    L.pt_mesh_intersect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_set_mesh_normals.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
    L.pt_get_mesh_normals_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(MeshNormalsInfo)]
    L.pt_mesh_shade.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_set_mesh_texture.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(MeshTexture)]
    L.pt_get_mesh_texture_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(MeshTextureInfo)]
    L.pt_mesh_texel.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_set_mesh_build.argtypes = [C.c_void_p, C.POINTER(MeshBuildOptions)]
    L.pt_get_mesh_build_info.argtypes = [C.c_void_p, C.POINTER(MeshBuildInfo)]
    L.pt_set_mesh_device_tree.argtypes = [C.c_void_p, C.c_int32]
    L.pt_get_mesh_device_tree_info.argtypes = [C.c_void_p, C.POINTER(MeshDeviceTreeInfo)]
    L.pt_update_mesh_vertices.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(MeshUpdate)]
    L.pt_get_mesh_update_info.argtypes = [C.c_void_p, C.POINTER(MeshUpdateInfo)]
    L.pt_get_trace_variant.argtypes = [C.c_void_p, C.POINTER(TraceVariantInfo)]
    L.pt_mesh_tree.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
    L.pt_set_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
    L.pt_get_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
    L.pt_set_env_map.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32]
    L.pt_env_map_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.pt_set_env_guide.argtypes = [C.c_void_p, C.POINTER(EnvGuide)]
    L.pt_env_guide_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.pt_env_guide_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.pt_set_env_guide_from_environment.argtypes = [C.c_void_p, C.POINTER(EnvGuideAuto)]
    L.pt_get_env_guide_info.argtypes = [C.c_void_p, C.POINTER(EnvGuideInfo)]
    L.pt_get_env_guide_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.pt_set_light_guide.argtypes = [C.c_void_p, C.POINTER(LightGuide)]
    L.pt_set_light_guide_ex.argtypes = [C.c_void_p, C.POINTER(LightGuideEx)]
    L.pt_get_light_guide_flags.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.pt_get_light_guide_info.argtypes = [C.c_void_p, C.POINTER(LightGuideInfo)]
    L.pt_light_guide_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_void_p]
    L.pt_light_guide_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.pt_feature_buffers.argtypes = [C.c_void_p, C.POINTER(Features)]
    L.pt_denoise_default_params.argtypes = [C.POINTER(DenoiseParams)]
    L.pt_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.c_int32, C.c_void_p, C.c_void_p]
    L.pt_nif_train_default_params.argtypes = [C.POINTER(NifTrainParams)]
    L.pt_nif_train_begin.argtypes = [C.c_void_p, C.POINTER(NifTrainParams)]
    L.pt_nif_train_layer_shapes.argtypes = [C.c_void_p, C.POINTER(Layer), C.c_uint32]
    L.pt_nif_train_steps.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
    L.pt_nif_train_get_weights.argtypes = [C.c_void_p, C.POINTER(Layer), C.c_uint32]
    L.pt_nif_train_set_weights.argtypes = [C.c_void_p, C.POINTER(Layer), C.c_uint32]
    L.pt_nif_train_get_encode_params.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.pt_nif_train_export.argtypes = [C.c_void_p, C.POINTER(Layer), C.c_uint32]
    L.pt_nif_train_install.argtypes = [C.c_void_p]
    L.pt_nif_train_end.argtypes = [C.c_void_p]
    L.pt_nif_train_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_nif_train_default_precision.argtypes = [C.POINTER(NifTrainPrecision)]
    L.pt_nif_train_set_precision.argtypes = [C.c_void_p, C.POINTER(NifTrainPrecision)]
    L.pt_nif_train_get_precision_state.argtypes = [C.c_void_p, C.POINTER(NifTrainPrecisionState)]
    L.pt_nif_train_gradients.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_float),
                                         C.POINTER(Layer), C.c_uint32]
    if diag:
        L.pt_diag_set_nif_share_capacity.argtypes = [C.c_void_p, C.c_uint32]
        L.pt_diag_set_nif_memo_slots.argtypes = [C.c_void_p, C.c_uint32]
        L.pt_diag_claim_resolve.argtypes = [C.c_void_p, C.c_int32, C.c_uint32] + [C.c_void_p] * 3 + [C.c_uint32] * 3 + [C.c_void_p] * 7
        L.pt_diag_set_nif_class_capacity.argtypes = [C.c_void_p, C.c_uint32]
        L.pt_diag_expand_launches.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.pt_diag_class_claim.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 5
        L.pt_diag_share_class_claim.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 4 + [C.c_void_p] * 6
        L.pt_diag_class_map_claim.argtypes = [C.c_void_p] * 4 + [C.c_uint32] * 4 + [C.c_int32] + [C.c_void_p] * 5
        L.pt_diag_inject_fault.argtypes = [C.c_void_p, C.c_int32]
        L.pt_diag_stamps.argtypes = [C.c_void_p, C.c_void_p]
        L.pt_diag_nif_clock.argtypes = [C.c_void_p, C.c_void_p]
        L.pt_diag_comm_self_exchange.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int)]
        L.pt_diag_denoise_bench.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
    _libs[diag] = L
    return L


def degrees_to_radians_f32(deg):
    """PathTracerApp.cpp:574: float fov = deg * (M_PI / 180.f) evaluated in single precision."""
    return float(np.float32(deg) * np.float32(np.pi / 180.0))


def rotation_to_radians_f32(deg):
    """PathTracerApp.cpp:584: (degrees / 360.f) * (2.0 * M_PI)."""
    return float(np.float32((np.float32(deg) / np.float32(360.0)) * (2.0 * np.pi)))


class Renderer:
    """One device context (pt_handle).  Methods are named after the reference's Poplar programs."""

    def __init__(self, width, height, max_work_items=None, max_path_length=10, roulette_depth=3, stop_prob=0.3,
                 refractive_index=1.5, aa_noise_type=AA_NORMAL, sample_precision=SAMPLES_HALF, device=0,
                 iterations_per_batch=0, stream=None, diag=False):
        self._lib = load_library(diag)
        cfg = Config()
        cfg.struct_size = C.sizeof(Config)
        cfg.width, cfg.height = width, height
        self._width, self._height = width, height
        cfg.max_path_length, cfg.roulette_depth = max_path_length, roulette_depth
        cfg.stop_prob, cfg.refractive_index = stop_prob, refractive_index
        cfg.aa_noise_type, cfg.sample_precision = aa_noise_type, sample_precision
        cfg.device = device
        self._device = device
        cfg.max_work_items = max_work_items if max_work_items else width * height
        cfg.iterations_per_batch = iterations_per_batch
        cfg.stream = stream
        self.handle = C.c_void_p()
        rc = self._lib.pt_create(C.byref(cfg), C.byref(self.handle))
        if rc:
            msg = self._lib.pt_last_error(None).decode()
            self.handle = None
            raise PtError(rc, msg)
        self._keep = []

    def _check(self, rc):
        if rc:
            raise PtError(rc, self._lib.pt_last_error(self.handle).decode())

    def close(self):
        if getattr(self, "handle", None):
            self._lib.pt_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()

    # ---- program "init_nif_weights"
    def init_nif_weights(self, layers, embedding_dim, max_value, mean_folded, log_tonemap=True):
        arr = (Layer * len(layers))()
        keep = []
        for i, (k, b, relu) in enumerate(layers):
            # float32 kernels are handed over as float32 (the library rounds them to binary16, as documented in
            # include/ptmi.h); everything else is passed as float16, the type the reference's shipped NIFs use
            dt = np.float32 if np.asarray(k).dtype == np.float32 else np.float16
            k = np.ascontiguousarray(k, dtype=dt)
            keep.append(k)
            arr[i].rows, arr[i].cols = k.shape
            arr[i].kernel = k.ctypes.data
            if b is not None:
                b = np.ascontiguousarray(b, dtype=dt)
                keep.append(b)
                arr[i].bias = b.ctypes.data
            arr[i].dtype = DTYPE_F32 if dt == np.float32 else DTYPE_F16
            arr[i].relu = int(bool(relu))
        mean = (C.c_float * 3)(*[float(x) for x in mean_folded])
        self._check(self._lib.pt_upload_nif(self.handle, arr, len(layers), embedding_dim, float(max_value), mean,
                                            int(log_tonemap)))

    def set_constant_env(self, rgb):
        v = (C.c_float * 3)(*[float(x) for x in rgb])
        self._check(self._lib.pt_set_constant_env(self.handle, v))

    def set_env_map(self, bgr, filter="bilinear"):
        """An equirectangular HDR image as the environment light (include/ptmi.h, pt_set_env_map): an (H, W, 3) array in B, G, R
        order, rows top to bottom, finite and not negative; filter "nearest" or "bilinear" (or the ENV_FILTER_* numbers).
        Replaces a NIF or a constant environment; takes effect at the next path_trace.  A rejected map (PtError) leaves the
        previous environment in force."""
        if isinstance(filter, str):
            if filter not in ENV_FILTERS:
                raise ValueError("env-map filter must be one of %s, got %r" % (sorted(ENV_FILTERS), filter))
            filter = ENV_FILTERS[filter]
        bgr = np.ascontiguousarray(bgr, dtype=np.float32)
        if bgr.ndim != 3 or bgr.shape[2] != 3:
            raise ValueError("env map must have shape (H, W, 3), got %r" % (bgr.shape,))
        self._check(self._lib.pt_set_env_map(self.handle, bgr.ctypes.data, bgr.shape[1], bgr.shape[0], int(filter)))

    def env_map_lookup(self, u, v):
        """The BGR the map kernel looks up for (u, v), float32 [n, 3] (pt_env_map_lookup)."""
        u = np.ascontiguousarray(u, dtype=np.float32).ravel()
        v = np.ascontiguousarray(v, dtype=np.float32).ravel()
        if u.size != v.size:
            raise ValueError("u and v must have the same size")
        out = np.empty((u.size, 3), dtype=np.float32)
        self._check(self._lib.pt_env_map_lookup(self.handle, u.ctypes.data, v.ctypes.data, u.size, out.ctypes.data))
        return out

    def set_env_guide(self, bgr, rows=None, cols=None, alpha=0.5):
        """Guide diffuse bounces by an equirectangular HDR image (include/ptmi.h, pt_set_env_guide): an (H, W, 3) array as
        set_env_map takes it, a grid of rows x cols cells (powers of two; default: the largest not above the image or the caps)
        and the probability alpha in [0, 0.9] of drawing from the guide.  None clears the guide.  It changes how directions are
        sampled, not the light: any environment stays unbiased.  Takes effect at the next path_trace / trace_paths; a rejected
        guide (PtError) leaves the previous one in force."""
        if bgr is None:
            self._check(self._lib.pt_set_env_guide(self.handle, None))
            return
        bgr = np.ascontiguousarray(bgr, dtype=np.float32)
        if bgr.ndim != 3 or bgr.shape[2] != 3:
            raise ValueError("env guide image must have shape (H, W, 3), got %r" % (bgr.shape,))
        drows, dcols = default_env_guide_grid(bgr.shape[1], bgr.shape[0])
        g = EnvGuide()
        g.struct_size = C.sizeof(EnvGuide)
        g.width, g.height = bgr.shape[1], bgr.shape[0]
        g.rows, g.cols = int(drows if rows is None else rows), int(dcols if cols is None else cols)
        g.alpha = float(alpha)
        g.bgr = bgr.ctypes.data
        self._check(self._lib.pt_set_env_guide(self.handle, C.byref(g)))

    def set_env_guide_from_environment(self, rows=256, cols=512, alpha=0.5, supersample=2, follow=True):
        """Guide diffuse bounces by the environment in force -- the NIF, the map or the constant -- with no image in host memory
        (include/ptmi.h, pt_set_env_guide_from_environment): the guide of the image the environment gives at supersample x
        supersample points per cell of a rows x cols grid, its masses summed on the device.  follow: every later
        init_nif_weights, set_env_map, set_constant_env and trainer install rebuilds it from the new environment.  A rejected
        call (PtError) leaves the previous guide in force."""
        a = EnvGuideAuto(C.sizeof(EnvGuideAuto), int(rows), int(cols), int(supersample), float(alpha), int(follow))
        self._check(self._lib.pt_set_env_guide_from_environment(self.handle, C.byref(a)))

    def env_guide_info(self):
        """pt_get_env_guide_info as a dict: set, source ("image" or "environment"), rows, cols, supersample, alpha as used,
        follow, stale, rebuilds, clamped, build_ms."""
        info = EnvGuideInfo()
        info.struct_size = C.sizeof(EnvGuideInfo)
        self._check(self._lib.pt_get_env_guide_info(self.handle, C.byref(info)))
        return info.as_dict()

    def env_guide_tables(self):
        """The tables the device holds (pt_get_env_guide_tables): (threshold uint32 [n], alias uint32 [n], q float32 [n]),
        n = rows x cols in cell order."""
        info = self.env_guide_info()
        n = info["rows"] * info["cols"]
        thr, alias, q = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.float32)
        self._check(self._lib.pt_get_env_guide_tables(self.handle, thr.ctypes.data, alias.ctypes.data, q.ctypes.data, n))
        return thr, alias, q

    def env_guide_sample(self, g1, g2, g3):
        """The kernels' own guide sampling over caller words (pt_env_guide_sample): (uv float32 [n, 2], cell uint32 [n])."""
        w = [np.ascontiguousarray(x, dtype=np.uint32).ravel() for x in (g1, g2, g3)]
        if not (w[0].size == w[1].size == w[2].size):
            raise ValueError("g1, g2 and g3 must have the same size")
        n = w[0].size
        uv, cell = np.empty((n, 2), np.float32), np.empty(n, np.uint32)
        self._check(self._lib.pt_env_guide_sample(self.handle, w[0].ctypes.data, w[1].ctypes.data, w[2].ctypes.data, n,
                                                  uv.ctypes.data, cell.ctypes.data))
        return uv, cell

    def env_guide_eval(self, dir_world):
        """The kernels' own guide density over caller world directions [n, 3] (pt_env_guide_eval): (cell uint32 [n],
        g float32 [n]), g = 2 pi x the guide's solid-angle density."""
        d = np.ascontiguousarray(dir_world, dtype=np.float32).reshape(-1, 3)
        cell, g = np.empty(len(d), np.uint32), np.empty(len(d), np.float32)
        self._check(self._lib.pt_env_guide_eval(self.handle, d.ctypes.data, len(d), cell.ctypes.data, g.ctypes.data))
        return cell, g

    def set_light_guide(self, beta=0.5, polygons=False):
        """Guide diffuse bounces towards the scene's emitters (include/ptmi.h, pt_set_light_guide): with probability beta in
        [0, 0.9] a bounce draws its direction from an emissive sphere's visible cone or a point of an emissive disc.  None
        clears the guide.  It changes how directions are sampled, not the light; a scene without emitters leaves it inert.  The
        guide follows set_scene; a rejected one (PtError) leaves the previous one in force.  polygons=True
        (pt_set_light_guide_ex, PT_LIGHT_GUIDE_POLYGONS) draws from emissive triangles and parallelograms too, a uniform point of
        their area; polygons=False is pt_set_light_guide itself, which skips them."""
        if beta is None:
            self._check(self._lib.pt_set_light_guide(self.handle, None))
            return
        if polygons:
            gx = LightGuideEx(C.sizeof(LightGuideEx), float(beta), LIGHT_GUIDE_POLYGONS)
            self._check(self._lib.pt_set_light_guide_ex(self.handle, C.byref(gx)))
            return
        g = LightGuide(C.sizeof(LightGuide), float(beta))
        self._check(self._lib.pt_set_light_guide(self.handle, C.byref(g)))

    def light_guide_flags(self):
        """pt_get_light_guide_flags: the flags of the emitter guide in force (LIGHT_GUIDE_POLYGONS), 0 without one."""
        flags = C.c_uint32(0)
        self._check(self._lib.pt_get_light_guide_flags(self.handle, C.byref(flags)))
        return flags.value

    def light_guide_info(self):
        """pt_get_light_guide_info as a dict: set, active, beta, and per emitter object_index, threshold, probability."""
        info = LightGuideInfo()
        info.struct_size = C.sizeof(LightGuideInfo)
        self._check(self._lib.pt_get_light_guide_info(self.handle, C.byref(info)))
        k = info.n_lights
        return {"set": bool(info.set), "active": bool(info.active), "beta": info.beta, "n_lights": k,
                "object_index": np.array(info.object_index[:k], np.uint32), "threshold": np.array(info.threshold[:k], np.uint32),
                "probability": np.array(info.probability[:k], np.float32)}

    def light_guide_sample(self, origin, normal, g1, g2, g3):
        """The kernels' own emitter selection and draw over caller data in world space (pt_light_guide_sample):
        (dir float32 [n, 3], light int32 [n]: the rank drawn from, -1 where the selected emitter is not eligible)."""
        o = np.ascontiguousarray(origin, dtype=np.float32).reshape(-1, 3)
        nn = np.ascontiguousarray(normal, dtype=np.float32).reshape(-1, 3)
        w = [np.ascontiguousarray(x, dtype=np.uint32).ravel() for x in (g1, g2, g3)]
        n = len(o)
        if not (len(nn) == w[0].size == w[1].size == w[2].size == n):
            raise ValueError("origin, normal, g1, g2 and g3 must have the same length")
        d, light = np.zeros((n, 3), np.float32), np.full(n, -1, np.int32)
        self._check(self._lib.pt_light_guide_sample(self.handle, o.ctypes.data, nn.ctypes.data, w[0].ctypes.data, w[1].ctypes.data,
                                                    w[2].ctypes.data, n, d.ctypes.data, light.ctypes.data))
        return d, light

    def light_guide_eval(self, origin, normal, direction):
        """The kernels' own emitter density over caller (origin, normal, unit direction) triples in world space
        (pt_light_guide_eval): (sum over the eligible emitters of p_k g_k, float32 [n]; P_E, float32 [n])."""
        o = np.ascontiguousarray(origin, dtype=np.float32).reshape(-1, 3)
        nn = np.ascontiguousarray(normal, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(direction, dtype=np.float32).reshape(-1, 3)
        if not (len(o) == len(nn) == len(d)):
            raise ValueError("origin, normal and direction must have the same length")
        total, pe = np.zeros(len(o), np.float32), np.zeros(len(o), np.float32)
        self._check(self._lib.pt_light_guide_eval(self.handle, o.ctypes.data, nn.ctypes.data, d.ctypes.data, len(o),
                                                  total.ctypes.data, pe.ctypes.data))
        return total, pe

    # ---- program "init_render_settings"
    def init_render_settings(self, seed=1, aa_noise_scale=0.3, fov_degrees=90.0, env_rotation_degrees=0.0,
                             samples_per_step=1):
        self._check(self._lib.pt_set_render_settings(self.handle, seed, aa_noise_scale,
                                                     degrees_to_radians_f32(fov_degrees),
                                                     rotation_to_radians_f32(env_rotation_degrees), samples_per_step))

    # ---- programs "setup" / "path_trace" / "read_results"
    def setup(self, records):
        assert records.dtype == TRACE_DTYPE and records.flags.c_contiguous
        self._check(self._lib.pt_setup(self.handle, records.ctypes.data, records.size))

    def path_trace(self):
        self._check(self._lib.pt_path_trace(self.handle))

    def read_results(self, records):
        assert records.dtype == TRACE_DTYPE and records.flags.c_contiguous
        st = Stats()
        self._check(self._lib.pt_read_results(self.handle, records.ctypes.data, records.size, C.byref(st)))
        return st

    def stats(self):
        st = Stats()
        self._check(self._lib.pt_get_stats(self.handle, C.byref(st)))
        return st

    def nif_kernel_name(self):
        """The NIF kernel(s) the library dispatched at its last NIF launch ('' before the first)."""
        buf = C.create_string_buffer(512)
        self._check(self._lib.pt_nif_kernel_name(self.handle, buf, len(buf)))
        return buf.value.decode()

    def trace_variant(self):
        """pt_get_trace_variant: which instance of the trace kernels the last launch of each family took, as a dict of three
        dicts -- "trace" (path_trace), "paths" (trace_paths), "features" (feature_buffers / denoise) -- each of camera, bounce,
        geometry (TRACE_CAMERA_*, TRACE_BOUNCE_*, TRACE_GEOMETRY_*), index (the dense number in the family: of 57, 19 and 5) and
        launches.  Before a family's first launch its four coordinates are -1 and its count 0."""
        info = TraceVariantInfo(struct_size=C.sizeof(TraceVariantInfo))
        self._check(self._lib.pt_get_trace_variant(self.handle, C.byref(info)))
        return {"trace": info.trace.as_dict(), "paths": info.paths.as_dict(), "features": info.features.as_dict()}

    def calibrate_nif(self, launches=4):
        """The NIF stage of the last path_trace's largest batch again, alone on the device.
        Returns (milliseconds per launch, NIF evaluations per launch)."""
        ms, evals = C.c_double(), C.c_uint64()
        self._check(self._lib.pt_calibrate_nif(self.handle, launches, C.byref(ms), C.byref(evals)))
        return ms.value, evals.value

    def set_nif_sharing(self, mode):
        """Exact sharing of NIF evaluations between paths with bit-identical (u, v): "off", "batch" or "step"
        (include/ptmi.h, pt_set_nif_sharing).  Takes effect at the next path_trace.  A Renderer on which this is never called
        chooses per step: "step" with a NIF environment, the memo off and room in device memory, otherwise "off"; the first
        call, "off" included, ends that choice, and so does set_nif_memo.  nif_sharing_stats()["mode"] says what a step really ran."""
        if mode not in NIF_SHARE_MODES:
            raise ValueError("NIF sharing mode must be one of %s, got %r" % (sorted(NIF_SHARE_MODES), mode))
        self._check(self._lib.pt_set_nif_sharing(self.handle, NIF_SHARE_MODES[mode]))

    def set_nif_memo(self, max_bytes):
        """Persistent memo of decoded NIF values across steps, at most `max_bytes` of device memory; 0 turns it off
        (include/ptmi.h, pt_set_nif_memo).  Exact: the film is bit-identical to memo off."""
        self._check(self._lib.pt_set_nif_memo(self.handle, int(max_bytes)))

    def clear_nif_memo(self):
        """Forget every memo entry: the next path_trace starts a new generation."""
        self._check(self._lib.pt_clear_nif_memo(self.handle))

    def nif_memo_stats(self):
        """dict of enabled, slots, occupied, escaped, served, evaluations, inserted, overflowed, generation, retains, memo_ms."""
        st = NifMemoStats()
        st.struct_size = C.sizeof(NifMemoStats)
        self._check(self._lib.pt_get_nif_memo_stats(self.handle, C.byref(st)))
        d = st.as_dict()
        d["enabled"] = bool(d["enabled"])
        return d

    def nif_sharing_stats(self):
        """NIF rows the last path_trace really ran: dict of mode, escaped, evaluations, overflowed, table_slots, share_ms."""
        st = NifSharingStats()
        st.struct_size = C.sizeof(NifSharingStats)
        self._check(self._lib.pt_get_nif_sharing_stats(self.handle, C.byref(st)))
        d = st.as_dict()
        d["mode"] = {v: k for k, v in NIF_SHARE_MODES.items()}.get(d["mode"], d["mode"])
        return d

    def nif_class_stats(self):
        """The class level of the NIF stage in the last path_trace (include/ptmi.h, pt_nif_class_stats): dict of ran, mlp_rows
        (rows the NIF kernels executed), alone, table_slots, class_ms."""
        st = NifClassStats()
        st.struct_size = C.sizeof(NifClassStats)
        self._check(self._lib.pt_get_nif_class_stats(self.handle, C.byref(st)))
        d = st.as_dict()
        d["ran"] = bool(d["ran"])
        return d

    def set_scene(self, objects):
        """Render a scene of 1..32 spheres and discs instead of the built-in one (include/ptmi.h, pt_set_scene): a SCENE_DTYPE
        array or a list of dicts (scene_array).  A list that holds a "triangle" or a "parallelogram" (scene_array_ex), or a
        SCENE_EX_DTYPE array, goes through pt_set_scene_ex, and a list that holds a "mesh" (scene_meshes) through
        pt_set_scene_meshes.  None restores the built-in scene.  Takes effect at the next path_trace."""
        if objects is None:
            self._check(self._lib.pt_set_scene(self.handle, None, 0))
            return
        if has_mesh(objects):
            table, meshes = scene_meshes(objects)
            self.set_scene_meshes(table, meshes)
            for k, normals, indices in mesh_normals(objects):   # a mesh with "normals" shades smooth (pt_set_mesh_normals)
                self.set_mesh_normals(k, normals, indices)
            for k, image, uvs, indices, filt, wrap in mesh_textures(objects):   # a mesh with "texture" (pt_set_mesh_texture)
                self.set_mesh_texture(k, image, uvs, indices, filter=filt, wrap=wrap)
            return
        if (isinstance(objects, np.ndarray) and objects.dtype == SCENE_EX_DTYPE) or has_polygon(objects):
            # a triangle or a parallelogram (or an ex table as it is): pt_set_scene_ex, keys of scene_array_ex
            arr = scene_array_ex(objects)
            self._check(self._lib.pt_set_scene_ex(self.handle, arr.ctypes.data, arr.size, SCENE_EX_DTYPE.itemsize))
            return
        arr = scene_array(objects)
        self._check(self._lib.pt_set_scene(self.handle, arr.ctypes.data, arr.size))   # (an empty table is refused)

    def set_scene_meshes(self, table, meshes):
        """pt_set_scene_meshes as it is: a SCENE_EX_DTYPE table and, for its rows of shape 4 in order, (vertices, triangles)
        pairs.  The library copies everything; with no mesh this is pt_set_scene_ex."""
        table = scene_array_ex(table)
        keep = [(np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(t, dtype=np.uint32)) for v, t in meshes]
        arr = (Mesh * max(len(keep), 1))()
        for k, (v, t) in enumerate(keep):
            if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
                raise ValueError("mesh %d: vertices must have shape (V, 3) and triangles (T, 3)" % k)
            arr[k] = Mesh(C.sizeof(Mesh), len(v), len(t), v.ctypes.data, t.ctypes.data)
        self._check(self._lib.pt_set_scene_meshes(self.handle, table.ctypes.data, table.size, SCENE_EX_DTYPE.itemsize,
                                                  arr if keep else None, len(keep)))

    def mesh_info(self, k):
        """pt_get_mesh_info of mesh k of the scene in force as a dict: object_index, n_triangles, n_nodes, max_leaf, depth,
        device_bytes, build_ms, pad."""
        info = MeshInfo(struct_size=C.sizeof(MeshInfo))
        self._check(self._lib.pt_get_mesh_info(self.handle, int(k), C.byref(info)))
        return info.as_dict()

    def set_mesh_build(self, builder="host", on_pose="rebuild"):
        """pt_set_mesh_build: who builds the meshes' trees ("host": binned SAH on one host thread; "device": a linear BVH built by
        kernels) and what a pose change does to them ("rebuild", or "refit": topology and slot order stay, frames and boxes
        follow).  The options belong to the renderer and outlive the scene; the defaults are ("host", "rebuild")."""
        if builder not in MESH_BUILDERS:
            raise ValueError("builder must be one of %s (got %r)" % (sorted(MESH_BUILDERS), builder))
        if on_pose not in MESH_POSES:
            raise ValueError("on_pose must be one of %s (got %r)" % (sorted(MESH_POSES), on_pose))
        o = MeshBuildOptions(C.sizeof(MeshBuildOptions), MESH_BUILDERS[builder], MESH_POSES[on_pose])
        self._check(self._lib.pt_set_mesh_build(self.handle, C.byref(o)))

    def mesh_build_info(self):
        """pt_get_mesh_build_info as a dict: builder, on_pose, sort_on_device, host_builds, device_builds, refits, last_kind,
        last_ms, device_bytes."""
        info = MeshBuildInfo(struct_size=C.sizeof(MeshBuildInfo))
        self._check(self._lib.pt_get_mesh_build_info(self.handle, C.byref(info)))
        return info.as_dict()

    def set_mesh_device_tree(self, kind="linear"):
        """pt_set_mesh_device_tree: which tree the device builder builds -- "linear" (the default: a linear BVH) or "sah" (the
        host builder's binned-SAH tree, byte for byte, built by kernels).  The kind belongs to the renderer and outlives the
        scene; under set_mesh_build("host") it is accepted and inert."""
        if not isinstance(kind, str) or kind not in MESH_DEVICE_TREES:
            raise ValueError("kind must be one of %s (got %r)" % (sorted(MESH_DEVICE_TREES), kind))
        self._check(self._lib.pt_set_mesh_device_tree(self.handle, MESH_DEVICE_TREES[kind]))

    def mesh_device_tree_info(self):
        """pt_get_mesh_device_tree_info as a dict: kind, sah_builds, last_levels, last_ms, device_bytes."""
        info = MeshDeviceTreeInfo(struct_size=C.sizeof(MeshDeviceTreeInfo))
        self._check(self._lib.pt_get_mesh_device_tree_info(self.handle, C.byref(info)))
        return info.as_dict()

    def _update_array(self, what, a):
        """(pointer, rows, memory, keep-alive) of vertices / normals for pt_mesh_update: a float32 numpy array (or anything numpy
        converts), or a contiguous float32 torch tensor on this renderer's device, which is passed by its data_ptr()."""
        if type(a).__module__.split(".")[0] == "torch":
            import torch
            if a.dtype != torch.float32:
                raise ValueError("%s: a tensor must be float32 (got %s)" % (what, a.dtype))
            if a.device.type != "cuda" or a.device.index != getattr(self, "_device", 0):
                raise ValueError("%s: a tensor must lie on the renderer's device cuda:%d (got %s)" % (what, getattr(self, "_device", 0), a.device))
            if a.dim() != 2 or a.shape[1] != 3 or a.shape[0] == 0 or not a.is_contiguous():
                raise ValueError("%s must be a contiguous tensor of shape (N, 3), N >= 1" % what)
            return a.data_ptr(), int(a.shape[0]), MESH_UPDATE_DEVICE_MEMORY, a
        arr = np.ascontiguousarray(a, dtype=np.float32)
        if arr.ndim != 2 or arr.shape[1] != 3 or len(arr) == 0:
            raise ValueError("%s must be an array of shape (N, 3), N >= 1" % what)
        return arr.ctypes.data, len(arr), MESH_UPDATE_HOST_MEMORY, arr

    def update_mesh_vertices(self, k, vertices, normals=None, mode="refit"):
        """pt_update_mesh_vertices: new positions (V, 3) for the vertices of mesh k of the scene in force -- the same V, the same
        triangles -- and, for a mesh with normals, optionally new normals (N, 3) in the attached layout; normals None keeps the
        attached ones.  mode "refit" keeps the tree's topology and refits its boxes, "rebuild" builds the mesh's tree again.
        vertices / normals are float32 numpy arrays, or contiguous float32 torch tensors on the renderer's device: those are read
        in place, device to device, after torch's current stream has been synchronised.  Both must lie in the same memory."""
        if mode not in MESH_UPDATE_MODES:
            raise ValueError("mode must be one of %s (got %r)" % (sorted(MESH_UPDATE_MODES), mode))
        vp, nv, memory, keep_v = self._update_array("vertices", vertices)
        np_, nn, keep_n = None, 0, None
        if normals is not None:
            np_, nn, memory_n, keep_n = self._update_array("normals", normals)
            if memory_n != memory:
                raise ValueError("vertices and normals must both be numpy arrays or both be tensors on the device")
        if memory == MESH_UPDATE_DEVICE_MEMORY:
            import torch
            torch.cuda.current_stream(keep_v.device).synchronize()   # the writes are complete before the library reads
        u = MeshUpdate(struct_size=C.sizeof(MeshUpdate), mode=MESH_UPDATE_MODES[mode], memory=memory, n_vertices=nv, vertices=vp,
                       n_normals=nn, normals=np_)
        self._check(self._lib.pt_update_mesh_vertices(self.handle, int(k), C.byref(u)))
        del keep_v, keep_n

    def mesh_update_info(self):
        """pt_get_mesh_update_info as a dict: last_kind, updates, refits, rebuilds, fallbacks, last_frames_ms, last_tree_ms,
        device_bytes."""
        info = MeshUpdateInfo(struct_size=C.sizeof(MeshUpdateInfo))
        self._check(self._lib.pt_get_mesh_update_info(self.handle, C.byref(info)))
        return info.as_dict()

    def mesh_tree(self, k):
        """pt_mesh_tree: mesh k's tree as the kernels read it, brought up to date for the camera in force: (nodes, orig), nodes a
        MESH_NODE_DTYPE array of mesh_info(k)["n_nodes"] rows, orig the slot -> triangle map."""
        k = int(k)
        self._check(self._lib.pt_mesh_tree(self.handle, k, None, 0, None, 0))   # (the trees follow the camera: n_nodes may change)
        info = self.mesh_info(k)
        nodes = np.zeros(info["n_nodes"], MESH_NODE_DTYPE)
        orig = np.zeros(info["n_triangles"], np.uint32)
        self._check(self._lib.pt_mesh_tree(self.handle, k, nodes.ctypes.data, nodes.size, orig.ctypes.data, orig.size))
        return nodes, orig

    def mesh_intersect(self, origin, direction, brute=False):
        """pt_mesh_intersect: the kernels' nearest hit over world-space rays origin (n, 3), direction (n, 3), the camera ignored.
        Returns (t, object, triangle): t 0 for a miss, object -1 for a miss, triangle -1 unless a mesh was hit.  brute=True
        loops over all triangles of each mesh instead of walking its tree."""
        o = np.ascontiguousarray(origin, dtype=np.float32)
        d = np.ascontiguousarray(direction, dtype=np.float32)
        if o.ndim != 2 or o.shape[1] != 3 or o.shape != d.shape:
            raise ValueError("origin and direction must both have shape (n, 3)")
        n = len(o)
        t = np.zeros(n, np.float32)
        obj = np.full(n, -1, np.int32)
        tri = np.full(n, -1, np.int32)
        self._check(self._lib.pt_mesh_intersect(self.handle, o.ctypes.data, d.ctypes.data, n,
                                                MESH_INTERSECT_BRUTE if brute else MESH_INTERSECT_BVH,
                                                t.ctypes.data, obj.ctypes.data, tri.ctypes.data))
        return t, obj, tri

    def set_mesh_normals(self, k, normals, indices=None):
        """pt_set_mesh_normals: vertex normals (N, 3) for mesh k of the scene in force, which then shades smooth.  indices None:
        one normal per vertex, looked up by the mesh's own triangles; else (T, 3) indices into normals, per corner (creases).
        normals None removes them: the mesh is flat again.  The library copies everything."""
        if normals is None:
            if indices is not None:
                raise ValueError("indices without normals")
            self._check(self._lib.pt_set_mesh_normals(self.handle, int(k), None, 0, None))
            return
        nrm = np.ascontiguousarray(normals, dtype=np.float32)
        if nrm.ndim != 2 or nrm.shape[1] != 3 or len(nrm) == 0:
            raise ValueError("normals must be an array of shape (N, 3), N >= 1")
        idx = None
        if indices is not None:
            raw = np.asarray(indices)
            if raw.ndim != 2 or raw.shape[1] != 3 or not np.issubdtype(raw.dtype, np.integer) or raw.min() < 0 or raw.max() > 0xffffffff:
                raise ValueError("indices must be an array of shape (T, 3) of unsigned 32-bit indices")
            if len(raw) != self.mesh_info(k)["n_triangles"]:
                raise ValueError("indices must have one row per triangle of mesh %d (%d), got %d" % (k, self.mesh_info(k)["n_triangles"], len(raw)))
            idx = np.ascontiguousarray(raw, dtype=np.uint32)
        self._check(self._lib.pt_set_mesh_normals(self.handle, int(k), nrm.ctypes.data, len(nrm),
                                                  idx.ctypes.data if idx is not None else None))

    def mesh_normals_info(self, k):
        """pt_get_mesh_normals_info of mesh k of the scene in force as a dict: has_normals, per_corner, n_normals, device_bytes."""
        info = MeshNormalsInfo(struct_size=C.sizeof(MeshNormalsInfo))
        self._check(self._lib.pt_get_mesh_normals_info(self.handle, int(k), C.byref(info)))
        return info.as_dict()

    def mesh_shade(self, origin, direction):
        """pt_mesh_shade: the smooth kernels' nearest hit and shading normal over world-space rays origin (n, 3), direction (n, 3),
        the camera ignored.  Returns (t, object, triangle, bary (n, 2), normal (n, 3)): bary and normal are zero unless a mesh
        triangle was hit; the normal faces the ray."""
        o = np.ascontiguousarray(origin, dtype=np.float32)
        d = np.ascontiguousarray(direction, dtype=np.float32)
        if o.ndim != 2 or o.shape[1] != 3 or o.shape != d.shape:
            raise ValueError("origin and direction must both have shape (n, 3)")
        n = len(o)
        t = np.zeros(n, np.float32)
        obj = np.full(n, -1, np.int32)
        tri = np.full(n, -1, np.int32)
        bary = np.zeros((n, 2), np.float32)
        nrm = np.zeros((n, 3), np.float32)
        self._check(self._lib.pt_mesh_shade(self.handle, o.ctypes.data, d.ctypes.data, n, t.ctypes.data, obj.ctypes.data,
                                            tri.ctypes.data, bary.ctypes.data, nrm.ctypes.data))
        return t, obj, tri, bary, nrm

    def set_mesh_texture(self, k, image, uvs=None, indices=None, filter="bilinear", wrap="repeat"):
        """pt_set_mesh_texture: an image (H, W, 3) of linear float B,G,R, rows top to bottom, and texture coordinates uvs (N, 2) for
        mesh k of the scene in force.  indices None: one (s, t) per vertex, looked up by the mesh's own triangles; else (T, 3)
        indices into uvs, per corner (OBJ's v/vt).  filter "nearest" / "bilinear", wrap "repeat" / "clamp" (or the integer codes).
        image None removes the texture.  The library copies everything."""
        if image is None:
            if uvs is not None or indices is not None:
                raise ValueError("uvs or indices without an image")
            self._check(self._lib.pt_set_mesh_texture(self.handle, int(k), None))
            return
        img = np.ascontiguousarray(image, dtype=np.float32)
        if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
            raise ValueError("image must be an array of shape (H, W, 3), H, W >= 1")
        if img.shape[0] > MESH_TEXTURE_MAX_SIZE or img.shape[1] > MESH_TEXTURE_MAX_SIZE:
            raise ValueError("image must be at most %d x %d texels" % (MESH_TEXTURE_MAX_SIZE, MESH_TEXTURE_MAX_SIZE))
        if uvs is None:
            raise ValueError("an image needs uvs")
        uv = np.ascontiguousarray(uvs, dtype=np.float32)
        if uv.ndim != 2 or uv.shape[1] != 2 or len(uv) == 0:
            raise ValueError("uvs must be an array of shape (N, 2), N >= 1")
        if isinstance(filter, str):
            if filter not in TEX_FILTERS:
                raise ValueError("filter must be one of %s" % sorted(TEX_FILTERS))
            filter = TEX_FILTERS[filter]
        if isinstance(wrap, str):
            if wrap not in TEX_WRAPS:
                raise ValueError("wrap must be one of %s" % sorted(TEX_WRAPS))
            wrap = TEX_WRAPS[wrap]
        idx = None
        if indices is not None:
            raw = np.asarray(indices)
            if raw.ndim != 2 or raw.shape[1] != 3 or not np.issubdtype(raw.dtype, np.integer) or raw.min() < 0 or raw.max() > 0xffffffff:
                raise ValueError("indices must be an array of shape (T, 3) of unsigned 32-bit indices")
            if len(raw) != self.mesh_info(k)["n_triangles"]:
                raise ValueError("indices must have one row per triangle of mesh %d (%d), got %d" % (k, self.mesh_info(k)["n_triangles"], len(raw)))
            idx = np.ascontiguousarray(raw, dtype=np.uint32)
        t = MeshTexture(struct_size=C.sizeof(MeshTexture), width=img.shape[1], height=img.shape[0], filter=int(filter), wrap=int(wrap),
                        bgr=img.ctypes.data, uvs=uv.ctypes.data, n_uvs=len(uv), uv_indices=idx.ctypes.data if idx is not None else None)
        self._check(self._lib.pt_set_mesh_texture(self.handle, int(k), C.byref(t)))

    def mesh_texture_info(self, k):
        """pt_get_mesh_texture_info of mesh k of the scene in force as a dict: has_texture, per_corner, width, height, filter, wrap,
        n_uvs, device_bytes."""
        info = MeshTextureInfo(struct_size=C.sizeof(MeshTextureInfo))
        self._check(self._lib.pt_get_mesh_texture_info(self.handle, int(k), C.byref(info)))
        return info.as_dict()

    def mesh_texel(self, origin, direction):
        """pt_mesh_texel: the textured kernels' nearest hit, uv interpolation and lookup over world-space rays origin (n, 3),
        direction (n, 3), the camera ignored.  Returns (t, object, triangle, uv (n, 2), bgr (n, 3)): for a hit on a textured mesh
        the interpolated (s, t) and the texel (not multiplied by the row's colour); an untextured mesh triangle gives uv 0 and
        bgr 1; a miss or any other hit gives 0."""
        o = np.ascontiguousarray(origin, dtype=np.float32)
        d = np.ascontiguousarray(direction, dtype=np.float32)
        if o.ndim != 2 or o.shape[1] != 3 or o.shape != d.shape:
            raise ValueError("origin and direction must both have shape (n, 3)")
        n = len(o)
        t = np.zeros(n, np.float32)
        obj = np.full(n, -1, np.int32)
        tri = np.full(n, -1, np.int32)
        uv = np.zeros((n, 2), np.float32)
        bgr = np.zeros((n, 3), np.float32)
        self._check(self._lib.pt_mesh_texel(self.handle, o.ctypes.data, d.ctypes.data, n, t.ctypes.data, obj.ctypes.data,
                                            tri.ctypes.data, uv.ctypes.data, bgr.ctypes.data))
        return t, obj, tri, uv, bgr

    def scene_ex(self):
        """The scene in force as a SCENE_EX_DTYPE array (pt_get_scene_ex): a polygon with centre = v0, radius 0 and its stored
        normal, a sphere or disc with vertex 0."""
        n = C.c_uint32()
        out = np.zeros(MAX_SCENE_OBJECTS, dtype=SCENE_EX_DTYPE)
        self._check(self._lib.pt_get_scene_ex(self.handle, out.ctypes.data, MAX_SCENE_OBJECTS, C.byref(n)))
        return out[:n.value].copy()

    def scene(self):
        """The scene in force as a SCENE_DTYPE array (disc normals as the library normalised them).  A scene that holds a
        polygon raises PtError: scene_ex() reports it."""
        n = C.c_uint32()
        out = np.zeros(MAX_SCENE_OBJECTS, dtype=SCENE_DTYPE)
        self._check(self._lib.pt_get_scene(self.handle, out.ctypes.data, MAX_SCENE_OBJECTS, C.byref(n)))
        return out[:n.value].copy()

    def set_camera(self, position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), lens_radius=0.0,
                   focus_distance=1.0):
        """Place the camera (include/ptmi.h, pt_set_camera): position, the point it looks at, an up vector (need not be unit
        or orthogonal), and a thin lens of radius lens_radius focused at focus_distance along the view axis (0: pinhole).
        A lens given without focus_distance focuses at the default, 1.0 (ipu_trace --scene asks for the distance instead).
        set_camera(None) restores the built-in camera; a Camera struct is taken as it is.  Takes effect at the next
        path_trace / trace_paths; a rejected camera (PtError) leaves the previous one in force."""
        if position is None:
            self._check(self._lib.pt_set_camera(self.handle, None))
            return
        cam = position if isinstance(position, Camera) else make_camera(position, look_at, up, lens_radius, focus_distance)
        self._check(self._lib.pt_set_camera(self.handle, C.byref(cam)))

    def camera(self):
        """The camera in force as a Camera struct, values as given."""
        cam = Camera()
        self._check(self._lib.pt_get_camera(self.handle, C.byref(cam)))
        return cam

    def feature_buffers(self):
        """First-hit feature buffers of every pixel (include/ptmi.h, pt_feature_buffers): a dict of numpy arrays, object_id
        int32 [H, W] (-1: miss), depth float32 [H, W], normal float32 [H, W, 3] (world space, facing the camera) and albedo
        float32 [H, W, 3] (B, G, R).  The centre ray without AA noise or lens; needs init_render_settings, no worklist."""
        shape = (self._height, self._width)
        out = {"object_id": np.empty(shape, np.int32), "depth": np.empty(shape, np.float32),
               "normal": np.empty(shape + (3,), np.float32), "albedo": np.empty(shape + (3,), np.float32)}
        f = Features()
        f.struct_size = C.sizeof(Features)
        for k, a in out.items():
            setattr(f, k, a.ctypes.data)
        self._check(self._lib.pt_feature_buffers(self.handle, C.byref(f)))
        return out

    def denoise(self, image=None, source="film", **params):
        """The edge-avoiding A-trous filter of include/ptmi.h (pt_denoise) on the device; returns float32 [H, W, 3] (B, G, R).
        image: an [H, W, 3] B, G, R array to denoise; None: this handle's work items scattered into the frame, source "film"
        (the resident film / film steps) or "accumulators" (mean radiance).  params: fields of DenoiseParams (iterations,
        sigma_colour, sigma_normal, sigma_depth, object_stop, demodulate), the others at their defaults; or params=DenoiseParams."""
        p = params.pop("params") if "params" in params else default_denoise_params(**params)
        out = np.empty((self._height, self._width, 3), np.float32)
        if image is not None:
            image = np.ascontiguousarray(image, dtype=np.float32)
            if image.shape != out.shape:
                raise ValueError("image must have shape %r, got %r" % (out.shape, image.shape))
            src, ptr = DENOISE_HOST_IMAGE, image.ctypes.data
        else:
            if source not in DENOISE_SOURCES:
                raise ValueError("denoise source must be one of %s, got %r" % (sorted(DENOISE_SOURCES), source))
            src, ptr = DENOISE_SOURCES[source], None
        self._check(self._lib.pt_denoise(self.handle, C.byref(p), src, ptr, out.ctypes.data))
        return out

    def train_nif(self, params=None, precision=None, **overrides):
        """Start training a NIF on the environment map this renderer holds (include/ptmi.h, pt_nif_train_begin): returns a
        NifTrainer.  params: a NifTrainParams, or None for the library's defaults with any field overridden by keyword
        (embedding_dim, hidden, layer_count, batch, learning_rate, beta1, beta2, adam_eps, seed, log_tone_map, eps).  A
        renderer has one trainer at a time: a new one replaces the old.  precision: None (float32, as begin leaves it), "f32" /
        "mixed", a dict of NifTrainer.set_precision's keywords, or a NifTrainPrecision."""
        if params is None:
            params = default_nif_train_params(**overrides)
        elif overrides:
            raise ValueError("give params or keyword overrides, not both")
        self._check(self._lib.pt_nif_train_begin(self.handle, C.byref(params)))
        old = getattr(self, "_trainer", None)
        if old is not None:
            old._r = None          # the handle's trainer is the new one: the old object must not end or drive it
        self._trainer = NifTrainer(self, params)
        if precision is not None:
            if isinstance(precision, (str, NifTrainPrecision)):
                self._trainer.set_precision(precision)
            else:
                self._trainer.set_precision(**dict(precision))
        return self._trainer

    def export_hdr_device(self, device_ptr, n):
        self._check(self._lib.pt_export_hdr_device(self.handle, C.c_void_p(device_ptr), n))

    # ---- multi-GPU film hand-off (RCCL inside libptmi.so)
    def comm_init_rank(self, unique_id, rank, world):
        """Join the RCCL communicator made from `unique_id` (bytes from `comm_unique_id()` on rank 0)."""
        assert len(unique_id) == COMM_ID_BYTES
        buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.pt_comm_init_rank(self.handle, buf, rank, world))

    def comm_info(self):
        rank, world = C.c_int(), C.c_int()
        self._check(self._lib.pt_comm_info(self.handle, C.byref(rank), C.byref(world)))
        return rank.value, world.value

    def comm_set_timeout(self, milliseconds):
        """Deadline of every communicator operation of this handle (set-up, slot agreement, gather)."""
        self._check(self._lib.pt_comm_set_timeout(self.handle, int(milliseconds)))

    def comm_abort(self):
        """Ask the handle to abort its communicator; callable from another thread while a gather is waiting."""
        self._check(self._lib.pt_comm_abort(self.handle))

    def film_accumulate(self):
        """AccumulatedImage::accumulate + clearInactiveAccumulators on the device (the film stays resident)."""
        self._check(self._lib.pt_film_accumulate(self.handle))

    def film_seed(self, bgr):
        """Set the resident film of the current work items (float32 [n, 3] BGR running sums): the film follows its pixels."""
        bgr = np.ascontiguousarray(bgr, dtype=np.float32)
        self._check(self._lib.pt_film_seed(self.handle, bgr.ctypes.data, bgr.shape[0]))

    def tile_costs_enable(self, tile_w, tile_h):
        """Keep per-tile sums of pathLength on the device (what the path-length balancer needs: kilobytes, not the worklist)."""
        self._tile_grid = (tile_w, tile_h)
        self._check(self._lib.pt_tile_costs_enable(self.handle, tile_w, tile_h))

    def tile_costs(self, width, height):
        """uint64 [tiles]: per-tile sum of pathLength since the last setup (row-major grid of the enabled tile size)."""
        tw, th = self._tile_grid
        n = ((width + tw - 1) // tw) * ((height + th - 1) // th)
        out = np.zeros(n, dtype=np.uint64)
        self._check(self._lib.pt_tile_costs(self.handle, out.ctypes.data, n))
        return out

    def gather_hdr(self, slot_items, source=HDR_ACCUMULATORS):
        """One RCCL gather of HDR tiles to rank 0.  Returns float32 [world, slot_items, 3] (BGR) on rank 0, None elsewhere."""
        rank, world = self.comm_info()
        out = np.empty((world, slot_items, 3), dtype=np.float32) if rank == 0 else None
        self._check(self._lib.pt_gather_hdr(self.handle, source, slot_items, out.ctypes.data if out is not None else None))
        return out

    def clear_accumulators(self):
        self._check(self._lib.pt_clear_accumulators(self.handle))

    def synchronize(self):
        self._check(self._lib.pt_synchronize(self.handle))

    # ---- kernel-level entry points
    def nif_infer(self, u, v):
        u = np.ascontiguousarray(u, dtype=np.float32)
        v = np.ascontiguousarray(v, dtype=np.float32)
        out = np.empty((u.size, 3), dtype=np.float32)
        self._check(self._lib.pt_nif_infer(self.handle, u.ctypes.data, v.ctypes.data, u.size, out.ctypes.data))
        return out

    def trace_paths(self, u, v, sample_index):
        u = np.ascontiguousarray(u, dtype=np.uint16)
        v = np.ascontiguousarray(v, dtype=np.uint16)
        s = np.ascontiguousarray(sample_index, dtype=np.uint32)
        out = np.zeros(u.size, dtype=PATH_DTYPE)
        self._check(self._lib.pt_trace_paths(self.handle, u.ctypes.data, v.ctypes.data, s.ctypes.data, u.size,
                                             out.ctypes.data))
        return out


class NifTrainer:
    """The trainer of one Renderer (Renderer.train_nif).  Weights travel as [(kernel [in, out], bias [out], relu)] triples of
    float32 arrays, the layout of nif_assets.synthetic_nif; export() gives the same in float16."""

    def __init__(self, renderer, params):
        self._r = renderer
        self.params = params
        self._loss = None
        n = params.layer_count + 1
        arr = (Layer * n)()
        renderer._check(renderer._lib.pt_nif_train_layer_shapes(renderer.handle, arr, n))
        self.shapes = [(arr[i].rows, arr[i].cols, bool(arr[i].relu)) for i in range(n)]

    def _layers_out(self, dtype):
        arr = (Layer * len(self.shapes))()
        out = []
        for i, (rows, cols, relu) in enumerate(self.shapes):
            k, b = np.empty((rows, cols), dtype), np.empty(cols, dtype)
            arr[i].rows, arr[i].cols, arr[i].kernel, arr[i].bias = rows, cols, k.ctypes.data, b.ctypes.data
            out.append((k, b, relu))
        return arr, out

    def _call(self, fn, *args):
        if self._r is None:
            raise PtError(-5, "this NifTrainer is closed, or a later Renderer.train_nif() has replaced it")
        self._r._check(getattr(self._r._lib, fn)(self._r.handle, *args))

    def steps(self, n=1):
        """n Adam steps; returns the loss of the last one (before its update)."""
        loss = C.c_float()
        self._call("pt_nif_train_steps", int(n), C.byref(loss))
        if n:
            self._loss = loss.value
        return self._loss

    def loss(self):
        """The loss steps() returned last (None before the first step)."""
        return self._loss

    def weights(self):
        arr, out = self._layers_out(np.float32)
        self._call("pt_nif_train_get_weights", arr, len(out))
        return out

    def set_weights(self, layers):
        """Replace the float32 master weights; resets the Adam moments and the step counter."""
        arr = (Layer * len(layers))()
        keep = []
        for i, (k, b, relu) in enumerate(layers):
            k = np.ascontiguousarray(k, dtype=np.float32)
            keep.append(k)
            arr[i].rows, arr[i].cols = k.shape
            arr[i].kernel = k.ctypes.data
            if b is not None:
                b = np.ascontiguousarray(b, dtype=np.float32)
                keep.append(b)
                arr[i].bias = b.ctypes.data
            arr[i].dtype, arr[i].relu = DTYPE_F32, int(bool(relu))
        self._call("pt_nif_train_set_weights", arr, len(layers))

    def encode_params(self):
        """{"max", "mean" (as computed, not folded), "eps", "log_tone_map"}."""
        mx, mean = C.c_float(), (C.c_float * 3)()
        self._call("pt_nif_train_get_encode_params", C.byref(mx), mean)
        return {"max": mx.value, "mean": [mean[0], mean[1], mean[2]], "eps": float(np.float32(self.params.eps)),
                "log_tone_map": bool(self.params.log_tone_map)}

    def metadata(self, image_shape):
        """The dict nif_assets.write_metadata takes, for an image of shape (H, W)."""
        enc = self.encode_params()
        return {"embedding_dimension": self.params.embedding_dim, "hidden_size": self.params.hidden,
                "layer_count": self.params.layer_count, "eps": enc["eps"], "log_tone_map": enc["log_tone_map"], "max": enc["max"],
                "mean": enc["mean"], "original_image_shape": [int(image_shape[0]), int(image_shape[1]), 3]}

    def export(self):
        """The layers rounded to float16 (round to nearest even)."""
        arr, out = self._layers_out(np.float16)
        self._call("pt_nif_train_export", arr, len(out))
        return out

    def install(self):
        """Make the exported NIF the renderer's environment (pt_upload_nif of export()); training can go on afterwards."""
        self._call("pt_nif_train_install")

    def batch(self, step):
        """(u, v, target [batch, 3]) of the batch step `step` draws."""
        n = self.params.batch
        u, v, t = np.empty(n, np.float32), np.empty(n, np.float32), np.empty((n, 3), np.float32)
        self._call("pt_nif_train_batch", int(step), u.ctypes.data, v.ctypes.data, t.ctypes.data)
        return u, v, t

    def gradients(self, u, v, target):
        """(loss, [(dW, db, relu)]) of the current weights on the given samples; moves nothing."""
        u = np.ascontiguousarray(u, dtype=np.float32).ravel()
        v = np.ascontiguousarray(v, dtype=np.float32).ravel()
        t = np.ascontiguousarray(target, dtype=np.float32).reshape(-1, 3)
        if not (u.size == v.size == t.shape[0]):
            raise ValueError("u, v and target must have the same number of samples")
        arr, out = self._layers_out(np.float32)
        loss = C.c_float()
        self._call("pt_nif_train_gradients", u.ctypes.data, v.ctypes.data, t.ctypes.data, u.size, C.byref(loss), arr, len(out))
        return loss.value, out

    def set_precision(self, mode="mixed", **fields):
        """Switch the precision mode between steps (pt_nif_train_set_precision): mode "mixed" / "f32" (or a NifTrainPrecision),
        fields loss_scale, dynamic, growth_interval.  Keeps weights, moments and applied steps; resets the scale's state."""
        p = mode if isinstance(mode, NifTrainPrecision) else default_nif_train_precision(mode=mode, **fields)
        self._call("pt_nif_train_set_precision", C.byref(p))

    def precision_state(self):
        """{"mode": "f32" | "mixed", "loss_scale", "good_steps", "applied_steps", "skipped_steps"}."""
        s = NifTrainPrecisionState()
        s.struct_size = C.sizeof(NifTrainPrecisionState)
        self._call("pt_nif_train_get_precision_state", C.byref(s))
        names = {v: k for k, v in NIF_TRAIN_MODES.items()}
        return {"mode": names[s.mode], "loss_scale": s.loss_scale, "good_steps": s.good_steps, "applied_steps": s.applied_steps,
                "skipped_steps": s.skipped_steps}

    def close(self):
        if self._r is not None and getattr(self._r, "handle", None):
            self._call("pt_nif_train_end")
            self._r._trainer = None
        self._r = None


def runtime_info(diag=False):
    """Which librccl / libamdhip64 the library's imports are bound to in THIS process, and their versions (pt_runtime_info)."""
    import json
    lib = load_library(diag)
    buf = C.create_string_buffer(2048)
    rc = lib.pt_runtime_info(buf, len(buf))
    if rc:
        raise PtError(rc, lib.pt_last_error(None).decode())
    return json.loads(buf.value.decode())


def comm_unique_id():
    """ncclGetUniqueId through the C-ABI: rank 0 makes it and hands the bytes to the other ranks."""
    lib = load_library()
    buf = (C.c_char * COMM_ID_BYTES)()
    rc = lib.pt_comm_get_unique_id(buf)
    if rc:
        raise PtError(rc, lib.pt_last_error(None).decode())
    return bytes(buf)


def worklist(width, height):
    """createWorkListForImage (src/LoadBalancer.cpp:38-52): one item per pixel, row-major (c, r)."""
    rec = np.zeros(width * height, dtype=TRACE_DTYPE)
    rr, cc = np.divmod(np.arange(width * height), width)
    rec["u"] = cc
    rec["v"] = rr
    return rec
