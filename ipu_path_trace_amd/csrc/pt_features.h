// pt_features.h -- first-hit feature buffers (pt_feature_buffers, include/ptmi.h): object id, depth, world-space normal and
// albedo of what every pixel's centre ray sees.  An EXTENSION: the reference has no such output.
//
// One thread per pixel of width x height (every pixel, whatever the worklist holds).  The ray is the production camera ray
// without AA noise and without the lens: start_path itself runs on a copy of the launch parameters whose aa_scale is 0, so
// hround(aa_scale * n) is a zero, c = (float)u and r = (float)v exactly, and camx, camy, the normalisation and the direction
// are start_path's own expressions (the Philox block it draws for the noise is multiplied away: a few hundred instructions per
// pixel, once per scene / camera / settings change).  The hit is nearest_hit_primary over the table in the kernel arguments,
// which is in camera space when a pose is set: the same function on the same ray as the production kernels' primary phase, so
// the object index is theirs bit for bit (with aa_noise_scale = 0 and the lens off).  The lens is ignored on purpose: a guide
// image must be sharp.
//
// Two packed float4 per pixel, the handle's feature cache (the denoiser reads them as they are):
//   f0 = (nx, ny, nz, depth)           f1 = (albedo B, albedo G, albedo R, bits of the object index)
#pragma once
#include "pt_trace.h"

namespace ptd {

constexpr int kFeatureBlock = 256;

template <bool POLY, bool MESH = false, bool SMOOTH = false, bool TEX = false>
__device__ __forceinline__ void features_body(const TraceParams& P, float4* __restrict__ f0, float4* __restrict__ f1,
                                              [[maybe_unused]] const TexParams* X = nullptr) {
  const uint32_t i = blockIdx.x * kFeatureBlock + threadIdx.x;
  if (i >= P.width * P.height) return;   // width, height <= 65535: the product fits 32 bits
  const uint32_t v = i / P.width, u = i - v * P.width;
  PathState st;
  float camx, camy, tbest;
  start_path(P, u | (v << 16), 0u, st, camx, camy);   // P.aa_scale == 0 (the host's copy): the noise-free ray
  if constexpr (MESH) {
    // On the image's middle row py = -(+0 x ty) = -0, so camy and d.y are -0.  In this instance the compiler folds the rounding to
    // half into a fused multiply-add with a +0 addend, which turns that -0 into +0; the other instances keep it.  The sign is put
    // back, so that a sphere centred on the camera's horizontal plane gets the normal.y = -0 there that the other instances report.
    if (camy == 0.0f) st.d.y = -0.0f;
  }
  int best = nearest_hit_primary<false, POLY, MESH>(P, st.d, tbest);
  [[maybe_unused]] const int packed = best;   // a MESH instance's hit is packed: `best` becomes the object's row, what the buffer reports
  if constexpr (MESH) best = packed < 0 ? -1 : hit_object<true>(packed);
  Vec3 n = mk(0.f, 0.f, 0.f), alb = mk(1.f, 1.f, 1.f);
  float depth = 0.f;
  if (best >= 0) {
    const SceneObject ob = P.obj[best];
    depth = tbest;
    // sphere: (hit - centre) / |hit - centre| -- (hit - centre) / radius but for the rounding of the hit point, and unit to
    // rounding as the production shading forms it (shade_hit); disc or polygon (shape code >= 1): its stored normal
    n = ob.is_disc ? mk(ob.nx, ob.ny, ob.nz) : normalise(sub(scale(st.d, tbest), mk(ob.cx, ob.cy, ob.cz)));
    if constexpr (MESH) {   // a mesh: the hit triangle's stored normal
      if (ob.is_disc == SHAPE_MESH) {
        const ptmesh::F4 tn = P.mesh_tris[3u * (size_t)hit_slot(packed) + 2u];
        n = mk(tn.y, tn.z, tn.w);
        if constexpr (SMOOTH) {   // pt_set_mesh_normals: the shading normal of the centre ray, as shade_hit forms it (rules 1-4)
          if (__float_as_uint(P.poly[best].e2y) != 0u) {
            const size_t slot = (size_t)hit_slot(packed);
            const float ov[3] = {0.f, 0.f, 0.f}, dv[3] = {st.d.x, st.d.y, st.d.z}, ng[3] = {tn.y, tn.z, tn.w};
            float a, b, ns[3];
            ptmesh::shading_normal(ov, dv, ptmesh::load_tri(P.mesh_tris + 3u * slot), ng, P.mesh_normals + 3u * slot, a, b, ns);
            n = mk(ns[0], ns[1], ns[2]);
          }
        }
      }
    }
    if (dot(n, st.d) > 0.0f) n = scale(n, -1.0f);                     // faces the ray
    if (P.cam_pose) n = normalise(to_world(P, n));                    // reported in world space; unit again after the rotation's roundings
    if (ob.type == MAT_DIFFUSE || ob.type == MAT_REFRACTIVE) alb = mk(ob.colr, ob.colg, ob.colb);   // mirrors, emitters and misses demodulate by 1
    if constexpr (TEX) {   // pt_set_mesh_texture: colour x texel at the centre ray's hit, the product shade_hit forms (rules 1-5)
      if (ob.is_disc == SHAPE_MESH && __float_as_uint(P.poly[best].e2z) != 0u && (ob.type == MAT_DIFFUSE || ob.type == MAT_REFRACTIVE)) {
        texture_colour(P, *X, best, packed, mk(0.f, 0.f, 0.f), st.d, alb.x, alb.y, alb.z);
      }
    }
  }
  f0[i] = make_float4(n.x, n.y, n.z, depth);
  f1[i] = make_float4(alb.z, alb.y, alb.x, __int_as_float(best));     // B, G, R like every image of the ABI
}

// One instance per geometry level of ptmi_trace_variant.h, launched while the scene in force is at that level: a polygon
// (pt_set_scene_ex), a mesh (pt_set_scene_meshes), vertex normals (pt_set_mesh_normals), a texture (pt_set_mesh_texture: the
// instance with the second argument, TexParams of pt_trace.h).
template <int GEOM>
__global__ __launch_bounds__(kFeatureBlock) void features_kernel(const TraceParams P, float4* __restrict__ f0, float4* __restrict__ f1) {
  static_assert(GEOM != GEOM_TEX, "a TEX instance takes TexParams: features_kernel_tex");
  using F = VariantFlags<0, GEOM>;   // the bounce plays no part
  features_body<F::POLY, F::MESH, F::SMOOTH, F::TEX>(P, f0, f1);
}
__global__ __launch_bounds__(kFeatureBlock) void features_kernel_tex(const TraceParams P, const TexParams X, float4* __restrict__ f0, float4* __restrict__ f1) {
  using F = VariantFlags<0, GEOM_TEX>;
  features_body<F::POLY, F::MESH, F::SMOOTH, F::TEX>(P, f0, f1, &X);
}

}  // namespace ptd
