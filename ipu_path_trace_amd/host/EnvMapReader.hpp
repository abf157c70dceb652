// Dependency-free readers of the image formats an equirectangular HDR environment map comes in (ipu_trace --env-map,
// pt_set_env_map): Radiance .hdr / .pic (RGBE), .pfm and the OpenEXR subset image_io::writeExr produces.  An extension: the
// reference renders with a NIF trained on such an image and never reads one itself.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

namespace env_map {

/// Largest width or height accepted (PT_ENV_MAP_MAX_SIZE of include/ptmi.h).
constexpr std::size_t kMaxSize = 16384;

struct Image {
  std::size_t width = 0, height = 0;
  std::vector<float> bgr;   ///< height x width x 3 floats in B,G,R order, rows top to bottom (what pt_set_env_map takes)
};

/// Reads `fileName` by its extension, case-insensitive:
///   .hdr / .pic  Radiance: "#?RADIANCE" or "#?RGBE", FORMAT=32-bit_rle_rgbe, flat and adaptive-RLE scanlines, orientation
///                "-Y H +X W" only; a pixel is mantissa * 2^(e - 136) per channel (0 for e == 0).  EXPOSURE and COLORCORR
///                lines are not applied.
///   .pfm         "PF" (three channels), little- or big-endian by the sign of the scale (its magnitude is not applied), rows
///                bottom to top in the file.
///   .exr         version 2 scanline files with exactly the FLOAT channels B, G, R, no compression, increasing line order.
/// Throws std::runtime_error naming the file and the byte offset for a file that is truncated, corrupt or outside these
/// subsets; never reads out of bounds.  Values are returned as stored (the library refuses a negative or non-finite texel).
Image read(const std::string& fileName);

}  // namespace env_map
