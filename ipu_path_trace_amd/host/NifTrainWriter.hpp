// Writers of the two asset files a trained NIF is kept in (ipu_trace --train-nif): nif_metadata.txt with the fields
// NifMetaData reads (NifModel.cpp; reference src/neural_networks/NifMetaData.cpp:11-71) and the flat converted.ptnif that
// NifModel::Data::setupModel reads.  Header-only and free of any device or library call, so the sanitizer program of the
// tests builds it on its own.
#pragma once
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace nif_train {

/// One dense layer as it goes into converted.ptnif: binary16 kernel [rows][cols] and bias [cols].
struct HalfLayer {
  std::uint32_t rows = 0, cols = 0;
  bool relu = false;
  std::vector<std::uint16_t> kernel, bias;
};

struct MetaData {
  std::string name;
  std::uint32_t embeddingDimension = 0, hiddenSize = 0, layerCount = 0;
  std::uint32_t imageHeight = 0, imageWidth = 0;
  float eps = 0.f, max = 0.f, mean[3] = {0.f, 0.f, 0.f};   ///< mean as computed: the loaders fold -eps into it
  bool logToneMap = true;
  std::string precision = "f32";   ///< --train-precision, recorded in train_command when it is not the default
};

inline std::string jsonString(const std::string& s) {
  std::string out = "\"";
  for (const char c : s) {
    if (c == '"' || c == '\\') { out += '\\'; out += c; }
    else if ((unsigned char)c < 0x20) { char buf[8]; std::snprintf(buf, sizeof buf, "\\u%04x", (unsigned)(unsigned char)c); out += buf; }
    else out += c;
  }
  return out + "\"";
}

/// A float with the nine significant digits that round-trip binary32.
inline std::string jsonFloat(float v) {
  char buf[48];
  std::snprintf(buf, sizeof buf, "%.9g", (double)v);
  return buf;
}

inline std::string metadataText(const MetaData& m) {
  std::string t = "{\n";
  t += "  \"embedding_dimension\": " + std::to_string(m.embeddingDimension) + ",\n";
  t += "  \"encode_params\": {\n";
  t += "    \"eps\": " + jsonFloat(m.eps) + ",\n";
  t += std::string("    \"log_tone_map\": ") + (m.logToneMap ? "true" : "false") + ",\n";
  t += "    \"max\": " + jsonFloat(m.max) + ",\n";
  t += "    \"mean\": [" + jsonFloat(m.mean[0]) + ", " + jsonFloat(m.mean[1]) + ", " + jsonFloat(m.mean[2]) + "],\n";
  t += std::string("    \"transfer_function\": ") + (m.logToneMap ? "\"log\"" : "\"linear\"") + "\n  },\n";
  t += "  \"name\": " + jsonString(m.name) + ",\n";
  t += "  \"original_image_shape\": [" + std::to_string(m.imageHeight) + ", " + std::to_string(m.imageWidth) + ", 3],\n";
  t += "  \"train_command\": [\"ipu_trace\", \"--train-nif\", \"--layer-count\", \"" + std::to_string(m.layerCount) + "\", \"--layer-size\", \"" +
       std::to_string(m.hiddenSize) + "\", \"--embedding-dimension\", \"" + std::to_string(m.embeddingDimension) + "\"" +
       (m.precision == "f32" ? std::string() : ", \"--train-precision\", " + jsonString(m.precision)) + "]\n";
  return t + "}\n";
}

inline void writeMetadata(const std::string& path, const MetaData& m) {
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  const std::string text = metadataText(m);
  f.write(text.data(), (std::streamsize)text.size());
  f.flush();
  if (!f) throw std::runtime_error("could not write '" + path + "'");
}

/// "PTNIF1\0\0", u32 n_layers, u32 embedding_dim, then per layer u32 rows, cols, dtype (0 = float16), relu, has_bias and the raw
/// kernel and bias bytes.  Refuses a layer whose buffers do not have the sizes its shape says.
inline void writePtnif(const std::string& path, const std::vector<HalfLayer>& layers, std::uint32_t embeddingDimension) {
  if (layers.empty() || layers.size() > 16) throw std::runtime_error("converted.ptnif: layer count must be in 1..16");
  for (std::size_t l = 0; l < layers.size(); ++l)
    if (layers[l].rows == 0 || layers[l].cols == 0 || layers[l].kernel.size() != (std::size_t)layers[l].rows * layers[l].cols ||
        layers[l].bias.size() != layers[l].cols)
      throw std::runtime_error("converted.ptnif: layer " + std::to_string(l) + " does not have the sizes of its shape");
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  f.write("PTNIF1\0\0", 8);
  const std::uint32_t head[2] = {(std::uint32_t)layers.size(), embeddingDimension};
  f.write((const char*)head, sizeof head);
  for (const HalfLayer& l : layers) {
    const std::uint32_t hdr[5] = {l.rows, l.cols, 0u, l.relu ? 1u : 0u, 1u};
    f.write((const char*)hdr, sizeof hdr);
    f.write((const char*)l.kernel.data(), (std::streamsize)(l.kernel.size() * 2));
    f.write((const char*)l.bias.data(), (std::streamsize)(l.bias.size() * 2));
  }
  f.flush();
  if (!f) throw std::runtime_error("could not write '" + path + "'");
}

}  // namespace nif_train
