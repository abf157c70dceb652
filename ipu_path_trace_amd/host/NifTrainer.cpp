#include "NifTrainer.hpp"

#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <stdexcept>

#include "../csrc/ptmi_nif_train_check.h"
#include "EnvMapReader.hpp"
#include "NifTrainWriter.hpp"
#include "logging.hpp"
#include "ptmi.h"

namespace nif_train {

void addOptions(std::vector<OptionSpec>& specs) {
  const pt_nif_train_params d = ptniftrain::defaults();
  specs.push_back({"train-nif", 0, "", false, false, "FILE.hdr|.pfm|.exr: train a NIF on this equirectangular HDR image on the device instead of rendering, and write DIR/assets.extra/nif_metadata.txt and converted.ptnif (--train-out DIR) for a later --assets DIR/assets.extra. --outfile and --assets are not needed. With --compile-only the arguments and the file are validated without a device."});
  specs.push_back({"train-steps", 0, "1000", false, false, "Adam steps of --train-nif."});
  specs.push_back({"train-out", 0, "", false, false, "Directory --train-nif writes assets.extra/ into."});
  specs.push_back({"train-layer-size", 0, std::to_string(d.hidden), false, false, "Hidden width of the trained NIF, a multiple of 32 in 32..1024."});
  specs.push_back({"train-layer-count", 0, std::to_string(d.layer_count), false, false, "Hidden layers of the trained NIF, 1..15."});
  specs.push_back({"train-embedding-dimension", 0, std::to_string(d.embedding_dim), false, false, "Fourier frequencies per coordinate of the trained NIF, 1..15."});
  specs.push_back({"train-batch", 0, std::to_string(d.batch), false, false, "Texels per Adam step, a multiple of 256."});
  specs.push_back({"train-learning-rate", 0, "0.001", false, false, "Adam learning rate."});
  specs.push_back({"train-seed", 0, "1", false, false, "Seed of the weight initialisation and of the batches."});
  specs.push_back({"train-precision", 0, "f32", false, false, "f32|mixed: precision of the trainer's matrix products. mixed = binary16 inputs with loss scaling and binary32 master weights (pt_nif_train_set_precision)."});
  specs.push_back({"train-loss-scale", 0, "65536", false, false, "Initial loss scale of --train-precision mixed, a power of two in 1..2^30."});
  specs.push_back({"train-loss-scale-static", 0, "false", false, true, "Keep the loss scale of --train-precision mixed fixed (no halving on overflow, no growth)."});
}

bool requested(const OptionMap& args) { return args.has("train-nif") && !args.str("train-nif").empty(); }

namespace {

std::uint64_t number(const OptionMap& args, const char* name) {
  const std::string& text = args.str(name);
  std::size_t used = 0;
  unsigned long long v = 0;
  try { v = std::stoull(text, &used); } catch (const std::exception&) { used = 0; }
  if (text.empty() || used != text.size() || text[0] == '-') throw std::runtime_error(std::string("--") + name + " must be a non-negative integer; got '" + text + "'");
  return v;
}

void makeDirectory(const std::string& path) {
  struct stat st;
  if (::mkdir(path.c_str(), 0777) != 0 && !(::stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode)))
    throw std::runtime_error("--train-out: could not create the directory '" + path + "'");
}

void check(pt_handle h, int rc, const char* what) {
  if (rc) throw std::runtime_error(std::string(what) + " failed: " + pt_last_error(h));
}

}  // namespace

void run(const OptionMap& args) {
  const std::string file = args.str("train-nif");
  pt_nif_train_params p = ptniftrain::defaults();
  p.hidden = (std::uint32_t)std::min<std::uint64_t>(number(args, "train-layer-size"), 0xffffffffu);
  p.layer_count = (std::uint32_t)std::min<std::uint64_t>(number(args, "train-layer-count"), 0xffffffffu);
  p.embedding_dim = (std::uint32_t)std::min<std::uint64_t>(number(args, "train-embedding-dimension"), 0xffffffffu);
  p.batch = (std::uint32_t)std::min<std::uint64_t>(number(args, "train-batch"), 0xffffffffu);
  p.seed = number(args, "train-seed");
  try { p.learning_rate = args.f32("train-learning-rate"); } catch (const std::exception&) { p.learning_rate = NAN; }
  const std::string bad = ptniftrain::check(&p);
  if (!bad.empty()) throw std::runtime_error("--train-nif: " + bad);
  pt_nif_train_precision prec = ptniftrain::default_precision();
  const std::string precision = args.str("train-precision");
  if (precision != "f32" && precision != "mixed") throw std::runtime_error("--train-precision must be f32 or mixed; got '" + precision + "'");
  prec.mode = precision == "mixed" ? PT_NIF_TRAIN_MIXED_F16 : PT_NIF_TRAIN_F32;
  try { prec.loss_scale = args.f32("train-loss-scale"); } catch (const std::exception&) { prec.loss_scale = NAN; }
  prec.dynamic = args.flag("train-loss-scale-static") ? 0 : 1;
  const std::string bad_precision = ptniftrain::check_precision(&prec);
  if (!bad_precision.empty()) throw std::runtime_error("--train-nif: " + bad_precision);
  const std::uint64_t steps = number(args, "train-steps");
  if (steps < 1 || steps > 0xffffffffu) throw std::runtime_error("--train-steps must be at least 1; got " + args.str("train-steps"));
  const std::string out = args.str("train-out");
  if (out.empty()) throw std::runtime_error("--train-nif needs --train-out DIR");
  env_map::Image img;
  try {
    img = env_map::read(file);
  } catch (const std::exception& e) {
    throw std::runtime_error(std::string("--train-nif ") + e.what());
  }
  for (std::size_t i = 0; i < img.bgr.size(); ++i)
    if (!(img.bgr[i] >= 0.f) || !std::isfinite(img.bgr[i]))
      throw std::runtime_error("--train-nif '" + file + "': texel at row " + std::to_string(i / 3 / img.width) + ", column " + std::to_string(i / 3 % img.width) +
                               ", channel " + std::to_string(i % 3) + " is " + std::to_string(img.bgr[i]) + ": texels must be finite and not negative");
  pt_log::info_("Training image '{}': {} x {}; NIF {} x {}, embedding {}, batch {}, {} steps, precision {}", file, img.width, img.height, p.layer_count,
                p.hidden, p.embedding_dim, p.batch, steps, precision);
  if (args.flag("compile-only")) {
    pt_log::info_("Compile only mode selected: finished.");
    return;
  }
  pt_config cfg{};
  cfg.struct_size = sizeof(pt_config);
  cfg.width = cfg.height = 32;   // no image is rendered: the handle is there for its device, its stream and the map
  cfg.max_path_length = 1; cfg.roulette_depth = 1; cfg.stop_prob = 0.3f; cfg.refractive_index = 1.5f;
  cfg.sample_precision = PT_SAMPLES_HALF;
  cfg.device = args.has("devices") && !args.str("devices").empty() ? std::atoi(args.str("devices").c_str()) : 0;
  cfg.max_work_items = 32 * 32;
  pt_handle h = nullptr;
  if (pt_create(&cfg, &h)) throw std::runtime_error(std::string("Could not attach to device: ") + pt_last_error(nullptr));
  struct Closer { pt_handle h; ~Closer() { pt_destroy(h); } } closer{h};
  check(h, pt_set_env_map(h, img.bgr.data(), (std::uint32_t)img.width, (std::uint32_t)img.height, PT_ENV_FILTER_NEAREST), "set_env_map");
  check(h, pt_nif_train_begin(h, &p), "nif_train_begin");
  if (prec.mode != PT_NIF_TRAIN_F32) check(h, pt_nif_train_set_precision(h, &prec), "nif_train_set_precision");
  const std::uint32_t interval = (std::uint32_t)std::max<std::uint64_t>(1, steps / 10);
  float loss = 0.f;
  for (std::uint64_t done = 0; done < steps;) {
    const std::uint32_t n = (std::uint32_t)std::min<std::uint64_t>(interval, steps - done);
    check(h, pt_nif_train_steps(h, n, &loss), "nif_train_steps");
    done += n;
    pt_log::info_("Training step {} of {}: loss {}", done, steps, loss);
  }
  const std::vector<ptniftrain::Shape> shapes = ptniftrain::shapes(p);
  std::vector<HalfLayer> layers(shapes.size());
  std::vector<pt_layer> views(shapes.size());
  for (std::size_t l = 0; l < shapes.size(); ++l) {
    layers[l].rows = shapes[l].rows; layers[l].cols = shapes[l].cols; layers[l].relu = shapes[l].relu;
    layers[l].kernel.resize((std::size_t)shapes[l].rows * shapes[l].cols);
    layers[l].bias.resize(shapes[l].cols);
    views[l] = pt_layer{shapes[l].rows, shapes[l].cols, layers[l].kernel.data(), layers[l].bias.data(), PT_DTYPE_F16, shapes[l].relu ? 1 : 0};
  }
  check(h, pt_nif_train_export(h, views.data(), (std::uint32_t)views.size()), "nif_train_export");
  MetaData meta;
  meta.name = file;
  meta.embeddingDimension = p.embedding_dim; meta.hiddenSize = p.hidden; meta.layerCount = p.layer_count;
  meta.imageHeight = (std::uint32_t)img.height; meta.imageWidth = (std::uint32_t)img.width;
  meta.eps = p.eps; meta.logToneMap = p.log_tone_map != 0;
  meta.precision = precision;
  check(h, pt_nif_train_get_encode_params(h, &meta.max, meta.mean), "nif_train_get_encode_params");
  pt_nif_train_precision_state state{};
  state.struct_size = sizeof(state);
  check(h, pt_nif_train_get_precision_state(h, &state), "nif_train_get_precision_state");
  check(h, pt_nif_train_end(h), "nif_train_end");
  makeDirectory(out);
  makeDirectory(out + "/assets.extra");
  writeMetadata(out + "/assets.extra/nif_metadata.txt", meta);
  writePtnif(out + "/assets.extra/converted.ptnif", layers, p.embedding_dim);
  pt_log::info_("Wrote '{}/assets.extra/nif_metadata.txt' and 'converted.ptnif' (final loss {}; precision {}, loss scale {}, {} steps applied, {} skipped)", out,
                loss, precision, state.loss_scale, state.applied_steps, state.skipped_steps);
}

}  // namespace nif_train
