// ipu_trace --train-nif: train a NIF on an HDR image with the library's trainer (pt_nif_train_*, include/ptmi.h) and write
// the assets ipu_trace --assets reads.  An extension: the reference sends its users to an external TensorFlow script.
#pragma once
#include <string>
#include <vector>

#include "Options.hpp"

namespace nif_train {

/// The --train-* options, appended to the tool's option list.
void addOptions(std::vector<OptionSpec>& specs);
/// True when --train-nif names a file: the tool then trains instead of rendering, and --outfile / --assets are not needed.
bool requested(const OptionMap& args);
/// Validates the arguments and the image (no device), then -- unless --compile-only -- trains and writes
/// DIR/assets.extra/nif_metadata.txt and DIR/assets.extra/converted.ptnif.  Throws std::runtime_error naming what is wrong.
void run(const OptionMap& args);

}  // namespace nif_train
