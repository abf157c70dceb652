// Test infrastructure (not product): for every file given on the command line, reads the whole file and then every proper
// prefix of it (written to <dir>/cut<ext>) through env_map::read, exactly as the host does.  Built with
// -fsanitize=address,undefined by tests/test_env_map_reader.py: a truncated file must end in a std::exception that names the
// file and an offset (counted), never in a sanitizer report (the process aborts with a non-zero status) or in an image.
#include <cstdio>
#include <cstring>
#include <exception>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "EnvMapReader.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string dir = argv[1];
  int whole = 0, rejected = 0, accepted = 0, unnamed = 0;
  for (int i = 2; i < argc; ++i) {
    const std::string file = argv[i];
    const std::string ext = file.substr(file.find_last_of('.'));
    try {
      whole += !env_map::read(file).bgr.empty();
    } catch (const std::exception& e) {
      std::printf("whole file refused: %s\n", e.what());
    }
    std::ifstream f(file, std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const std::string cut = dir + "/cut" + ext;
    for (std::size_t n = 0; n < raw.size(); ++n) {
      { std::ofstream o(cut, std::ios::binary | std::ios::trunc); o.write(raw.data(), (std::streamsize)n); }
      try {
        (void)env_map::read(cut);
        accepted += 1;
        std::printf("accepted: %s cut at %zu\n", file.c_str(), n);
      } catch (const std::exception& e) {
        rejected += 1;
        const std::string what = e.what();
        if (what.find(cut) == std::string::npos || what.find("offset") == std::string::npos) { unnamed += 1; std::printf("unnamed: %s\n", what.c_str()); }
      }
    }
  }
  std::printf("whole %d rejected %d accepted %d unnamed %d\n", whole, rejected, accepted, unnamed);
  return 0;
}
