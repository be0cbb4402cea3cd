// tools/png_read_main.cpp -- a stand-alone program around pine_amd/host/png_read.hpp, for tests/test_png_reader.py, which builds
// it with -fsanitize=address,undefined and runs it over the reader fixtures and over seeded mutations of them.
//
//   png_read_main <channels> <list.txt>      list.txt: one file name per line
//
// Per file one line: `ok <w> <h> <texels in hex>` or `refused <message>`.  The exit status is 0 whatever the files hold; a
// crash or a sanitizer report is what the test looks for.
#include <cstdio>
#include <fstream>
#include <string>

#include "../pine_amd/host/png_read.hpp"

int main(int argc, char** argv) {
  if (argc != 3) return fprintf(stderr, "usage: png_read_main <channels> <list.txt>\n"), 2;
  const int channels = atoi(argv[1]);
  std::ifstream list(argv[2]);
  if (!list) return fprintf(stderr, "cannot open %s\n", argv[2]), 2;
  std::string path;
  while (std::getline(list, path)) {
    if (path.empty()) continue;
    try {
      const pine::PngImage img = pine::read_png(path, channels);
      std::string hex;
      static const char digits[] = "0123456789abcdef";
      for (unsigned char c : img.texels) hex += digits[c >> 4], hex += digits[c & 15];
      printf("ok %d %d %s\n", img.w, img.h, hex.c_str());
    } catch (const std::exception& e) {
      printf("refused %s\n", e.what());
    }
  }
  return 0;
}
