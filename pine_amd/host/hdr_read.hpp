// pine_amd/host/hdr_read.hpp -- Radiance HDR (.hdr / RGBE) reader: what the reference's image loader (stb's stbi_loadf, 3
// channels) returns for such a file -- w * h * 3 floats, rows top first.  `#?RADIANCE` / `#?RGBE` headers,
// FORMAT=32-bit_rle_rgbe, `-Y h +X w` only, flat and new-style run-length encoded scanlines; each channel is
// mantissa * ldexp(1, e - 136), zero where e = 0.  Anything else is refused by name (there is no PNG / JPEG decoder in this
// tree).  Header-only; pine_amd/hdr.py is the same reader in Python.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace pine {

struct HdrImage {
  int w = 0, h = 0;
  std::vector<float> rgb;  // 3 per texel
};

inline HdrImage read_hdr_bytes(const std::vector<unsigned char>& data, const std::string& name) {
  auto refuse = [&](const char* why) -> void {
    throw std::runtime_error("`" + name + "` is no Radiance HDR image this reader takes (" + why + "); other image formats enter as arrays");
  };
  size_t pos = 0;
  auto line = [&]() {
    size_t end = pos;
    while (end < data.size() && data[end] != '\n') end++;
    if (end >= data.size()) refuse("truncated header");
    std::string s(data.begin() + long(pos), data.begin() + long(end));
    pos = end + 1;
    return s;
  };
  const std::string sig = line();
  if (sig != "#?RADIANCE" && sig != "#?RGBE") refuse("no #?RADIANCE / #?RGBE signature");
  bool format = false;
  for (;;) {
    const std::string s = line();
    if (s.empty()) break;
    if (s == "FORMAT=32-bit_rle_rgbe") format = true;
  }
  if (!format) refuse("FORMAT is not 32-bit_rle_rgbe");
  HdrImage img;
  {
    const std::string s = line();
    char tail = 0;
    if (sscanf(s.c_str(), "-Y %d +X %d%c", &img.h, &img.w, &tail) != 2) refuse("orientation is not -Y h +X w");
  }
  if (img.w < 1 || img.h < 1 || (long long)img.w * img.h > (1ll << 26)) refuse("bad image size");
  const size_t w = size_t(img.w), h = size_t(img.h);
  std::vector<unsigned char> rgbe(w * h * 4);
  auto flat = [&]() {
    if (pos + rgbe.size() > data.size()) refuse("truncated pixels");
    memcpy(rgbe.data(), data.data() + pos, rgbe.size());
  };
  bool rle = w >= 8 && w < 32768;
  if (!rle) flat();
  for (size_t j = 0; rle && j < h; j++) {
    if (pos + 4 > data.size()) refuse("truncated pixels");
    const unsigned char* p = data.data() + pos;
    if (p[0] != 2 || p[1] != 2 || (p[2] & 0x80)) {
      if (j != 0) refuse("a scanline that is not run-length encoded after one that is");
      flat();  // not run-length encoded: the four bytes were the first pixel
      break;
    }
    pos += 4;
    if ((size_t(p[2]) << 8 | p[3]) != w) refuse("scanline width");
    for (int k = 0; k < 4; k++)
      for (size_t i = 0; i < w;) {
        if (pos >= data.size()) refuse("truncated pixels");
        size_t count = data[pos++];
        const bool run = count > 128;
        if (run) count -= 128;
        if (count == 0 || count > w - i || pos + (run ? 1 : count) > data.size()) refuse("corrupt run");
        for (size_t c = 0; c < count; c++) rgbe[(j * w + i + c) * 4 + size_t(k)] = data[pos + (run ? 0 : c)];
        pos += run ? 1 : count;
        i += count;
      }
  }
  img.rgb.resize(w * h * 3);
  for (size_t i = 0; i < w * h; i++) {
    const unsigned char* p = &rgbe[i * 4];
    const float f = p[3] ? std::ldexp(1.0f, int(p[3]) - 136) : 0.0f;
    for (int k = 0; k < 3; k++) img.rgb[i * 3 + size_t(k)] = p[3] ? float(p[k]) * f : 0.0f;
  }
  return img;
}

inline HdrImage read_hdr(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open `" + path + "`");
  std::vector<unsigned char> data;
  unsigned char buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + n);
  fclose(f);
  return read_hdr_bytes(data, path);
}

}  // namespace pine
