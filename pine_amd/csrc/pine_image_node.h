// pine_amd/csrc/pine_image_node.h -- NodeImage's lookup (node.cpp:20-27, image.cpp:7-17), written once: the kernels'
// node evaluator runs it per hit, and the host folds a `Texture` whose coordinate does not read the surface with it -- this
// header needs pine_math.h and pine_types.h alone, so a plain C++ build of the host code includes it.
#pragma once
#include "pine_math.h"
#include "pine_types.h"

namespace pine_gpu {

// NodeImage's texel index along one axis (node.cpp:21): fract, float(size) * fract in binary32, truncation, min(., size - 1).
// Where fract rounds to exactly 1.0 (a tiny negative coordinate: p = -1e-9) the product is `size`: only the min keeps that read inside.  Where the reference converts a NaN to an
// int (a non-finite coordinate: undefined, and it reads outside its array), the index here is 0.
PINE_HD int image_axis_index(float p, int size) {
  const float s = float(size) * (p - floorf(p));
  if (!(s >= 0.0f)) return 0;
  if (s >= float(size)) return size - 1;
  const int i = int(s);
  return i < size - 1 ? i : size - 1;
}
// Image::operator[](vec2i) as vec3 (image.cpp:7-17): column x of row y, rows as loaded; `image` = the image's first word.
PINE_HD f3 image_lookup(const float* table, const float* image, int w, int h, bool u8, f3 p) {
  const long long i = (long long)image_axis_index(p.x, w) + (long long)image_axis_index(p.y, h) * w;
  if (u8) {
    const unsigned t = unsigned(as_int(image[i]));
    return f3{table[t & 255u], table[(t >> 8) & 255u], table[(t >> 16) & 255u]};
  }
  return ld3(image + i * 3);
}

}  // namespace pine_gpu
