// pine_amd/host/png_read.hpp -- PNG reader: the bytes the reference's image loaders return for such a file -- w * h * channels
// bytes, rows top first.  PNG is lossless, so a correct decoder returns exactly what stb_image returns: channels = 3 is what
// the reference's image_from asks stb for, 4 what tinygltf asks for.  Bit depth 8, colour types 0 (grey), 2 (rgb), 3 (palette,
// alpha from tRNS), 4 (grey + alpha) and 6 (rgba), non-interlaced; a tRNS colour key of a grey or rgb image gives alpha 0, as
// in stb.  Expansion as stb does it: grey becomes r = g = b, a missing alpha is 255, a dropped alpha is simply dropped.
// Refused by name: 16-bit samples, depths below 8, interlaced images, and every damaged file -- chunk lengths and CRCs, the
// zlib header and Adler-32, each row's filter byte and the decompressed size are checked.  The inflate (RFC 1951) is this
// file's own, so nothing new is linked.  Header-only; pine_amd/png.py is the same reader in Python.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace pine {

struct PngImage {
  int w = 0, h = 0, channels = 0;
  std::vector<unsigned char> texels;
};

namespace png_detail {

struct Refused : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline uint32_t crc32(const unsigned char* p, size_t n) {
  static uint32_t table[256];
  static bool made = false;
  if (!made) {
    for (uint32_t i = 0; i < 256; i++) {
      uint32_t c = i;
      for (int k = 0; k < 8; k++) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
      table[i] = c;
    }
    made = true;
  }
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; i++) c = table[(c ^ p[i]) & 255] ^ (c >> 8);
  return c ^ 0xffffffffu;
}

// Canonical Huffman decoding table of one alphabet (RFC 1951 3.2.2): symbols sorted by code, counts per length.
struct Huffman {
  uint16_t count[16] = {};
  uint16_t symbol[288] = {};
  bool build(const uint8_t* lengths, int n) {
    memset(count, 0, sizeof count);
    for (int i = 0; i < n; i++) count[lengths[i]]++;
    if (count[0] == n) return true;  // no codes: decoding with it fails
    int left = 1;
    for (int len = 1; len < 16; len++) {
      left <<= 1;
      left -= count[len];
      if (left < 0) return false;  // over-subscribed
    }
    uint16_t offs[16];
    offs[1] = 0;
    for (int len = 1; len < 15; len++) offs[len + 1] = uint16_t(offs[len] + count[len]);
    for (int i = 0; i < n; i++)
      if (lengths[i]) symbol[offs[lengths[i]]++] = uint16_t(i);
    return true;
  }
};

struct Bits {
  const unsigned char* p;
  size_t n, pos = 0;
  uint32_t buf = 0;
  int cnt = 0;
  int bit() {
    if (cnt == 0) {
      if (pos >= n) throw Refused("truncated IDAT stream");
      buf = p[pos++];
      cnt = 8;
    }
    const int b = int(buf & 1);
    buf >>= 1;
    cnt--;
    return b;
  }
  uint32_t bits(int need) {
    uint32_t v = 0;
    for (int i = 0; i < need; i++) v |= uint32_t(bit()) << i;
    return v;
  }
  int decode(const Huffman& h) {
    int code = 0, first = 0, index = 0;
    for (int len = 1; len < 16; len++) {
      code |= bit();
      const int c = h.count[len];
      if (code - c < first) return h.symbol[index + (code - first)];
      index += c;
      first += c;
      first <<= 1;
      code <<= 1;
    }
    throw Refused("IDAT does not inflate: a code that is in no table");
  }
};

// zlib stream (RFC 1950) -> at most `limit` bytes; more, or a damaged stream, is refused.
inline std::vector<unsigned char> inflate(const std::vector<unsigned char>& z, size_t limit) {
  if (z.size() < 6) throw Refused("truncated IDAT stream");
  if ((z[0] & 15) != 8 || (z[0] >> 4) > 7 || ((unsigned(z[0]) << 8) | z[1]) % 31 != 0 || (z[1] & 32)) throw Refused("IDAT does not inflate: bad zlib header");
  static const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  static const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  static const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  static const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  Bits in{z.data() + 2, z.size() - 2};
  std::vector<unsigned char> out;
  auto put = [&](unsigned char c) {
    if (out.size() >= limit) throw Refused("IDAT holds more bytes than the image needs");
    out.push_back(c);
  };
  for (bool last = false; !last;) {
    last = in.bit() != 0;
    const uint32_t type = in.bits(2);
    if (type == 0) {
      in.cnt = 0;  // to the byte boundary
      if (in.pos + 4 > in.n) throw Refused("truncated IDAT stream");
      const unsigned len = in.p[in.pos] | unsigned(in.p[in.pos + 1]) << 8, nlen = in.p[in.pos + 2] | unsigned(in.p[in.pos + 3]) << 8;
      in.pos += 4;
      if ((len ^ 0xffffu) != nlen) throw Refused("IDAT does not inflate: stored block length");
      if (in.pos + len > in.n) throw Refused("truncated IDAT stream");
      for (unsigned i = 0; i < len; i++) put(in.p[in.pos + i]);
      in.pos += len;
      continue;
    }
    if (type == 3) throw Refused("IDAT does not inflate: block type 3");
    Huffman lit, dist;
    uint8_t lengths[320];
    if (type == 1) {
      for (int i = 0; i < 288; i++) lengths[i] = uint8_t(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
      lit.build(lengths, 288);
      for (int i = 0; i < 30; i++) lengths[i] = 5;
      dist.build(lengths, 30);
    } else {
      const int nlen = int(in.bits(5)) + 257, ndist = int(in.bits(5)) + 1, ncode = int(in.bits(4)) + 4;
      if (nlen > 286 || ndist > 30) throw Refused("IDAT does not inflate: too many codes");
      uint8_t cl[19] = {};
      for (int i = 0; i < ncode; i++) cl[order[i]] = uint8_t(in.bits(3));
      Huffman lencode;
      if (!lencode.build(cl, 19)) throw Refused("IDAT does not inflate: code lengths");
      for (int i = 0; i < nlen + ndist;) {
        const int sym = in.decode(lencode);
        if (sym < 16) {
          lengths[i++] = uint8_t(sym);
          continue;
        }
        uint8_t value = 0;
        int rep;
        if (sym == 16) {
          if (i == 0) throw Refused("IDAT does not inflate: repeat without a length");
          value = lengths[i - 1];
          rep = 3 + int(in.bits(2));
        } else if (sym == 17) rep = 3 + int(in.bits(3));
        else rep = 11 + int(in.bits(7));
        if (i + rep > nlen + ndist) throw Refused("IDAT does not inflate: too many lengths");
        while (rep--) lengths[i++] = value;
      }
      if (lengths[256] == 0) throw Refused("IDAT does not inflate: no end-of-block code");
      if (!lit.build(lengths, nlen) || !dist.build(lengths + nlen, ndist)) throw Refused("IDAT does not inflate: code lengths");
    }
    for (;;) {
      const int sym = in.decode(lit);
      if (sym < 256) {
        put((unsigned char)sym);
      } else if (sym == 256) {
        break;
      } else {
        if (sym > 285) throw Refused("IDAT does not inflate: length symbol");
        const size_t len = lbase[sym - 257] + in.bits(lext[sym - 257]);
        const int ds = in.decode(dist);
        if (ds > 29) throw Refused("IDAT does not inflate: distance symbol");
        const size_t d = dbase[ds] + in.bits(dext[ds]);
        if (d > out.size()) throw Refused("IDAT does not inflate: distance before the start");
        for (size_t i = 0; i < len; i++) put(out[out.size() - d]);
      }
    }
  }
  in.cnt = 0;
  if (in.pos + 4 > in.n) throw Refused("truncated IDAT stream");
  uint32_t a = 1, b = 0;
  for (unsigned char c : out) {
    a = (a + c) % 65521u;
    b = (b + a) % 65521u;
  }
  const unsigned char* t = in.p + in.pos;
  if (((b << 16) | a) != (uint32_t(t[0]) << 24 | uint32_t(t[1]) << 16 | uint32_t(t[2]) << 8 | t[3])) throw Refused("IDAT does not inflate: Adler-32");
  return out;
}

}  // namespace png_detail

inline PngImage read_png_bytes(const std::vector<unsigned char>& data, int channels, const std::string& name) {
  using png_detail::Refused;
  try {
    if (channels != 3 && channels != 4) throw Refused("channels is 3 or 4");
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    if (data.size() < 8 || memcmp(data.data(), sig, 8) != 0) throw Refused("no PNG signature");
    auto be32 = [&](size_t at) { return uint32_t(data[at]) << 24 | uint32_t(data[at + 1]) << 16 | uint32_t(data[at + 2]) << 8 | data[at + 3]; };
    size_t pos = 8;
    bool have_header = false, ended = false, have_trns = false;
    uint32_t w = 0, h = 0;
    int depth = 0, ctype = 0, compression = 0, filter = 0, interlace = 0;
    std::vector<unsigned char> palette, trns, idat;
    bool any_idat = false;
    while (!ended) {
      if (data.size() - pos < 12) throw Refused("truncated: a chunk header or CRC is missing");
      const uint32_t length = be32(pos);
      const std::string kind(data.begin() + long(pos) + 4, data.begin() + long(pos) + 8);
      std::string shown = kind;  // (for messages: a damaged file's chunk type may hold any byte)
      for (char& c : shown)
        if (!((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))) c = '?';
      if (length > data.size() - pos - 12) throw Refused("truncated: chunk " + shown + " is longer than the file");
      const unsigned char* body = data.data() + pos + 8;
      if (png_detail::crc32(data.data() + pos + 4, 4 + size_t(length)) != be32(pos + 8 + length)) throw Refused("bad CRC in chunk " + shown);
      pos += 12 + size_t(length);
      if (!have_header && kind != "IHDR") throw Refused("the first chunk is not IHDR");
      if (kind == "IHDR") {
        if (have_header || length != 13) throw Refused("bad IHDR");
        have_header = true;
        w = uint32_t(body[0]) << 24 | uint32_t(body[1]) << 16 | uint32_t(body[2]) << 8 | body[3];
        h = uint32_t(body[4]) << 24 | uint32_t(body[5]) << 16 | uint32_t(body[6]) << 8 | body[7];
        depth = body[8], ctype = body[9], compression = body[10], filter = body[11], interlace = body[12];
      } else if (kind == "PLTE") {
        if (length == 0 || length % 3 || length > 768) throw Refused("bad PLTE length");
        palette.assign(body, body + length);
      } else if (kind == "tRNS") {
        if (any_idat) throw Refused("tRNS after IDAT");
        trns.assign(body, body + length);
        have_trns = true;
      } else if (kind == "IDAT") {
        idat.insert(idat.end(), body, body + length);
        any_idat = true;
      } else if (kind == "IEND") {
        ended = true;
      } else if (!(kind[0] & 32)) {
        throw Refused("unknown critical chunk " + shown);
      }
    }
    if (w < 1 || h < 1 || uint64_t(w) * h > (1ull << 26)) throw Refused("a size below 1 or more than 2^26 texels");
    const int bpp = ctype == 0 ? 1 : ctype == 2 ? 3 : ctype == 3 ? 1 : ctype == 4 ? 2 : ctype == 6 ? 4 : 0;
    if (!bpp) throw Refused("colour type " + std::to_string(ctype));
    if (depth == 16) throw Refused("16-bit samples are not supported");
    if (depth != 8) throw Refused("bit depth " + std::to_string(depth) + ": depths below 8 are not supported");
    if (interlace) throw Refused("interlaced images are not supported");
    if (compression || filter) throw Refused("unknown compression or filter method");
    if (!any_idat) throw Refused("no IDAT chunk");
    const size_t stride = size_t(w) * size_t(bpp), need = size_t(h) * (1 + stride);
    std::vector<unsigned char> raw = png_detail::inflate(idat, need);
    if (raw.size() != need) throw Refused("IDAT holds " + std::to_string(raw.size()) + " bytes, the image needs " + std::to_string(need));
    std::vector<unsigned char> px(size_t(h) * stride), zero(stride, 0);
    for (size_t y = 0; y < h; y++) {
      const int f = raw[y * (1 + stride)];
      const unsigned char* line = &raw[y * (1 + stride) + 1];
      unsigned char* cur = &px[y * stride];
      const unsigned char* up = y ? &px[(y - 1) * stride] : zero.data();
      if (f > 4) throw Refused("row " + std::to_string(y) + " has filter type " + std::to_string(f));
      for (size_t i = 0; i < stride; i++) {
        const int a = i >= size_t(bpp) ? cur[i - size_t(bpp)] : 0, b = up[i], c = i >= size_t(bpp) ? up[i - size_t(bpp)] : 0;
        int p = 0;
        if (f == 1) p = a;
        else if (f == 2) p = b;
        else if (f == 3) p = (a + b) >> 1;
        else if (f == 4) {
          const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
          p = pa <= pb && pa <= pc ? a : pb <= pc ? b : c;
        }
        cur[i] = (unsigned char)(line[i] + p);
      }
    }
    if (ctype == 3 && palette.empty()) throw Refused("a palette image without PLTE");
    if (ctype == 3 && have_trns && trns.size() > palette.size() / 3) throw Refused("tRNS is longer than PLTE");
    if (have_trns && ((ctype == 0 && trns.size() != 2) || (ctype == 2 && trns.size() != 6))) throw Refused("bad tRNS length");
    PngImage img;
    img.w = int(w), img.h = int(h), img.channels = channels;
    img.texels.resize(size_t(w) * h * size_t(channels));
    for (size_t i = 0; i < size_t(w) * h; i++) {
      const unsigned char* s = &px[i * size_t(bpp)];
      unsigned char rgba[4] = {s[0], s[0], s[0], 255};
      if (ctype == 3) {
        if (size_t(s[0]) * 3 + 2 >= palette.size()) throw Refused("a palette index past the end of PLTE");
        memcpy(rgba, &palette[size_t(s[0]) * 3], 3);
        if (have_trns && s[0] < trns.size()) rgba[3] = trns[s[0]];
      } else if (ctype == 0) {
        if (have_trns && s[0] == trns[1]) rgba[3] = 0;
      } else if (ctype == 4) {
        rgba[3] = s[1];
      } else {
        memcpy(rgba, s, 3);
        if (ctype == 6) rgba[3] = s[3];
        else if (have_trns && s[0] == trns[1] && s[1] == trns[3] && s[2] == trns[5]) rgba[3] = 0;
      }
      memcpy(&img.texels[i * size_t(channels)], rgba, size_t(channels));
    }
    return img;
  } catch (const Refused& e) {
    throw std::runtime_error("`" + name + "` is no PNG image this reader takes (" + e.what() + ")");
  }
}

inline PngImage read_png(const std::string& path, int channels) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot open `" + path + "`");
  std::vector<unsigned char> data;
  unsigned char buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + n);
  fclose(f);
  return read_png_bytes(data, channels, path);
}

}  // namespace pine
