// pine_amd/csrc/pine_specialize.h -- scene-specialised path kernels (PINE_GPU_FLAG_SPECIALIZE): host side.
//
// With the flag, plan creation compiles path_queue_kernel for the scene at hand:
//  level 1 -- with exactly the scene's feature set instead of the nearest precompiled superset (pine_variants.h);
//  level 2 -- small scenes without meshes: with the scene's BVH as nested straight-line code in pine's visiting order
//             (bvh.cpp:405-446: both child boxes against the tmax of the moment, leaf children in stored order, the child
//             with the larger exit distance second), every box and every primitive record an immediate.  The same device
//             functions do the tests -- same arithmetic, same order, bit-identical films -- but the compiler folds what the
//             constants allow (x * 1, the kind dispatch, the loops) and there is nothing left to load; axis-aligned Rects
//             are tested over their non-zero components only (the one folding the compiler may not do; see below).
//             cbox 12.94 -> 9.87 ms.
// This file: the generator (host code, no GPU needed), and the compile step -- `hipcc --genco` in a child process with the
// device headers next to this library, the code object cached on disk by content; the background compile queue and the
// handle a waiting plan holds on one of its jobs.  All of it plain C++ (the host sanitizer builds compile it with g++).
// The plan's side -- request, look up, load, adopt -- is SceneKernel (pine_scene_kernel.h), which launches the code object
// in place of the precompiled variant.
#pragma once
#include <dirent.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <signal.h>
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cmath>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pine_host.h"

extern char** environ;

namespace pine_gpu {

// What qualifies: measured on MI355X over cbox, the test scenes and seeded random scenes (tools/spec_scenes.py,
// profiles/r03_specialised_scenes.txt): up to 10 primitives the specialised kernel always wins (cbox 8: -19 %, the materials
// scene 10: -24 %, the lights scene 8: -42 %); at 12-13 it wins or loses by scene (-15 % ... +29 %: the unrolled tests keep
// more values live than 128 registers hold), so the line is drawn at 10.  Re-measured with exact feature sets under both
// (profiles/r03_specialised_scenes_cap24.txt, with the line at 24): at 12-13 primitives baked vs feature-set-only
// 0.282 / 0.202, 0.388 / 0.309, 0.367 / 0.355, 0.340 / 0.333, 0.083 / 0.096 ms -- the line stays.
constexpr int kBakedMaxPrimitives = 10;
constexpr unsigned kBakedFeature = 1u << 17;  // F_BAKED for host code that cannot include pine_device.h (pine_scene_kernel.h asserts they agree)

// The generated text (pine_baked_scene.inc), or "" when the scene does not qualify.  `words`: the packed primitive word of
// every entry of A.prims (geometry | emissive | kind), as the generic traversal reports it.
// `top_with_mesh`: the scene has exactly one mesh (C5's class).  Then only the TOP-LEVEL BVH becomes code
// (scene_traverse_baked_top), run once per ray at full lane occupancy, and the flat traversal of the traversal stages is left
// the mesh's BVH alone.  Pine's order survives by construction: the first pass (MODE 0) walks the top level with the mesh
// skipped and notes the state at the mesh's place (reached? tmax and hit so far); the mesh is traversed with that tmax; if
// it is hit and a primitive stored AFTER the mesh had been accepted (or any primitive of the top level is not an axis-aligned
// Rect: kBakedTopPlainRects), the top level is REPLAYED (MODE 1) with the mesh's result put in at its place -- the reference's
// own sequence of tests, same bounds at every box and primitive.
inline std::string generate_baked_scene(const FlatAccel& A, const std::vector<DShape>& shapes, const std::vector<int>& words, bool top_with_mesh = false) {
  if (A.bvhs.size() != (top_with_mesh ? 2u : 1u)) return "";  // (a mesh brings a second BVH)
  const DBvh top = A.bvhs[0];
  // a float as an exact hexadecimal literal, from its bits (printf's %a writes the LOCALE's radix character)
  auto fl = [](float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    const uint32_t e = (u >> 23) & 0xffu, m = (u & 0x7fffffu) << 1;  // 23 mantissa bits as six hexadecimal digits
    if (e == 0xffu) return std::string();                            // NaN / infinity: not baked
    char b[40];
    if (e == 0 && m == 0) snprintf(b, sizeof b, "%s0x0p+0f", (u >> 31) ? "-" : "");
    else snprintf(b, sizeof b, "%s0x%d.%06xp%+df", (u >> 31) ? "-" : "", e ? 1 : 0, unsigned(m), e ? int(e) - 127 : -126);
    return std::string(b);
  };
  std::string out = "// generated by pine_specialize.h for one scene: its BVH and primitive records as immediates\n";
  std::string recs;
  std::vector<char> have(shapes.size(), 0);
  int instances = 0, node_copies = 0;
  int mesh_word = -1, mesh_id = -1;
  std::vector<int> top_words;
  bool ok = true, plain_rects = true;
  auto leaf = [&](int start, int count, const std::string& ind, std::string& o) {
    for (int i = start; i < start + count && ok; i++) {
      const int g = A.prims[size_t(i)];
      if (g < 0 || size_t(g) >= shapes.size()) { ok = false; return; }
      const std::string gs = std::to_string(g), kind = std::to_string(shapes[size_t(g)].kind);
      // (top level only: the code reports SMALL ids -- the primitive's place in this text -- so that two hits and a flag fit
      //  one word of the context on the way from the stage that creates the ray to the one that traverses the mesh;
      //  baked_top_word() maps them back to the packed words the rest of the kernel knows)
      if (top_with_mesh) top_words.push_back(words[size_t(i)]);
      const std::string word = std::to_string(top_with_mesh ? int(top_words.size()) - 1 : words[size_t(i)]);
      if (shapes[size_t(g)].kind == SHAPE_MESH) {
        int bvh;
        memcpy(&bvh, &shapes[size_t(g)].f[2], 4);
        if (!top_with_mesh || mesh_word >= 0 || bvh != 1) { ok = false; return; }  // (one mesh, met once)
        mesh_word = words[size_t(i)];
        mesh_id = int(top_words.size()) - 1;
        o += ind + "{ /* the mesh: traversed by the flat machine */\n";
        // ... unless its first node visit (the mesh BVH's root: both child boxes against the tmax of this moment, exactly what
        // the flat machine does first) already finds nothing to visit: most rays of a room miss the mesh altogether.
        // (C5 96.4 -> 94.6 ms, although the 24 box constants cost the traversal stage 30 spilled VGPRs: 34 against 4)
        std::string gate = "true";
        const DBvh mb = A.bvhs[1];
        const int gate_depth = 1;  // (C5: depth 1 70.0 ms, 2 70.4, 3 72.9, 4 93.4 -- the tests cost more than the rays they turn away)
        if (mb.root_count == 0 && mb.root >= 0 && size_t(mb.root) < A.nodes.size()) {
          // the first `gate_depth` levels of the mesh's BVH against the tmax of this moment (no triangle has been tested, so it is
          // the bound every one of these boxes would meet at the earliest; later bounds are smaller and the box test is monotone
          // in tmax): if no leaf and no node below those levels can be reached, the mesh cannot be hit
          bool finite = true;
          std::function<void(int, int, const std::string&)> gnode = [&](int k, int depth, const std::string& gi) {
            if (k < 0 || size_t(k) >= A.nodes.size()) { finite = false; return; }
            const DNode& gn = A.nodes[size_t(k)];
            std::string b[12];
            for (int j = 0; j < 12; j++) finite = finite && !(b[j] = fl(gn.lo0[j])).empty();
            if (!finite) return;
            o += gi + "{ const float gl0[3] = {" + b[0] + ", " + b[1] + ", " + b[2] + "}, gh0[3] = {" + b[3] + ", " + b[4] + ", " + b[5] + "}, gl1[3] = {" + b[6] + ", " + b[7] + ", " + b[8] +
                 "}, gh1[3] = {" + b[9] + ", " + b[10] + ", " + b[11] + "};\n";
            o += gi + "  float q0 = ray.tmax, q1 = ray.tmax;\n";
            for (int c = 0; c < 2; c++) {
              const std::string cs = std::to_string(c);
              o += gi + "  if (!mesh_reach && box_hit_oct(gl" + cs + ", gh" + cs + ", oct, ray.tmin, q" + cs + ")) {\n";
              if (gn.count[c] > 0 || depth + 1 >= gate_depth) o += gi + "    mesh_reach = true;\n";
              else gnode(gn.child[c], depth + 1, gi + "    ");
              o += gi + "  }\n";
            }
            o += gi + "}\n";
          };
          std::string keep = o;
          o += ind + "  bool mesh_reach = false;\n";
          gnode(mb.root, 0, ind + "  ");
          if (finite) gate = "mesh_reach";
          else o = keep;
        }
        o += ind + "  if (MODE == 0) { if (" + gate + ") { m.reached = true; m.t = ray.tmax; m.geom = hit ? geom_out : -1; } }\n";
        o += ind + "  else if (m.t < ray.tmax) { ray.tmax = m.t; hit = true; geom_out = " + word + "; } }\n";
        if (++instances > kBakedMaxPrimitives) ok = false;
        continue;
      }
      if (shapes[size_t(g)].kind == SHAPE_RECT) {
        // An axis-aligned Rect (normal and both edge directions along coordinate axes -- cbox's walls): rect_test with the
        // products by its zero components dropped.  For the rays of the path kernel (finite origin, unit direction,
        // tmin >= 0) this is the same test with the same t: a dot product with one non-zero factor c_k is a_k * c_k plus
        // signed zeros, which change nothing but the sign of a zero result; a zero denominator fails `denom == 0` either
        // way, a zero numerator gives t = +-0 <= tmin, a zero u / v compares alike; the components of p that are never
        // read are finite (|t d_j| <= |t|) and enter the generic sums as +-0; and whenever t is not finite the t-range
        // test has already failed.  (The compiler may not do this: it must assume NaN and infinite operands.)
        // tests/test_specialize.py compares the two traversals ray by ray on rays built to probe exactly these cases.
        const float* f = shapes[size_t(g)].f;
        auto axis_of = [&](const float* v) {
          int k = -1;
          for (int j = 0; j < 3; j++)
            if (v[j] != 0.0f) k = k == -1 ? j : -2;
          return k;
        };
        const int kn = axis_of(f + 9), ku = axis_of(f + 14), kv = axis_of(f + 17);
        if (kn >= 0 && ku >= 0 && kv >= 0) {
          static const char* const C[3] = {"x", "y", "z"};
          auto times = [&](const std::string& e, float c) { return c == 1.0f ? e : c == -1.0f ? "(-" + e + ")" : "(" + e + " * " + fl(c) + ")"; };
          const std::string cn = C[kn], cu = C[ku], cv = C[kv];
          o += ind + "{ const float denom = " + times("ray.d." + cn, f[9 + kn]) + ";\n";
          o += ind + "  const float num = " + times("(" + fl(f[kn]) + " - ray.o." + cn + ")", f[9 + kn]) + ";\n";
          // The division.  A normal along +-k with the component +-1 (cbox's walls) divides by +-ray.d.k, whose refined
          // reciprocal an ordinary ray's oct.dir_inv.k is (make_oct; negation commutes with every step): t is pdiv_short
          // of it (pine_math.h, "division": the same bits as num / denom inside the window).  The ray's flag bounds the
          // denominator, and with the plane's literal at most kRayHi here it bounds |num| by 2^41 < kDivHi; the floor of
          // |num| (an origin on or within 2^-42 of the plane: zero and tiny numerators) is this site's own compare.
          // Anything else divides plainly, as does a Rect whose normal component is not +-1.
          const bool unit_normal = (f[9 + kn] == 1.0f || f[9 + kn] == -1.0f) && std::fabs(f[kn]) <= kRayHi;
          o += ind + "  bool ok = !(denom == 0.0f);\n" + ind + "  dup_div(num, denom);\n";
          if (unit_normal) {
            o += ind + "  float t = pdiv_short(num, denom, " + times("oct.dir_inv." + cn, f[9 + kn]) + ");\n";
            o += ind + "  if (__builtin_expect(!(ordinary & (pabs(num) >= kDivLo)), 0)) t = num / denom;\n";
          } else {
            o += ind + "  const float t = num / denom;\n";
          }
          o += ind + "  ok = ok & !(t <= ray.tmin || t >= ray.tmax);\n";
          o += ind + "  const float u = " + times("((ray.o." + cu + " + t * ray.d." + cu + ") - " + fl(f[ku]) + ")", f[14 + ku]) + ";\n";
          o += ind + "  ok = ok & !(u < -0.5f || u > 0.5f);\n";
          o += ind + "  const float v = " + times("((ray.o." + cv + " + t * ray.d." + cv + ") - " + fl(f[kv]) + ")", f[17 + kv]) + ";\n";
          o += ind + "  ok = ok & !(v < -0.5f || v > 0.5f);\n";
          o += ind + "  if (ANY) { if (ok) return true; } else if (ok) { ray.tmax = t; hit = true; geom_out = " + word + "; } }\n";
          if (++instances > kBakedMaxPrimitives) ok = false;
          continue;
        }
      }
      plain_rects = false;  // (a primitive that goes through a generic test: see kBakedTopPlainRects below)
      if (!have[size_t(g)]) {
        have[size_t(g)] = 1;
        recs += "__device__ static constexpr float kBakedRec" + std::to_string(g) + "[30] = {";
        for (int k = 0; k < 30; k++) {
          const std::string t = fl(shapes[size_t(g)].f[k]);
          if (t.empty()) { ok = false; return; }
          recs += (k ? ", " : "") + t;
        }
        recs += "};\n";
      }
      o += ind + "{ DShape rec; for (int k = 0; k < 30; k++) rec.f[k] = kBakedRec" + gs + "[k];\n";
      // a transformed box with an ordinary record (the literals are finite; lo <= hi on every axis): the tests over
      // box_slabs_lean (pine_device.h), the same answers for the path kernel's rays from fewer instructions.  An inverted
      // box keeps the generic call.
      const float* bf = shapes[size_t(g)].f;
      if (shapes[size_t(g)].kind == SHAPE_OBB && bf[0] <= bf[3] && bf[1] <= bf[4] && bf[2] <= bf[5])
        o += ind + "  if (ANY) { if (obb_hit<true>(rec.f, ray)) return true; } else if (obb_intersect<true>(rec.f, ray)) { hit = true; geom_out = " + word + "; } }\n";
      else
        o += ind + "  if (ANY) { if (shape_hit<F>(" + kind + ", &rec, ray)) return true; } else if (shape_intersect<F>(" + kind + ", &rec, ray)) { hit = true; geom_out = " + word + "; } }\n";
      if (++instances > kBakedMaxPrimitives) ok = false;
    }
  };
  // one node: returns its text; `depth` bounds the recursion (a node with two inner children appears twice per level)
  std::function<void(int, const std::string&, std::string&, int)> node = [&](int k, const std::string& ind, std::string& o, int depth) {
    if (!ok || k < 0 || size_t(k) >= A.nodes.size() || depth > 8 || ++node_copies > kBakedMaxPrimitives) { ok = false; return; }
    const DNode& nd = A.nodes[size_t(k)];
    std::string b[12];
    const float* f = nd.lo0;  // lo0[3] hi0[3] lo1[3] hi1[3] are contiguous
    for (int j = 0; j < 12; j++) {
      b[j] = fl(f[j]);
      if (b[j].empty()) { ok = false; return; }
    }
    o += ind + "{ const float lo0[3] = {" + b[0] + ", " + b[1] + ", " + b[2] + "}, hi0[3] = {" + b[3] + ", " + b[4] + ", " + b[5] + "}, lo1[3] = {" + b[6] + ", " + b[7] + ", " + b[8] +
         "}, hi1[3] = {" + b[9] + ", " + b[10] + ", " + b[11] + "};\n";
    o += ind + "  float t0 = ray.tmax, t1 = ray.tmax; bool in0 = false, in1 = false; (void)in0; (void)in1;\n";
    for (int c = 0; c < 2; c++) {
      const std::string cs = std::to_string(c);
      o += ind + "  if (box_hit_oct(lo" + cs + ", hi" + cs + ", oct, ray.tmin, t" + cs + ")) {\n";
      if (nd.count[c] > 0) leaf(nd.child[c], nd.count[c], ind + "    ", o);
      else o += ind + "    in" + cs + " = true;\n";
      o += ind + "  }\n";
    }
    const bool i0 = nd.count[0] == 0, i1 = nd.count[1] == 0;
    if (i0 && i1) {
      // both children are inner nodes: the one with the larger exit distance is visited second (pushed, bvh.cpp:431-440).
      // Two passes over one copy of each subtree's code (a copy per order would double the text at every such node).
      o += ind + "  { const bool swap01 = in0 && in1 && t0 > t1;\n";
      o += ind + "    _Pragma(\"nounroll\") for (int pass = 0; pass < 2; pass++) {\n";
      o += ind + "      if (in0 && (pass == 1) == swap01) {\n";
      node(nd.child[0], ind + "        ", o, depth + 1);
      o += ind + "      }\n";
      o += ind + "      if (in1 && (pass == 0) == swap01) {\n";
      node(nd.child[1], ind + "        ", o, depth + 1);
      o += ind + "      }\n";
      o += ind + "    } }\n";
    } else if (i0) {
      o += ind + "  if (in0) {\n";
      node(nd.child[0], ind + "    ", o, depth + 1);
      o += ind + "  }\n";
    } else if (i1) {
      o += ind + "  if (in1) {\n";
      node(nd.child[1], ind + "    ", o, depth + 1);
      o += ind + "  }\n";
    }
    o += ind + "}\n";
  };
  std::string body;
  if (top.root_count > 0) leaf(top.root_start, top.root_count, "  ", body);  // the root itself is a leaf (bvh.cpp:331-334)
  else if (top.root >= 0) node(top.root, "  ", body, 0);
  if (!ok || (top_with_mesh && mesh_word < 0)) return "";
  out += recs;
  if (top_with_mesh) {
    out = "#define PINE_BAKED_TOP 1\n" + out;
    out += "struct BakedMesh { bool reached; float t; int geom; };  // at the mesh's place: MODE 0 out (tmax and hit so far), MODE 1 in (t = the mesh's hit)\n";
    out += "constexpr int kBakedMeshWord = " + std::to_string(mesh_word) + ", kBakedMeshId = " + std::to_string(mesh_id) + ";\n";
    // Every primitive beside the mesh is an inline axis-aligned Rect (C5's class): its t does not depend on the bound it is tested
    // with and it is accepted exactly when t < tmax, which is what lets a triangle stand without a replay (pine_queue_kernel.h).
    // Any other primitive -- a scaled Box(AABB, mat4) reports min(exit, tmax) in LOCAL units for a ray that starts inside it, a
    // smaller t under a smaller bound -- and every triangle hit is settled by the replay.
    out += std::string("constexpr bool kBakedTopPlainRects = ") + (plain_rects ? "true" : "false") + ";\n";
    out += "__device__ __forceinline__ int baked_top_word(int id) {\n  switch (id) {\n";
    for (size_t k = 0; k < top_words.size(); k++) out += "    case " + std::to_string(k) + ": return " + std::to_string(top_words[k]) + ";\n";
    out += "    default: return -1;\n  }\n}\n";
    if (top_words.size() > 14) return "";  // (ids travel in four bits, 0 = none)
    out += "template <bool ANY, unsigned F, int MODE>\n__device__ __forceinline__ bool scene_traverse_baked_top(DRay& ray, int& geom_out, BakedMesh& m) {\n";
  } else {
    out += "template <bool ANY, unsigned F>\n__device__ __forceinline__ bool scene_traverse_baked(DRay& ray, int& geom_out) {\n";
  }
  // (one range test of the ray answers for every division below: ray_ordinary, pine_device.h)
  out += "  const bool ordinary = ray_ordinary(ray);\n  const DRayOct oct = make_oct(ray, ordinary);\n  bool hit = false;\n  (void)oct;\n";
  out += body;
  out += "  return hit;\n}\n";
  return out;
}

// Which baked form a scene gets under a kernel with (`stages`) or without traversal stages, and its text: the WHOLE scene when
// it has no mesh and the kernel traverses inside its stages; the TOP level when it has exactly one mesh and traversal is a
// stage of its own (C5's class), the mesh left to the flat traversal; otherwise -- or when the generator declines -- none.
enum class BakedForm { kNone, kWhole, kTop };
struct BakedScene { std::string text; BakedForm form = BakedForm::kNone; };
inline BakedScene bake_scene(const FlatAccel& A, const std::vector<DShape>& shapes, const std::vector<int>& words, bool stages) {
  BakedScene b;
  if (!stages && A.top_prim_begin == 0) b.text = generate_baked_scene(A, shapes, words), b.form = BakedForm::kWhole;
  else if (stages && A.bvhs.size() == 2) b.text = generate_baked_scene(A, shapes, words, true), b.form = BakedForm::kTop;
  if (b.text.empty()) b.form = BakedForm::kNone;
  return b;
}

// pine_amd/ as seen from this library ($PINE_GPU_SOURCE_DIR overrides): csrc/ and ../include/ hold the device headers
inline std::string library_dir() {
  if (const char* e = getenv("PINE_GPU_SOURCE_DIR")) return std::string(e) + "/lib";
  Dl_info info;
  if (dladdr(reinterpret_cast<const void*>(&library_dir), &info) && info.dli_fname) {
    const std::string lib = info.dli_fname;
    const size_t slash = lib.rfind('/');
    return slash == std::string::npos ? std::string(".") : lib.substr(0, slash);
  }
  return ".";
}

// ---- compile: hipcc --genco in a child process, cached by content ----------------------------------------------------
inline bool read_file(const std::string& path, std::string& out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  char buf[65536];
  size_t n;
  out.clear();
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
  fclose(f);
  return true;
}
inline bool write_file(const std::string& path, const std::string& text) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  return fclose(f) == 0 && ok;
}
// A cached code object is handed to the runtime only if it is whole: a clang offload bundle whose entries lie inside the file,
// the device entry an ELF64 whose section table does too (a file cut short by a full disk must not reach a loader that
// trusts its offsets).  Other containers (a compressed bundle, a bare ELF) are left to the runtime's own checks.
inline bool code_object_is_whole(const std::string& image) {
  static const char kMagic[] = "__CLANG_OFFLOAD_BUNDLE__";
  const size_t n = image.size();
  if (n < 32 || memcmp(image.data(), kMagic, 24) != 0) return n >= 64;
  auto u64 = [&](size_t at) {
    uint64_t v;
    memcpy(&v, image.data() + at, 8);
    return v;
  };
  const uint64_t entries = u64(24);
  if (entries == 0 || entries > 64) return false;
  size_t at = 32;
  bool device = false;
  for (uint64_t i = 0; i < entries; i++) {
    if (at + 24 > n) return false;
    const uint64_t off = u64(at), size = u64(at + 8), idlen = u64(at + 16);
    at += 24;
    if (idlen > 4096 || at + idlen > n || off > n || size > n - off) return false;
    at += size_t(idlen);
    if (size == 0) continue;
    if (size < 64 || memcmp(image.data() + off, "\x7f" "ELF", 4) != 0) return false;
    const uint64_t shoff = u64(size_t(off) + 0x28);
    uint16_t shentsize, shnum;
    memcpy(&shentsize, image.data() + off + 0x3a, 2);
    memcpy(&shnum, image.data() + off + 0x3c, 2);
    if (shoff > size || uint64_t(shentsize) * shnum > size - shoff) return false;
    device = true;
  }
  return device;
}
inline unsigned long long fnv1a(const std::string& s, unsigned long long h = 1469598103934665603ull) {
  for (unsigned char c : s) h = (h ^ c) * 1099511628211ull;
  return h;
}
// The scene's kernel is exported from its translation unit under a plain C name (the generated text wraps
// path_queue_kernel<features, ctx> in an extern "C" __global__ function of the same arguments): nothing here depends on how
// the compiler mangles HIP's vector types.  The name carries the feature bits (F_BAKED among them) and the context count, so
// a profile tells the scene's kernel from the precompiled path_queue_kernel<...> and one scene's kernel from another's.
inline std::string kernel_symbol(unsigned features, int ctx) { return "pine_scene_kernel_" + std::to_string(features) + "_" + std::to_string(ctx); }

// sizeof / offsetof fingerprints of what the host half of this library and a run-time compiled kernel must agree on (kernel
// argument layout, counters, LDS layout constants).  The generated translation unit static_asserts them against the headers
// it is compiled from: headers next to the library that are not the ones it was built from (an edited tree without a rebuilt
// .so, a library built with -DPINE_PROFILE_SECTIONS while the run-time compile lacks the flag) fail the compile with that
// message instead of producing a kernel with another argument or LDS layout.
struct AbiFingerprint {
  size_t device_scene, work_params, counters, dnode, dshape, dmaterial, dlight, work_params_total_items, device_scene_cam, device_scene_off_frames;
  int qfields, qwin, qctl_words, token_dwords, trav_record_dwords, ctx_plain, ctx_sss;
};
AbiFingerprint abi_fingerprint();  // (pine_kernels.hip: evaluated by the library's own compile)
inline std::string abi_fingerprint_asserts(const AbiFingerprint& f) {
  char buf[1500];
  snprintf(buf, sizeof buf,
           "static_assert(sizeof(pine_gpu::DeviceScene) == %zu && sizeof(pine_gpu::WorkParams) == %zu && sizeof(pine_gpu::Counters) == %zu && "
           "sizeof(pine_gpu::DNode) == %zu && sizeof(pine_gpu::DShape) == %zu && sizeof(pine_gpu::DMaterial) == %zu && sizeof(pine_gpu::DLight) == %zu && "
           "offsetof(pine_gpu::WorkParams, total_items) == %zu && offsetof(pine_gpu::DeviceScene, cam) == %zu && "
           "offsetof(pine_gpu::DeviceScene, off_frames) == %zu && "
           "pine_gpu::kQFields == %d && pine_gpu::kQWinDwords == %d && pine_gpu::QC_WORDS == %d && pine_gpu::kQTokenDwords == %d && "
           "pine_gpu::kTravRecordDwords == %d && pine_gpu::kQCtxGlobalDwordsPlain == %d && pine_gpu::kQCtxGlobalDwordsSss == %d,\n"
           "              \"the device headers this kernel is compiled from are not the ones libpine_gpu.so was built from (rebuild the library, or point $PINE_GPU_SOURCE_DIR at its own sources)\");\n",
           f.device_scene, f.work_params, f.counters, f.dnode, f.dshape, f.dmaterial, f.dlight, f.work_params_total_items, f.device_scene_cam, f.device_scene_off_frames, f.qfields, f.qwin,
           f.qctl_words, f.token_dwords, f.trav_record_dwords, f.ctx_plain, f.ctx_sss);
  return buf;
}

// A directory this process may keep code objects in: created 0700 if missing; accepted only if it is a real directory (not
// a symlink) that belongs to this user and that nobody else can write to -- a code object found in it is loaded and
// launched, so another local user must not be able to plant one (the predictable /tmp fallback name is why this matters).
inline bool private_cache_dir(const std::string& d) {
  for (size_t i = 1; i <= d.size(); i++)
    if (i == d.size() || d[i] == '/') mkdir(d.substr(0, i).c_str(), 0700);
  struct stat st;
  if (lstat(d.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return false;
  if (st.st_uid != geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH)) != 0) return false;
  return access(d.c_str(), W_OK) == 0;
}

// The environment a compiler child gets: the caller's, minus everything that would make the child a profiled / tool-loaded
// process.  Under rocprofv3 this process carries LD_PRELOAD and the ROCP_* / ROCPROFILER_* / HSA_TOOLS_* variables of the
// profiler's tool library; inherited, they would initialise the GPU runtime inside hipcc before it execs clang (a pattern the
// GPU pool forbids) and put the compiler's processes into the trace.
inline std::vector<std::string> scrubbed_environment() {
  static const char* const kDrop[] = {"LD_PRELOAD=", "ROCP_", "ROCPROFILER_", "HSA_TOOLS_", "ROCTRACER_", "ROCPROF_", "RPD_", "OMNITRACE_", "ROCPROFSYS_"};
  std::vector<std::string> out;
  for (char** e = environ; e && *e; e++) {
    bool drop = false;
    for (const char* p : kDrop)
      if (strncmp(*e, p, strlen(p)) == 0) drop = true;
    if (!drop) out.emplace_back(*e);
  }
  return out;
}

// What to compile, and where its code object lives.
struct KernelRequest {
  std::string baked;  // the scene as code (generate_baked_scene), or "" for the generic traversal with the scene's exact feature set
  unsigned features = 0;
  int ctx = 0;
  std::string arch;
  // filled by kernel_cache_lookup:
  std::string key, csrc_dir, include_dir, cache_dir, path;
  std::vector<std::string> extra;  // $PINE_GPU_SPECIALIZE_EXTRA
  bool packaged = false;           // found in the package's own kernel_cache/ (read-only installs ship kernels there)
};
static const char* const kSpecHeaders[] = {"pine_types.h", "pine_math.h", "pine_libm.h", "pine_atmosphere.h", "pine_image_node.h", "pine_rng.h", "pine_noise.h", "pine_device.h", "pine_trav.h", "pine_kernels_device.h", "pine_traverse.h", "pine_radiance.h", "pine_queue_kernel.h"};
static const char* const kSpecFlags[] = {"-O3", "-std=c++17", "-fno-slp-vectorize", "-ffp-contract=off", "-w"};  // = the Makefile's CXXFLAGS

// Computes the request's content key (the generated text, the device headers, the flags, the architecture, <features, ctx>)
// and looks for its code object: the package's kernel_cache/ first (unless $PINE_GPU_CACHE_DIR is set or `skip_packaged`),
// then the user's cache directory.  Returns 1 = R.path exists, 0 = not cached (R.path / R.cache_dir say where it goes),
// -1 = cannot even look (headers missing, no private cache directory) with the reason in `err`.
inline int kernel_cache_lookup(KernelRequest& R, std::string& err, bool skip_packaged = false) {
  const std::string dir = library_dir() + "/..";
  R.csrc_dir = dir + "/csrc", R.include_dir = dir + "/../include";  // (library_dir() honours $PINE_GPU_SOURCE_DIR)
  unsigned long long h = fnv1a(R.baked);
  for (const char* name : kSpecHeaders) {
    std::string text;
    if (!read_file(R.csrc_dir + "/" + name, text)) {
      err = "scene specialisation needs the device headers next to the library: cannot read " + R.csrc_dir + "/" + name + " ($PINE_GPU_SOURCE_DIR overrides)";
      return -1;
    }
    h = fnv1a(text, h);
  }
  for (const char* f : kSpecFlags) h = fnv1a(f, h);
  R.extra.clear();  // $PINE_GPU_SPECIALIZE_EXTRA: more compiler flags, space-separated (diagnostic builds: -DPINE_PROFILE_SECTIONS)
  if (const char* e = getenv("PINE_GPU_SPECIALIZE_EXTRA")) {
    std::string cur;
    for (const char* c = e;; c++) {
      if (*c == ' ' || *c == '\0') {
        if (!cur.empty()) R.extra.push_back(cur);
        cur.clear();
        if (*c == '\0') break;
      } else cur += *c;
    }
  }
  for (const std::string& f : R.extra) h = fnv1a(f, h);
  h = fnv1a(abi_fingerprint_asserts(abi_fingerprint()), h);
  h = fnv1a(R.arch + "/" + std::to_string(R.features) + "/" + std::to_string(R.ctx) + "/v2", h);
  char key[32];
  snprintf(key, sizeof key, "%016llx", h);
  R.key = key;
  struct stat st;
  R.packaged = false;
  if (getenv("PINE_GPU_CACHE_DIR") == nullptr && !skip_packaged) {
    // kernels built ahead of time may travel with the package (pine_amd/lib/kernel_cache/): same key, so a stale one is
    // simply never found
    R.path = library_dir() + "/kernel_cache/scene_" + R.key + ".co";
    if (stat(R.path.c_str(), &st) == 0 && st.st_size > 0) {
      R.packaged = true;
      return 1;
    }
  }
  std::string cache;
  if (const char* e = getenv("PINE_GPU_CACHE_DIR")) cache = e;
  else if (const char* x = getenv("XDG_CACHE_HOME")) cache = std::string(x) + "/pine_gpu";
  else if (const char* home = getenv("HOME")) cache = std::string(home) + "/.cache/pine_gpu";
  else cache = "/tmp/pine_gpu_cache_" + std::to_string(unsigned(geteuid()));
  if (!private_cache_dir(cache)) {
    cache = "/tmp/pine_gpu_cache_" + std::to_string(unsigned(geteuid()));
    if (!private_cache_dir(cache)) {
      // (somebody else owns the predictable name, or it is writable by others: a directory of our own)
      std::string tmpl = "/tmp/pine_gpu_cache_" + std::to_string(unsigned(geteuid())) + "_XXXXXX";
      static std::string made;  // one per process
      static std::mutex made_mutex;
      std::lock_guard<std::mutex> lock(made_mutex);
      if (made.empty() && mkdtemp(&tmpl[0])) made = tmpl;
      if (made.empty()) {
        err = "scene specialisation: no private writable cache directory (" + cache + "; $PINE_GPU_CACHE_DIR overrides)";
        return -1;
      }
      cache = made;
    }
  }
  R.cache_dir = cache;
  R.path = cache + "/scene_" + R.key + ".co";
  return stat(R.path.c_str(), &st) == 0 && st.st_size > 0 ? 1 : 0;
}

// Runs the compiler for a request kernel_cache_lookup has keyed (R.path does not exist): `hipcc --genco` in a CHILD process
// (posix_spawn: never an exec of this, GPU-initialised, process) with a scrubbed environment, its output into a log file; an
// atomic rename publishes the finished code object.  `child` (optional) holds the compiler's pid while it runs, so that a
// shutting-down process can end it.  On failure returns false with the reason in `err`.
inline bool kernel_compile(const KernelRequest& R, std::string& err, std::atomic<int>* child = nullptr) {
  struct stat st;
  // a private build directory: the generated include, the one-line translation unit, the compiler's output
  std::string work = R.cache_dir + "/build_" + R.key + "_" + std::to_string(int(getpid())) + "_XXXXXX";
  if (!mkdtemp(&work[0])) {
    err = "scene specialisation: mkdtemp failed in " + R.cache_dir;
    return false;
  }
  const std::string inc = work + "/pine_baked_scene.inc", src = work + "/scene.hip", obj = work + "/scene.co", log = work + "/hipcc.log";
  const std::string targs = std::to_string(R.features) + "u, " + std::to_string(R.ctx);
  std::string tu = std::string(R.baked.empty() ? "" : "#define PINE_BAKED_SCENE 1\n") + "#include <hip/hip_runtime.h>\n#include <math.h>\n#include <stddef.h>\n#include <stdint.h>\n#include <string.h>\n#include <type_traits>\n"
                   "#include \"pine_kernels_device.h\"\n" + abi_fingerprint_asserts(abi_fingerprint()) +
                   "extern \"C\" __global__ void __launch_bounds__(pine_gpu::kQBlock, pine_gpu::kQBlock / 256) " + kernel_symbol(R.features, R.ctx) +
                   "(pine_gpu::DeviceScene S, pine_gpu::WorkParams W, const ulonglong2* __restrict__ ckpt, float4* __restrict__ samples, float* __restrict__ fold, "
                   "uint32_t* __restrict__ ctxg, pine_gpu::Counters* __restrict__ counters) {\n"
                   "  pine_gpu::path_queue_body<" + targs + ">(S, W, ckpt, samples, fold, ctxg, counters);\n}\n";
  if (!R.baked.empty())
    // test hook (pine_gpu_plan_test_traverse_baked): the baked traversal on caller-given rays -- per ray: hit, geometry, tmax
    // bits of the closest-hit query, result of the any-hit query
    tu += "#ifndef PINE_BAKED_TOP\nextern \"C\" __global__ void __launch_bounds__(64) pine_baked_traverse_test(const float* rays, long long nrays, unsigned* out) {\n"
          "  using namespace pine_gpu;\n  const long long i = blockIdx.x * 64ll + threadIdx.x;\n  if (i >= nrays) return;\n  const float* q = rays + i * 8;\n"
          "  DRay ray{f3{q[0], q[1], q[2]}, f3{q[3], q[4], q[5]}, q[6], q[7]};\n  int geom = 0;\n"
          "  const bool hit = scene_traverse_baked<false, " + std::to_string(R.features) + "u>(ray, geom);\n"
          "  out[i * 4] = hit ? 1u : 0u;\n  out[i * 4 + 1] = hit ? unsigned(geom & kPrimIndexMask) : 0u;\n  out[i * 4 + 2] = __float_as_uint(ray.tmax);\n"
          "  DRay r2{f3{q[0], q[1], q[2]}, f3{q[3], q[4], q[5]}, q[6], q[7]};\n  int g2 = 0;\n"
          "  out[i * 4 + 3] = scene_traverse_baked<true, " + std::to_string(R.features) + "u>(r2, g2) ? 1u : 0u;\n}\n#endif\n";
  auto cleanup = [&]() {
    for (const std::string& f : {inc, src, obj, log}) unlink(f.c_str());
    rmdir(work.c_str());
  };
  if ((!R.baked.empty() && !write_file(inc, R.baked)) || !write_file(src, tu)) {
    err = "scene specialisation: cannot write into " + work;
    cleanup();
    return false;
  }
  std::string hipcc;
  if (const char* e = getenv("PINE_GPU_HIPCC")) hipcc = e;
  else {
    const std::string rocm = getenv("ROCM_PATH") ? getenv("ROCM_PATH") : "/opt/rocm";
    hipcc = rocm + "/bin/hipcc";
    if (access(hipcc.c_str(), X_OK) != 0) hipcc = "hipcc";  // on $PATH
  }
  std::vector<std::string> args = {hipcc, "--genco", "--offload-arch=" + R.arch};
  for (const char* f : kSpecFlags) args.push_back(f);
  for (const std::string& f : R.extra) args.push_back(f);
  for (const std::string& a : {"-I" + work, "-I" + R.csrc_dir, "-I" + R.include_dir, src, std::string("-o"), obj}) args.push_back(a);
  std::vector<char*> argv;
  for (auto& a : args) argv.push_back(&a[0]);
  argv.push_back(nullptr);
  std::vector<std::string> env = scrubbed_environment();
  std::vector<char*> envp;
  for (auto& e : env) envp.push_back(&e[0]);
  envp.push_back(nullptr);
  posix_spawn_file_actions_t fa;
  posix_spawn_file_actions_init(&fa);
  posix_spawn_file_actions_addopen(&fa, 1, log.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
  posix_spawn_file_actions_adddup2(&fa, 1, 2);
  posix_spawn_file_actions_addopen(&fa, 0, "/dev/null", O_RDONLY, 0);
  posix_spawnattr_t at;
  posix_spawnattr_init(&at);
  posix_spawnattr_setpgroup(&at, 0);  // (its own process group: ending the compiler ends clang and lld with it)
  posix_spawnattr_setflags(&at, POSIX_SPAWN_SETPGROUP);
  pid_t pid = 0;
  const int rc = posix_spawnp(&pid, hipcc.c_str(), &fa, &at, argv.data(), envp.data());
  posix_spawn_file_actions_destroy(&fa);
  posix_spawnattr_destroy(&at);
  if (rc != 0) {
    err = "scene specialisation: cannot start " + hipcc + " (" + strerror(rc) + "; $PINE_GPU_HIPCC overrides)";
    cleanup();
    return false;
  }
  if (child) child->store(int(pid));
  int status = 0;
  while (waitpid(pid, &status, 0) < 0 && errno == EINTR) {
  }
  if (child) child->store(0);
  if (!WIFEXITED(status) || WEXITSTATUS(status) != 0 || stat(obj.c_str(), &st) != 0 || st.st_size == 0) {
    std::string text, first;
    read_file(log, text);
    // the compiler's first diagnostics (what went wrong) before the tail of its output (the command line it echoes last)
    for (size_t at = 0, n = 0; n < 4 && (at = text.find("error:", at)) != std::string::npos; n++) {
      const size_t b = text.rfind('\n', at), e = text.find('\n', at);
      first += text.substr(b == std::string::npos ? 0 : b + 1, (e == std::string::npos ? text.size() : e) - (b == std::string::npos ? 0 : b + 1)) + "\n";
      at = e == std::string::npos ? text.size() : e;
    }
    if (first.size() > 1200) first.resize(1200);
    if (text.size() > 800) text = text.substr(text.size() - 800);
    err = "scene specialisation: " + hipcc + (WIFSIGNALED(status) ? " was ended by a signal: " : " failed: ") + first + text;
    cleanup();
    return false;
  }
  if (rename(obj.c_str(), R.path.c_str()) != 0) {  // (atomic: a concurrent process compiling the same scene wins or loses whole)
    err = "scene specialisation: cannot move the code object into " + R.cache_dir;
    cleanup();
    return false;
  }
  cleanup();
  return true;
}

// the state of a background build (SpecJob::state)
enum : int { kSpecBuilding = 0, kSpecBuilt, kSpecFailed };

// The background compile queue.  A job is one code object (content key); plans hold a SpecWaiter and poll `state`.  Workers
// are started on demand, run jobs in order, skip jobs nobody waits for any more, and exit when the queue is empty.  The
// singleton is never destroyed (worker threads may outlive static destruction); at process exit an atexit handler raises
// `closing`, ends running compilers (their own process groups) and joins the workers, so nothing of ours runs while the
// runtime goes down and no half-written build directory is left behind.
struct SpecJob {
  KernelRequest req;
  std::atomic<int> state{kSpecBuilding};
  std::atomic<int> waiters{0};
  std::string error;  // (written before `state` becomes kSpecFailed)
};
// One waiter's share of a job: a move-only handle.  SpecQueue::submit counts the waiter (under the queue's lock) and hands it
// out; the handle's end -- reset(), destruction, being assigned over -- is the only place that gives the count back, once (a
// moved-from or empty handle holds nothing).  A job whose count is zero when a worker reaches it is dropped from the queue; a
// running build goes on for the next plan of the geometry.
struct SpecWaiterRelease {
  std::shared_ptr<SpecJob> keep;  // (the job lives as long as a waiter points at it)
  void operator()(SpecJob* job) { job->waiters.fetch_sub(1), keep.reset(); }
};
using SpecWaiter = std::unique_ptr<SpecJob, SpecWaiterRelease>;
struct SpecQueue {
  static constexpr int kSpecWorkers = 2, kMaxPending = 6;
  std::mutex mu;
  std::map<std::string, std::shared_ptr<SpecJob>> jobs;  // by key: every job ever started in this process
  std::deque<std::shared_ptr<SpecJob>> pending;
  std::vector<std::thread> workers;
  bool busy[kSpecWorkers] = {};  // a worker runs in this slot (its compiler's pid: children[slot])
  std::atomic<int> children[kSpecWorkers];
  std::atomic<bool> closing{false};
  static SpecQueue& get() {
    static SpecQueue* q = [] {
      SpecQueue* x = new SpecQueue();
      for (auto& c : x->children) c.store(0);
      atexit([] { SpecQueue::get().shutdown(); });
      return x;
    }();
    return *q;
  }
  // the job for `req` (already keyed), with the caller counted among its waiters: an existing one, or a new one queued for a
  // worker; an empty handle, nothing counted, when the queue is full or closing
  // (`retry_failed`: a kernel whose build failed earlier in this process is tried again -- the caller asked for it by flag;
  //  the automatic mode does not spend a compiler run per plan on a kernel that does not build)
  SpecWaiter submit(const KernelRequest& req, bool retry_failed) {
    std::lock_guard<std::mutex> lock(mu);
    if (closing.load()) return SpecWaiter();
    auto it = jobs.find(req.key);
    if (it != jobs.end() && (it->second->state.load() != kSpecFailed || !retry_failed)) {
      it->second->waiters.fetch_add(1);  // (under the lock: a worker cannot cancel the job before the caller counts)
      return SpecWaiter(it->second.get(), SpecWaiterRelease{it->second});
    }
    if (int(pending.size()) >= kMaxPending) return SpecWaiter();
    auto job = std::make_shared<SpecJob>();
    job->req = req;
    job->waiters.store(1);
    jobs[req.key] = job;
    pending.push_back(job);
    for (int slot = 0; slot < kSpecWorkers; slot++)
      if (!busy[slot]) {
        busy[slot] = true;
        workers.emplace_back([this, slot] { work(slot); });
        break;
      }
    return SpecWaiter(job.get(), SpecWaiterRelease{job});
  }
  void work(int slot) {
    for (;;) {
      std::shared_ptr<SpecJob> job;
      {
        std::lock_guard<std::mutex> lock(mu);
        while (!pending.empty() && !job) {
          job = pending.front();
          pending.pop_front();
          if (job->waiters.load() == 0 || closing.load()) {  // nobody wants it any more
            job->error = "cancelled";
            job->state.store(kSpecFailed);
            jobs.erase(job->req.key);
            job.reset();
          }
        }
        if (!job) {
          busy[slot] = false;
          return;
        }
      }
      std::string err;
      struct stat st;
      const bool ok = (stat(job->req.path.c_str(), &st) == 0 && st.st_size > 0) || kernel_compile(job->req, err, &children[slot]);
      job->error = err;
      job->req.baked.clear();  // (the text is no longer needed: waiting plans keep their own copy)
      job->req.baked.shrink_to_fit();
      job->state.store(ok ? kSpecBuilt : kSpecFailed);
      if (ok) {  // later plans find the code object on disk; only failures are remembered
        std::lock_guard<std::mutex> lock(mu);
        jobs.erase(job->req.key);
      }
    }
  }
  void shutdown() {
    closing.store(true);
    for (auto& c : children) {
      const int pid = c.load();
      if (pid > 0) kill(-pid, SIGKILL);  // the compiler's process group
    }
    std::vector<std::thread> w;
    {
      std::lock_guard<std::mutex> lock(mu);
      w.swap(workers);
    }
    for (auto& t : w)
      if (t.joinable()) t.join();
  }
};

}  // namespace pine_gpu
