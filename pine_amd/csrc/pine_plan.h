// pine_amd/csrc/pine_plan.h -- what the host side of the two kernel translation units shares: the plan record
// (struct pine_gpu_plan), HIP_OK, the sampler-table loader, the device memory pool and need_device.  Included by
// pine_kernels.hip (plans, launches) and pine_test_hooks.hip (the device unit-test hooks).
// Device memory, pinned memory, events and streams are held by the owners of pine_device_buffer.h: a plan owns what its members
// hold and gives it back when it is deleted, a hook or a builder when it returns.  DeviceScene / WorkParams keep raw views.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include <dlfcn.h>

#include "../../include/pine_gpu.h"
#include "pine_host.h"
#include "pine_variants.h"

struct pine_gpu_scene;
namespace pine_gpu {
SceneHost& scene_host(pine_gpu_scene* s);
}  // namespace pine_gpu
#include "pine_kernels_device.h"
#include "pine_ao_kernel.h"
#include "pine_guides_kernel.h"
#include "pine_accel_kernel.h"
#include "pine_shade_kernel.h"
namespace pine_gpu {

#define HIP_OK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                           \
      (void)hipGetLastError(); /* reported here: do not leave it sticky for the caller's next HIP user */ \
      return -1;                                                                              \
    }                                                                                         \
  } while (0)

inline std::string g_table_path;  // (inline: one loader state for every translation unit)
// The packed tables are immutable once read; users take a shared snapshot, so a concurrent
// pine_gpu_set_table_path (which only drops the library's own reference) cannot free them under a reader.
using TableBlob = std::shared_ptr<const std::vector<uint8_t>>;
inline TableBlob g_tables;
inline std::mutex g_table_mutex;

inline int load_tables(TableBlob& out) {
  std::lock_guard<std::mutex> lock(g_table_mutex);
  if (g_tables) {
    out = g_tables;
    return 0;
  }
  if (g_table_path.empty()) {
    // not set by the host: $PINE_GPU_TABLES, else data/bluesobol_u8.bin next to the directory this library sits in
    // (pine_amd/lib/libpine_gpu.so -> pine_amd/data/), wherever the process was started from
    if (const char* env = getenv("PINE_GPU_TABLES")) g_table_path = env;
    else {
      Dl_info info;
      if (dladdr(reinterpret_cast<const void*>(&load_tables), &info) && info.dli_fname) {
        std::string lib = info.dli_fname;
        const size_t slash = lib.rfind('/');
        g_table_path = (slash == std::string::npos ? std::string(".") : lib.substr(0, slash)) + "/../data/bluesobol_u8.bin";
      }
    }
  }
  if (g_table_path.empty()) {
    set_error("BlueSobol table path not set (pine_gpu_set_table_path)");
    return -1;
  }
  FILE* f = fopen(g_table_path.c_str(), "rb");
  if (!f) {
    set_error("cannot open " + g_table_path);
    return -1;
  }
  std::vector<uint8_t> buf(65536 + 9 * 262144);
  size_t n = fread(buf.data(), 1, buf.size(), f);
  fclose(f);
  if (n != buf.size()) {
    set_error("short read of " + g_table_path);
    return -1;
  }
  g_tables = std::make_shared<const std::vector<uint8_t>>(std::move(buf));
  out = g_tables;
  return 0;
}
// The device keeps sobol_256spp_256d transposed ([dimension][sample] instead of [sample][dimension]):
// lanes of a wave usually ask for the same dimension at 64 different (ranked) sample rows, which is
// one 256-byte row here instead of 64 cache lines 256 bytes apart.
static std::vector<uint8_t> transposed_sobol(const std::vector<uint8_t>& tables) {
  std::vector<uint8_t> t(65536);
  for (int s = 0; s < 256; s++)
    for (int d = 0; d < 256; d++) t[d * 256 + s] = tables[s * 256 + d];
  return t;
}
static int effective_spp(int spp) {  // BlueSobolSampler ctor sampler.cpp:115-121
  if (spp > 256) spp = 256;
  if (spp <= 0) return 0;
  int x = spp - 1;
  for (unsigned i = 1; i < 32; i <<= 1) x |= x >> i;
  return x + 1;
}

// Device memory of plans comes from a process-wide pool: hipMalloc / hipFree of the big per-plan buffers (the per-sample
// radiance buffer is 1.7 GB for a 640 x 640 x 256 render, 6.8 GB for 1920 x 1080) cost 30 - 90 ms per plan, which is most of
// what a ONE-SHOT render (pine_gpu_path_render: create, launch, destroy -- what PathIntegrator::render does) spends outside
// its kernels.  A destroyed plan's blocks of 256 KB and more go to a per-device free list instead and the next plan takes
// the smallest one that fits within 25 %; at most $PINE_GPU_POOL_MB (default 16 384; 0: no pool) are kept,
// pine_gpu_release_cached_memory() frees them.  No kernel reads a buffer before writing it (hipMalloc does not clear either):
// DESIGN.md 4.3.1 lists every block with its first writer and first reader, and tests/test_poisoned_memory.py runs every kernel
// family on blocks that PINE_GPU_TEST_POISON (pine_device_buffer.h) has filled with a word no kernel wrote.
inline thread_local size_t g_alloc_tally = 0;  // bytes asked of DevicePool::alloc by this thread (plan_build: pine_gpu_plan_device_bytes)
struct DevicePool {
  struct Block {
    void* p;
    size_t bytes;
    int device;
  };
  std::mutex mu;
  std::vector<Block> free_blocks;
  std::map<void*, Block> live;  // pooled-size allocations handed out
  size_t pooled = 0, cap = size_t(16384) << 20;
  DevicePool() {
    if (const char* e = getenv("PINE_GPU_POOL_MB")) cap = size_t(atoll(e) > 0 ? atoll(e) : 0) << 20;
  }
  static DevicePool& get() {
    static DevicePool* q = new DevicePool();  // (never destroyed: plans may be destroyed during static destruction)
    return *q;
  }
  static constexpr size_t kMinPooled = size_t(256) << 10;
  hipError_t alloc(void** out, size_t bytes) {
    *out = nullptr;
    g_alloc_tally += bytes;
    if (bytes < kMinPooled || cap == 0) return hipMalloc(out, bytes);
    int device = 0;
    (void)hipGetDevice(&device);
    const size_t want = (bytes + (size_t(2) << 20) - 1) & ~((size_t(2) << 20) - 1);
    {
      std::lock_guard<std::mutex> lock(mu);
      int best = -1;
      for (size_t i = 0; i < free_blocks.size(); i++) {
        const Block& b = free_blocks[i];
        if (b.device != device || b.bytes < want || b.bytes > want + want / 4) continue;
        if (best < 0 || b.bytes < free_blocks[size_t(best)].bytes) best = int(i);
      }
      if (best >= 0) {
        const Block b = free_blocks[size_t(best)];
        free_blocks.erase(free_blocks.begin() + best);
        pooled -= b.bytes;
        live[b.p] = b;
        *out = b.p;
        return hipSuccess;
      }
    }
    hipError_t e = hipMalloc(out, want);
    if (e != hipSuccess) {  // memory is short: give the pool back and try once more
      release_all();
      (void)hipGetLastError();
      e = hipMalloc(out, want);
    }
    if (e == hipSuccess) {
      std::lock_guard<std::mutex> lock(mu);
      live[*out] = Block{*out, want, device};
    }
    return e;
  }
  // the size of the block alloc handed out for `bytes`: the rounded size of a pooled one (PINE_GPU_TEST_POISON fills all of it)
  size_t block_bytes(void* p, size_t bytes) {
    std::lock_guard<std::mutex> lock(mu);
    auto it = live.find(p);
    return it != live.end() ? it->second.bytes : bytes;
  }
  void free(void* p) {
    if (!p) return;
    Block b{nullptr, 0, 0};
    {
      std::lock_guard<std::mutex> lock(mu);
      auto it = live.find(p);
      if (it != live.end()) {
        b = it->second;
        live.erase(it);
        if (pooled + b.bytes <= cap) {
          free_blocks.push_back(b);
          pooled += b.bytes;
          return;
        }
      }
    }
    (void)hipFree(p);  // (a small allocation, or the pool is full)
  }
  void release_all() {
    std::vector<Block> blocks;
    {
      std::lock_guard<std::mutex> lock(mu);
      blocks.swap(free_blocks);
      pooled = 0;
    }
    int keep = 0;
    (void)hipGetDevice(&keep);
    for (const Block& b : blocks) {
      (void)hipSetDevice(b.device);
      (void)hipFree(b.p);
    }
    (void)hipSetDevice(keep);
  }
};
}  // namespace pine_gpu
#include "pine_device_buffer.h"
#include "pine_scene_kernel.h"
namespace pine_gpu {

// The frame table of a scene's shapes (pine_device.h frame_entry): one entry per face of every Rect, AABB and OBB
// in geometry order, kFrameFloats floats each; base[g] = the first entry of shape g, or -1 for a kind without faces.
inline void build_frame_table(const std::vector<DShape>& shapes, std::vector<float>& entries, std::vector<int>& base) {
  entries.clear();
  base.assign(shapes.size(), -1);
  for (size_t g = 0; g < shapes.size(); g++) {
    const int faces = frame_faces(shapes[g].kind);
    if (faces == 0) continue;
    base[g] = int(entries.size() / kFrameFloats);
    for (int face = 0; face < faces; face++) {
      entries.resize(entries.size() + kFrameFloats);
      frame_entry(&shapes[g], face, &entries[entries.size() - kFrameFloats]);
    }
  }
}

// A sampler's tables as the kernels read them, from the packed table file, the sampler (DTables::kind; spp: BlueSampler's effective
// count, the others' as given) and the film size (pine_kernels.hip): what a plan's kernels get, and pine_gpu_test_sampler_draws.
// T views the two blocks, which own the memory on the current device -- or, with host_tables, host memory: that vector and the
// library's own copy of HaltonSampler's tables (no device is touched: the host pass of the test hook).
int fill_sampler_tables(const std::vector<uint8_t>& tables, int kind, int spp, int W, int H, DTables& T, DeviceBuffer<uint8_t>& d_tables,
                        DeviceBuffer<uint8_t>& d_halton, std::vector<uint8_t>* host_tables = nullptr);

static int need_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error("no HIP device available");
    return -1;
  }
  HIP_OK(hipSetDevice(device));
  return 0;
}

}  // namespace pine_gpu

using namespace pine_gpu;

struct pine_gpu_plan {
  int device = 0;
  pine_gpu_render_params params{};
  DeviceScene S{};
  WorkParams W{};
  int film_w = 0, film_h = 0;
  // device buffers: blocks of the pool (the plan's last launch has finished before `delete` gives them back: pine_gpu_plan_destroy)
  DeviceBuffer<char> d_blob{kFromPool};  // nodes | shapes | materials | bvhs | prims | lights | frame table
  DeviceBuffer<float> d_tri{kFromPool};
  DeviceBuffer<float> d_tri_leaf{kFromPool};
  DeviceBuffer<uint32_t> d_tri_packets{kFromPool};  // (DeviceScene::tri_packets views it as uint4)
  DeviceBuffer<uint8_t> d_halton{kFromPool};
  DeviceBuffer<float> d_tri_attrs{kFromPool};
  DeviceBuffer<float> d_tex{kFromPool};  // image nodes: what compile_node_programs collected (null: no program reads an image)
  DeviceBuffer<float> d_env{kFromPool};  // ImageSky, Atmosphere: SceneHost::env_words (null: another environment light, or none)
  DeviceBuffer<uint8_t> d_tables{kFromPool};
  int variant = -1;
  int queue_variant = -1;   // >= 0: the stage-queued kernel is used instead of path_trace_kernel
  const PineFastVariant* fast = nullptr;  // PINE_GPU_FLAG_FAST: the declared-tolerance variant that runs instead (pine_kernels_fast.hip)
  DeviceBuffer<uint32_t> d_ctxg{kFromPool};
  DeviceBuffer<ulonglong2> d_ckpt{kFromPool};
  // The RNG checkpoints are a function of the film partition and the sample counts alone: the FIRST launch of a plan of one pass
  // computes them, later launches reuse the table (they wait for `ckpt_done` when they run on another stream).
  // $PINE_GPU_CKPT_EVERY_LAUNCH=1: as before round 4, every launch recomputes it (measurement aid).  A plan of several passes
  // keeps the checkpoints of one pass only: each pass computes its own from the carried states.
  bool ckpt_valid = false, ckpt_every_launch = false;
  EventOwner ckpt_done;
  hipStream_t ckpt_stream = nullptr;
  DeviceBuffer<float> d_vertex_log{kFromPool};  // test hook (pine_gpu_plan_vertex_log)
  DeviceBuffer<int> d_tile_order{kFromPool};    // tile classes (WorkParams::tile_order), or null
  std::vector<int> tile_order;                  // ... its host copy (empty: local tile t is film tile t * shard_world + shard_rank)
  DeviceBuffer<float4> d_samples{kFromPool};
  // Passes: every launch is a pass of pass_plan (pass_plan.n == 1: an ordinary plan, none of the buffers below).  The running sum is
  // one float4 per local pixel ([local tile][pixel in tile], .w unused); the carried RNG states one per pixel of the independent class.
  int pass_samples_req = 0;
  PassPlan pass_plan;
  int next_pass = 0;                        // the pass that may be launched next (0 may always be)
  DeviceBuffer<float4> d_sum{kFromPool};
  DeviceBuffer<ulonglong2> d_rng_carry{kFromPool};
  size_t bytes_samples = 0, bytes_ckpt = 0, bytes_carry = 0, bytes_total = 0;
  DeviceBuffer<float> d_fold{kFromPool};
  DeviceBuffer<Counters> d_counters{kFromPool};
  int grid = 0;
  size_t lds_bytes = 0;
  bool serial_rng = false;
  // per-launch HIP events (prepass start / path kernel start / resolve start / end) for the last
  // kEvRing launches: reading them (stats_get) averages over the launches since the previous read,
  // so a timed loop never has to synchronise inside
  static constexpr int kEvRing = 64;
  EventOwner ev[kEvRing][4];
  unsigned long long launch_count = 0, stats_read_upto = 0;
  bool timed = false;
  bool launched = false;
  hipStream_t last_stream = nullptr;
  PinnedOwner<unsigned long long> h_progress;  // host-mapped progress word (PINE_GPU_FLAG_PROGRESS)
  float accel_build_ms = 0.0f, upload_ms = 0.0f;  // host-side cost of plan creation (reported by stats_get)
  bool accel_on_device = false;
  // the stage-queued kernel compiled for this scene (pine_scene_kernel.h), when there is one: it launches instead of the variant
  SceneKernel scene_kernel;
  // An AOIntegrator plan (pine_gpu_ao_plan_create, pine_ao_host.h): S.spp is the AO sample count, the kernel one of
  // pine_gpu_ao_variants() in the schedule `ao_serial` selects; per film pixel one counter of unoccluded rays.
  bool ao = false, ao_serial = false;
  int ao_variant = -1;
  AoParams ao_params{};
  DeviceBuffer<unsigned> d_ao_counts{kFromPool};
};
// A plan held for the length of a call (the one-shot renders, the multi-device render, pine_gpu_test_traverse).
struct PlanDeleter {
  void operator()(pine_gpu_plan* p) const { pine_gpu_plan_destroy(p); }
};
using PlanOwner = std::unique_ptr<pine_gpu_plan, PlanDeleter>;
