// pine_amd/csrc/pine_kernels.hip -- the PathIntegrator hot path on gfx950 (MI355X).
//
// Formulation (DESIGN.md has the long version):
//  * A persistent grid of 64-lane waves.  Each lane owns one *work item* = `samples_per_item`
//    consecutive camera samples of one pixel, and runs the reference's radiance() recursion as an
//    iterative state machine: one radiance() invocation ("path vertex") per loop trip.  A lane
//    whose path ends regenerates immediately (next sample of its item, or a new item pulled from a
//    global queue with one wave-aggregated atomic), so all 64 lanes stay busy until the queue runs
//    dry -- the exit condition every wave reaches.
//  * The per-level firefly clamp of the reference (path.cpp:121) forces a backward fold of
//    per-vertex terms; each non-terminal vertex spills a 32-byte FoldEntry to a lane-interleaved
//    global stack and the terminal vertex folds it back.
//  * Per-sample radiance goes to a [tile][sample][pixel-in-tile] buffer; a second kernel sums each
//    pixel's samples in sample order (the reference's `L += ...` order, path.cpp:34-37) so the
//    film is independent of scheduling and of the number of GPUs.
//  * The per-pixel RNG stream (pixel jitter) is sequential across a pixel's samples; a prepass
//    computes its state at every item boundary when the scene has no in-path RNG consumer,
//    otherwise one item = the whole pixel.
//
// No MFMA (no dense contraction here); the kernel is VALU/latency bound on cbox-class scenes.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "pine_plan.h"
#include "pine_bvh_build_device.h"
#include "pine_embree_order.h"
#include "../data/rcpps_table.h"
namespace pine_gpu {

// ---- the Atmosphere light's tables (pine_atmosphere.h): one thread per grid point of the (w + 1) x (h + 1) grid ----
__global__ void __launch_bounds__(256) atmosphere_table_kernel(f3 sun, int w, int h, float* __restrict__ colors, float* __restrict__ density) {
  const long long t = blockIdx.x * 256ll + threadIdx.x;
  if (t >= (long long)(w + 1) * (h + 1)) return;
  atmosphere_table_entry(int(t % (w + 1)), int(t / (w + 1)), w, h, sun, colors, density);
}
int atmosphere_table_device(int device, const float sun_dir[3], int w, int h, float* colors, float* density) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    set_error("no HIP device available: the Atmosphere tables were asked of a device (device = -1 builds them on the host)");
    return -1;
  }
  if (device >= ndev || w < 1 || h < 1 || (long long)w * h > (1ll << 22)) {
    set_error("bad argument");
    return -1;
  }
  const size_t grid = size_t(w + 1) * size_t(h + 1), n = size_t(w) * size_t(h);
  int keep = 0;
  (void)hipGetDevice(&keep);  // (the caller's current device is the caller's)
  const int rc = [&] {
    const char* const what = "Atmosphere tables on the device";
    if (const hipError_t e = hipSetDevice(device)) return hip_error(what, e);
    DeviceBuffer<float> d_colors, d_density;
    if (d_colors.alloc(grid * 3, what) || d_density.alloc(n, what)) return -1;
    hipLaunchKernelGGL(atmosphere_table_kernel, dim3(unsigned((grid + 255) / 256)), dim3(256), 0, 0, ld3(sun_dir), w, h, d_colors.get(), d_density.get());
    if (hip_launch_check(what) || d_colors.download(colors, grid * 3, what) || d_density.download(density, n, what)) return -1;
    return 0;
  }();
  (void)hipSetDevice(keep);
  return rc;
}

// ---- the BVH build on the device: host orchestration (one decide / scan / split triple per level) ----
static int device_build(std::vector<BuildPrim>& prims, const std::vector<BuildTask>& roots, FlatAccel& A, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    return -1;
  }
  if (hipSetDevice(device) != hipSuccess) return -1;
  const size_t n = prims.size();
  // (every failure is silent -- no error text: the host build takes over)
  const size_t max_tasks = std::max<size_t>(n, roots.size()) + 2;
  DeviceBuffer<BuildPrim> d_prims, d_scratch;
  DeviceBuffer<BuildTask> d_tasks[2];
  DeviceBuffer<BuildDecision> d_dec;
  DeviceBuffer<int> d_rank, d_perm, d_src, d_counts;
  DeviceBuffer<unsigned char> d_pred;
  DeviceBuffer<DNode> d_nodes;
  DeviceBuffer<DBvh> d_bvhs;
  if (d_prims.upload(prims, nullptr) || d_scratch.alloc(n, nullptr) || d_tasks[0].alloc(max_tasks, nullptr) || d_tasks[0].write(roots.data(), roots.size(), nullptr) ||
      d_tasks[1].alloc(max_tasks, nullptr) || d_dec.alloc(max_tasks, nullptr) || d_rank.alloc(max_tasks, nullptr) || d_perm.alloc(n, nullptr) ||
      d_src.alloc(n, nullptr) || d_pred.alloc(n, nullptr) || d_nodes.alloc(n + 1, nullptr) || d_bvhs.upload(A.bvhs, nullptr) || d_counts.alloc(4, nullptr))
    return -1;
  int counts[4] = {0, 0, 0, 0};  // nodes so far | tasks of the next level | largest range of the next level
  int ntasks = int(roots.size()), node_base = 0, max_n = 0;
  for (const BuildTask& t : roots) max_n = std::max(max_n, t.end - t.begin);
  if (const hipError_t e = hipFuncSetAttribute((const void*)bvh_split_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kBuildLdsPrims * 9 + 16))
    return hip_error(nullptr, e);
  for (int cur = 0; ntasks > 0; cur ^= 1) {
    if (d_counts.write(counts, 4, nullptr)) return -1;
    hipLaunchKernelGGL(bvh_decide_kernel, dim3(ntasks), dim3(kBuildWave), 0, 0, d_prims.get(), d_tasks[cur].get(), ntasks, d_dec.get());
    hipLaunchKernelGGL(bvh_scan_kernel, dim3(1), dim3(1024), 0, 0, d_tasks[cur].get(), ntasks, d_dec.get(), d_rank.get(), d_nodes.get(), d_bvhs.get(), d_counts.get());
    const int lds_prims = std::min(max_n, kBuildLdsPrims);
    hipLaunchKernelGGL(bvh_split_kernel, dim3(ntasks), dim3(kSplitBlock), size_t(lds_prims) * 8 + ((size_t(lds_prims) + 15) & ~size_t(15)), 0, d_prims.get(), d_scratch.get(),
                       d_tasks[cur].get(), ntasks, d_dec.get(), d_rank.get(), node_base, d_nodes.get(), d_tasks[cur ^ 1].get(), d_perm.get(), d_src.get(), d_pred.get(), lds_prims,
                       d_counts.get() + 2);
    if (hip_launch_check(nullptr) || d_counts.download(counts, 4, nullptr)) return -1;
    node_base = counts[0];
    ntasks = counts[1];
    max_n = counts[2];
    counts[1] = counts[2] = 0;
    if (size_t(node_base) > n || size_t(ntasks) > max_tasks) return -1;  // (cannot happen: a binary tree over n leaves)
  }
  A.nodes.resize(size_t(node_base));
  if (d_nodes.download(A.nodes.data(), size_t(node_base), nullptr) || d_prims.download(prims.data(), n, nullptr) || d_bvhs.download(A.bvhs.data(), A.bvhs.size(), nullptr))
    return -1;
  return 0;
}
static const bool g_device_builder_installed = (g_device_builder = &device_build, true);

// Compiled specialisations (pine_variants.h): instantiated by the PART translation units (pine_kernels_part.hip, built in
// parallel), merged here in `order`; the host takes the first one that covers a scene.
struct VariantTables {
  std::vector<PineKernelVariant> queue, mega;
  VariantTables() {
    using PartFn = const PineKernelVariant* (*)(int*, int*);
    static const PartFn parts[kPineKernelParts] = {pine_gpu_kernel_part_0, pine_gpu_kernel_part_1, pine_gpu_kernel_part_2, pine_gpu_kernel_part_3,
                                                   pine_gpu_kernel_part_4, pine_gpu_kernel_part_5, pine_gpu_kernel_part_6, pine_gpu_kernel_part_7};
    for (PartFn f : parts) {
      int nq = 0, nm = 0;
      const PineKernelVariant* t = f(&nq, &nm);
      queue.insert(queue.end(), t, t + nq);
      mega.insert(mega.end(), t + nq, t + nq + nm);
    }
    auto by_order = [](const PineKernelVariant& a, const PineKernelVariant& b) { return a.order < b.order; };
    std::sort(queue.begin(), queue.end(), by_order);
    std::sort(mega.begin(), mega.end(), by_order);
  }
};
static const VariantTables& variant_tables() {
  static const VariantTables t;
  return t;
}
#define kVariants (variant_tables().mega)
#define kQueueVariants (variant_tables().queue)
#define kNumVariants (int(variant_tables().mega.size()))
#define kNumQueueVariants (int(variant_tables().queue.size()))

// The resolve: one wave per local tile runs resolve_tile (pine_kernels_device.h) -- over every tile that the path kernel has
// not summed itself (WorkParams::tile_done: the owned tiles of a stage-queued launch).
__global__ void __launch_bounds__(kBlock) resolve_kernel(WorkParams W, ResolvePass R, const float4* __restrict__ samples,
                                                        float4* __restrict__ sum, float4* __restrict__ film,
                                                        Counters* __restrict__ counters) {
  const unsigned long long t = blockIdx.x * (unsigned long long)kBlock + threadIdx.x;
  const int ltile = int(t >> 6);
  if (ltile >= W.num_local_tiles) return;  // (whole waves: one wave per tile)
  if (W.tile_done && W.tile_done[ltile]) return;
  unsigned long long verts = resolve_tile<8>(W, R, samples, sum, film, ltile, int(t & 63));
  // radiance() invocation count of the launch (the unit of the roofline's algorithmic bytes)
  for (int off = 32; off > 0; off >>= 1) verts += __shfl_down(verts, off);
  if ((threadIdx.x & 63) == 0 && verts) atomicAdd(&counters->vertices, verts);
}

// Multi-GPU: scatter the gathered per-rank slabs [rank][local tile][pixel in tile] into the row-major film.
__global__ void __launch_bounds__(kBlock) unpack_film_kernel(int film_w, int film_h, int tiles_x, int total_tiles, int world,
                                                            int tiles_per_rank, const float4* __restrict__ slabs,
                                                            float4* __restrict__ film) {
  const unsigned long long t = blockIdx.x * (unsigned long long)kBlock + threadIdx.x;
  const int tile = int(t >> 6);
  if (tile >= total_tiles) return;
  const int p = int(t & 63);
  const int px = (tile % tiles_x) * kTile + (p & 7), py = (tile / tiles_x) * kTile + (p >> 3);
  if (px >= film_w || py >= film_h) return;
  const int rank = tile % world, ltile = tile / world;
  film[size_t(py) * film_w + px] = slabs[(size_t(rank) * tiles_per_rank + ltile) * 64u + p];
}

// ================================================================================================
// Host side: plans, launches
// ================================================================================================
static std::atomic<float> g_progress{0.0f};
static std::atomic<const volatile unsigned long long*> g_progress_src{nullptr};
static std::atomic<unsigned long long> g_progress_total{0};
static std::atomic<unsigned long long> g_progress_base{0};  // (a render in passes: the items of the passes already done)
// depth of the inner-node tree below `node` (= traversal stack entries that can be live)
static int bvh_depth(const std::vector<DNode>& nodes, int node) {
  const DNode& n = nodes[node];
  int d = 0;
  for (int c = 0; c < 2; c++)
    if (n.count[c] == 0) d = std::max(d, bvh_depth(nodes, n.child[c]));
  return d + 1;
}

// Everything the kernels index with comes from these host arrays: check every index against its array BEFORE anything
// is uploaded or launched (an out-of-range access on the device can take the whole GPU down, for everyone on it).
static int validate_device_scene(const FlatAccel& A, const std::vector<DShape>& shapes, size_t num_materials,
                                 const std::vector<DLight>& lights, int stack_top, int stack_total) {
  const int n_nodes = int(A.nodes.size()), n_prims = int(A.prims.size()), n_tris = int(A.tri_verts.size() / 9);
  auto bad = [](const std::string& what) {
    set_error("internal: inconsistent acceleration structure (" + what + ")");
    return -1;
  };
  if (A.bvhs.empty()) return bad("no top-level BVH");
  if (A.top_prim_begin < 0 || A.top_prim_begin > n_prims) return bad("top_prim_begin");
  if (A.tri_leaf.size() != size_t(A.top_prim_begin) * 12) return bad("tri_leaf size");
  if (!A.tri_attrs.empty() && A.tri_attrs.size() != size_t(n_tris) * 16) return bad("tri_attrs size");
  for (size_t b = 0; b < A.bvhs.size(); b++) {
    const DBvh& v = A.bvhs[b];
    const int lo = b == 0 ? A.top_prim_begin : 0, hi = b == 0 ? n_prims : A.top_prim_begin;
    if (v.root_count > 0) {
      if (v.root_start < lo || v.root_start + v.root_count > hi) return bad("root leaf range");
    } else if (v.root >= n_nodes || (v.root < 0 && b != 0)) return bad("root node");
    // depth-first walk of this BVH: child indices, leaf ranges, depth against the stack the kernels get
    std::vector<std::pair<int, int>> todo;
    if (v.root_count == 0 && v.root >= 0) todo.push_back({v.root, 1});
    size_t visited = 0;
    while (!todo.empty()) {
      const auto [node, depth] = todo.back();
      todo.pop_back();
      if (++visited > size_t(n_nodes)) return bad("cycle in the node graph");
      if (depth > (b == 0 ? stack_top : stack_total - stack_top) + 1) return bad("tree deeper than the traversal stack");
      for (int c = 0; c < 2; c++) {
        const int ch = A.nodes[size_t(node)].child[c], cnt = A.nodes[size_t(node)].count[c];
        if (cnt > 0) {
          if (ch < lo || ch + cnt > hi) return bad("leaf range");
        } else if (cnt < 0 || ch < 0 || ch >= n_nodes) return bad("child index");
        else todo.push_back({ch, depth + 1});
      }
    }
  }
  for (int i = 0; i < A.top_prim_begin; i++) {
    int tri;
    memcpy(&tri, &A.tri_leaf[size_t(i) * 12 + 9], 4);
    if (tri < 0 || tri >= n_tris) return bad("triangle index of a leaf record");
  }
  for (int i = A.top_prim_begin; i < n_prims; i++)
    if (A.prims[size_t(i)] < 0 || A.prims[size_t(i)] >= int(shapes.size())) return bad("geometry index of a top-level primitive");
  for (const DShape& sh : shapes) {
    if (sh.material < 0 || size_t(sh.material) >= num_materials) return bad("material index");
    if (sh.kind == SHAPE_MESH) {
      int first, count, bvh;
      memcpy(&first, &sh.f[0], 4), memcpy(&count, &sh.f[1], 4), memcpy(&bvh, &sh.f[2], 4);
      if (count > 0 && (bvh < 1 || bvh >= int(A.bvhs.size()) || first < 0 || first + count > n_tris)) return bad("mesh record");
    }
  }
  for (const DLight& L : lights)
    if (L.kind == LIGHT_AREA && (L.geom < 0 || L.geom >= int(shapes.size()))) return bad("area light geometry");
  return 0;
}

}  // namespace pine_gpu

using namespace pine_gpu;

namespace pine_gpu {
AbiFingerprint abi_fingerprint() {
  return AbiFingerprint{sizeof(DeviceScene), sizeof(WorkParams), sizeof(Counters), sizeof(DNode), sizeof(DShape), sizeof(DMaterial), sizeof(DLight),
                        offsetof(WorkParams, total_items), offsetof(DeviceScene, cam), offsetof(DeviceScene, off_frames), kQFields, kQWinDwords, int(QC_WORDS), kQTokenDwords,
                        kTravRecordDwords, kQCtxGlobalDwordsPlain, kQCtxGlobalDwordsSss};
}
}  // namespace pine_gpu

// The plan-time measurement aids, read from the environment once per plan: the phases of plan_build read only
// this.  The numbers are kUnset when their variable is not set.
constexpr int kUnset = INT_MIN;
struct PlanKnobs {
  // PINE_GPU_SPECIALIZE (0: precompiled kernels only, else as PINE_GPU_FLAG_SPECIALIZE), _LDS_TRIS, _XSTAGE, _TRAV_MIN_LANES,
  // _TRAV_MIN_TRIPS, _MAX_PIXELS, _FAIR_PERIOD, _POOL_ITEMS
  int specialize, lds_tris, xstage, trav_min_lanes, trav_min_trips, max_pixels, fair_period, pool_items;
  // PINE_GPU_SPECIALIZE_FORCE, _NO_LDS_SCENE, _KERNEL=mega, _NO_TILE_CLASSES, _NO_FORK, _CKPT_EVERY_LAUNCH (not 0)
  bool specialize_force, no_lds_scene, mega, no_tile_classes, no_fork, ckpt_every_launch;
  double idle_budget_s;  // PINE_GPU_IDLE_BUDGET_S: the path kernel's watchdog, 30 s
  // Test hooks (tests/test_kernel_matrix.py).  PINE_GPU_TEST_VARIANT=queue:<order> / mega:<order>: choose_variants considers
  // that precompiled variant only (pin_kind 0 / 1; -1 unset, 2 malformed) and the plan never specialises.
  // PINE_GPU_TEST_LDS_NODES=<n>: F_LDS_TOP variants cache at most n BVH nodes in LDS.
  int pin_kind, pin_order, lds_nodes_cap;
  // PINE_GPU_OWNED_TILES: tiles claimed whole and summed inside the stage-queued kernel (0: none, n: that many, unset: automatic;
  // size_and_allocate).  Test hook PINE_GPU_TEST_TILE_SLOTS=<n>: a workgroup's table of such tiles in flight has n slots.
  int owned_tiles, tile_slots;
  int frame_table;  // PINE_GPU_FRAME_TABLE (0: plans have no frame table)
};
static PlanKnobs read_knobs() {
  auto num = [](const char* name) { return getenv(name) ? atoi(getenv(name)) : kUnset; };
  auto set = [](const char* name) { return getenv(name) != nullptr; };
  const char* kernel = getenv("PINE_GPU_KERNEL");
  const char* budget = getenv("PINE_GPU_IDLE_BUDGET_S");
  const int ckpt = num("PINE_GPU_CKPT_EVERY_LAUNCH");
  int pin_kind = -1, pin_order = -1;
  if (const char* pin = getenv("PINE_GPU_TEST_VARIANT")) {
    const std::string s = pin;
    const size_t colon = s.find(':');
    const std::string kind = s.substr(0, colon), digits = colon == std::string::npos ? "" : s.substr(colon + 1);
    pin_kind = kind == "queue" ? 0 : kind == "mega" ? 1 : 2;
    if (digits.empty() || digits.size() > 6 || digits.find_first_not_of("0123456789") != std::string::npos) pin_kind = 2;
    else pin_order = atoi(digits.c_str());
  }
  return PlanKnobs{num("PINE_GPU_SPECIALIZE"), num("PINE_GPU_LDS_TRIS"), num("PINE_GPU_XSTAGE"), num("PINE_GPU_TRAV_MIN_LANES"),
                   num("PINE_GPU_TRAV_MIN_TRIPS"), num("PINE_GPU_MAX_PIXELS"), num("PINE_GPU_FAIR_PERIOD"), num("PINE_GPU_POOL_ITEMS"),
                   set("PINE_GPU_SPECIALIZE_FORCE"), set("PINE_GPU_NO_LDS_SCENE"), kernel && std::string(kernel) == "mega",
                   set("PINE_GPU_NO_TILE_CLASSES"), set("PINE_GPU_NO_FORK"), ckpt != kUnset && ckpt != 0,
                   budget && atof(budget) > 0 ? atof(budget) : 30.0, pin_kind, pin_order, num("PINE_GPU_TEST_LDS_NODES"),
                   num("PINE_GPU_OWNED_TILES"), num("PINE_GPU_TEST_TILE_SLOTS"), num("PINE_GPU_FRAME_TABLE")};
}

// Plan creation asks for the scene's own kernel (SceneKernel::request, pine_scene_kernel.h: the modes), unless the caller or the
// environment rules it out or the plan runs a kernel it does not replace.
static int plan_request_scene_kernel(pine_gpu_plan* p, const FlatAccel& A, const std::vector<DShape>& shapes, const std::vector<int>& packed_prims,
                                     const pine_gpu_render_params* prm, unsigned need, const PlanKnobs& K) {
  if (K.pin_kind >= 0) return 0;  // (PINE_GPU_TEST_VARIANT: the pinned variant renders; no cache lookup)
  // 1: the caller asked for the scene's kernel (failures are errors); 0: automatic, the default (failures are silent); -1: not at all
  int want = (prm->flags & PINE_GPU_FLAG_SPECIALIZE) ? 1 : (prm->flags & PINE_GPU_FLAG_NO_SPECIALIZE) ? -1 : 0;
  if (K.specialize != kUnset) want = K.specialize != 0 ? 1 : -1;
  if (want < 0 || p->queue_variant < 0 || (prm->flags & (PINE_GPU_FLAG_FAST | PINE_GPU_FLAG_VERTEX_LOG))) return 0;
  const SceneKernel::Mode mode = want == 0 ? SceneKernel::Mode::kAutomatic
                                 : (prm->flags & PINE_GPU_FLAG_SPECIALIZE_ASYNC) ? SceneKernel::Mode::kExplicitAsync : SceneKernel::Mode::kExplicit;
  // (a baked scene IS pine's visiting order as code: the EmbreeAccel order mode keeps to the feature-set level)
  const bool may_bake = !(prm->flags & (PINE_GPU_FLAG_SPECIALIZE_NO_BAKE | PINE_GPU_FLAG_ORDER_EMBREE));
  return p->scene_kernel.request(mode, p->device, kQueueVariants[p->queue_variant], need, may_bake, K.specialize_force, A, shapes, packed_prims);
}

static int plan_check_counters(const Counters& c) {
  if (c.bail_count == 0) return 0;
  static const char* const kWhat[] = {"?", "idle budget exhausted with work outstanding", "ring slot never filled", "item-pool lock never released",
                                      "work-item hand-out did not converge", "?", "scene-specialised kernel: a closest-hit ray with an unexpected tmax", "forced by PINE_GPU_FLAG_DEBUG_FORCE_BAIL"};
  char msg[256];
  snprintf(msg, sizeof msg, "path kernel bailed out (%llu wave(s)): code %llu (%s), operands 0x%llx 0x%llx -- the film of this launch is incomplete",
           c.bail_count, c.bail_code, c.bail_code < 8 ? kWhat[c.bail_code] : "?", c.bail_a, c.bail_b);
  set_error(msg);
  return -1;
}

#include "pine_plan_steps.h"  // what path plans, AO plans, the guide pass, accels and shaders build and launch alike, one function per step

// The launch side of a one-shot render (create, launch, download, destroy), which the path and the AO render share: a film from
// the pool, `run(film, bytes)` -- launches, downloads, checks; 0, PINE_GPU_RENDER_STOPPED or -1 -- while get_progress() follows
// the plan's progress word over `total_items`, the error kept across the cleanup.  After a failure a launch may still be
// running: nothing of it may touch a block the pool hands out again, so the device is synchronised before any goes back.
template <class Run>
static int one_shot_render(pine_gpu_plan* plan, unsigned long long total_items, Run run) {
  PlanOwner p(plan);
  int rc = -1;
  std::string keep;
  {
    DeviceBuffer<float4> film(kFromPool);
    if (film.alloc(size_t(p->film_w) * p->film_h, "one-shot render: the film") == 0) {
      g_progress_total.store(total_items);
      g_progress_base.store(0);
      g_progress_src.store(p->h_progress.get());
      rc = run(film.get(), size_t(p->film_w) * p->film_h * sizeof(float4));
    }
    g_progress_src.store(nullptr);
    g_progress_base.store(0);
    g_progress.store(rc == 0 ? 1.0f : 0.0f);
    if (rc < 0) {
      keep = pine_gpu_last_error();
      (void)hipDeviceSynchronize();
    }
  }
  p.reset();
  if (rc < 0) set_error(keep);
  return rc;
}

extern "C" {

float pine_gpu_progress(void) {
  // while a one-shot render is in flight: items claimed by the device / items of the launch
  const volatile unsigned long long* src = g_progress_src.load();
  if (src) {
    const unsigned long long total = g_progress_total.load();
    const float f = total ? float(double(g_progress_base.load() + *src) / double(total)) : 0.0f;
    return f < 1.0f ? f : 1.0f;
  }
  return g_progress.load();
}

/* Synchronise with the plan's last launch and report a protocol failure of its path kernel (a bounded
 * spin or the idle budget ran out: the film of that launch is incomplete).  0 = the launch completed. */
int pine_gpu_plan_check(pine_gpu_plan* p) {
  if (!p) {
    set_error("null argument");
    return -1;
  }
  if (!p->launched) return 0;
  HIP_OK(hipSetDevice(p->device));
  HIP_OK(hipStreamSynchronize(p->last_stream));
  Counters c;
  HIP_OK(hipMemcpy(&c, p->d_counters, sizeof c, hipMemcpyDeviceToHost));
  return plan_check_counters(c);
}

int pine_gpu_test_kernel_variants(int kind, uint32_t* features, int32_t* ctx, int32_t* order, int cap) {
  if (kind != 0 && kind != 1) {
    set_error("pine_gpu_test_kernel_variants: kind is 0 (stage-queued kernel) or 1 (megakernel)");
    return -1;
  }
  const std::vector<PineKernelVariant>& t = kind == 0 ? kQueueVariants : kVariants;
  for (int i = 0; i < int(t.size()) && i < cap; i++) {
    if (features) features[i] = t[size_t(i)].features;
    if (ctx) ctx[i] = t[size_t(i)].ctx;
    if (order) order[i] = t[size_t(i)].order;
  }
  return int(t.size());
}

int pine_gpu_set_table_path(const char* path) {
  if (!path) {
    set_error("null path");
    return -1;
  }
  std::lock_guard<std::mutex> lock(g_table_mutex);
  g_table_path = path;
  g_tables.reset();  // (plans being built keep their own snapshot)
  return 0;
}

void pine_gpu_plan_destroy(pine_gpu_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  // the plan's buffers go back to the pool (its members' destructors), which hands them to the next plan without the device-wide
  // synchronisation hipFree implies: the plan's last launch must have finished first
  if (p->launched) (void)hipStreamSynchronize(p->last_stream);
  delete p;
}

// HaltonSampler's tables for the device (sampler.cpp:39-62, lowdiscrepancy.cpp:5-17, primes.cpp): the first kHaltonDims
// primes, their prefix sums (PrimeSums) and, per prime p, a permutation of 0 .. p-1 -- the identity shuffled with ONE
// default-seeded RNG running through all the primes in order (shuffle(): element i swaps with i + next32u(p - i)), so the
// permutations of the first kHaltonDims primes are a prefix of the reference's table of 1000.  Derived, not stored.
struct HaltonHostTables {
  std::vector<int> primes_and_sums;  // [kHaltonDims] primes, [kHaltonDims] prefix sums
  std::vector<uint16_t> perms;
};
static const HaltonHostTables& halton_host_tables() {
  static const HaltonHostTables tables = [] {
    HaltonHostTables t;
    t.primes_and_sums.assign(size_t(2 * kHaltonDims), 0);
    int count = 0, sum = 0;
    for (int n = 2; count < kHaltonDims; n++) {
      bool prime = true;
      for (int d = 2; d * d <= n && prime; d++) prime = n % d != 0;
      if (!prime) continue;
      t.primes_and_sums[size_t(count)] = n;
      t.primes_and_sums[size_t(kHaltonDims + count)] = sum;
      sum += n;
      count++;
    }
    t.perms.resize(size_t(sum));
    DRng rng = rng_seed(0);  // `RNG rng;`
    for (int k = 0; k < kHaltonDims; k++) {
      const int p = t.primes_and_sums[size_t(k)];
      uint16_t* perm = &t.perms[size_t(t.primes_and_sums[size_t(kHaltonDims + k)])];
      for (int j = 0; j < p; j++) perm[j] = uint16_t(j);
      for (int j = 0; j < p; j++) {
        const uint64_t u = rng_next64(rng);  // RNG::next32u(n) = uint32(u ^ (u >> 32)) % n  (rng.h:107-114)
        const uint32_t other = uint32_t(j) + uint32_t(u ^ (u >> 32)) % uint32_t(p - j);
        std::swap(perm[j], perm[other]);
      }
    }
    return t;
  }();
  return tables;
}
int pine_gpu_test_halton_tables(uint32_t* crc32, int64_t* counts) {
  if (!crc32 || !counts) {
    set_error("pine_gpu_test_halton_tables: bad argument");
    return -1;
  }
  const auto crc = [](const void* data, size_t bytes) {  // CRC-32 as zlib computes it (reflected 0xedb88320)
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < bytes; i++) {
      c ^= static_cast<const uint8_t*>(data)[i];
      for (int b = 0; b < 8; b++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
  };
  const HaltonHostTables& ht = halton_host_tables();
  counts[0] = kHaltonDims, counts[1] = kHaltonDims, counts[2] = int64_t(ht.perms.size());
  crc32[0] = crc(ht.primes_and_sums.data(), size_t(kHaltonDims) * sizeof(int));
  crc32[1] = crc(ht.primes_and_sums.data() + kHaltonDims, size_t(kHaltonDims) * sizeof(int));
  crc32[2] = crc(ht.perms.data(), ht.perms.size() * sizeof(uint16_t));
  return 0;
}

// The mesh triangles as LDS-sized packets (DeviceScene::tri_packets): per leaf-ordered triangle an 8-byte entry -- three
// 16-bit numbers into the table of the scene's DISTINCT vertices (by bit pattern) and the 16-bit triangle index -- then the
// vertices as float4.  Returns false when a number does not fit 16 bits (the traversal then reads tri_leaf from memory).
static bool build_tri_packets(const FlatAccel& A, std::vector<uint32_t>& out, int& entries, int& verts) {
  entries = A.top_prim_begin;
  verts = 0;
  out.clear();
  if (entries <= 0) return false;
  if (size_t(entries) * 8 > 96 * 1024) return false;  // (the entries alone would not fit the LDS the variants leave: no point in building the table)
  struct Key {
    uint32_t a, b, c;
    bool operator<(const Key& o) const { return a != o.a ? a < o.a : b != o.b ? b < o.b : c < o.c; }
  };
  std::map<Key, uint32_t> index;
  std::vector<Key> table;
  std::vector<uint32_t> ent(size_t((entries + 1) & ~1) * 2, 0u);
  for (int i = 0; i < entries; i++) {
    uint32_t w[10];
    memcpy(w, &A.tri_leaf[size_t(i) * 12], sizeof w);
    uint32_t id[3];
    for (int k = 0; k < 3; k++) {
      const Key key{w[3 * k], w[3 * k + 1], w[3 * k + 2]};
      auto it = index.find(key);
      if (it == index.end()) {
        if (table.size() >= 65536) return false;
        it = index.emplace(key, uint32_t(table.size())).first;
        table.push_back(key);
      }
      id[k] = it->second;
    }
    if (w[9] >= 65536u) return false;  // (the triangle index, as tri_leaf stores it)
    ent[size_t(i) * 2] = id[0] | (id[1] << 16);
    ent[size_t(i) * 2 + 1] = id[2] | (w[9] << 16);
  }
  verts = int(table.size());
  out = ent;
  for (const Key& k : table) {
    out.push_back(k.a);
    out.push_back(k.b);
    out.push_back(k.c);
    out.push_back(0u);
  }
  return true;
}

// The plan's precompiled path kernel: the declared-tolerance variant, else the stage-queued one, else the megakernel's.  (The
// scene's own kernel, pine_gpu_plan::scene_kernel, replaces a stage-queued variant and keeps its contexts and LDS layout.)
struct PathKernel {
  const void* fn;
  unsigned features;
  int ctx;    // work items a workgroup holds: the stage-queued kernel's path contexts, the megakernel's threads
  int block;  // threads per workgroup
  bool queued() const { return block == kQBlock; }  // the stage-queued kernel (exact or declared-tolerance build)
};
static_assert(kQBlock != kBlock, "PathKernel::queued tells the two kernels apart by their workgroup size");
static PathKernel plan_kernel(const pine_gpu_plan* p) {
  if (p->ao) {
    int n = 0;
    const PineAoVariant& V = pine_gpu_ao_variants(&n)[p->ao_variant];
    return {p->ao_serial ? V.serial : V.regrouped, V.features, kBlock, kBlock};
  }
  if (p->fast) return {p->fast->fn, p->fast->features, p->fast->ctx, kQBlock};
  if (p->queue_variant >= 0) {
    const PineKernelVariant& V = kQueueVariants[p->queue_variant];
    return {V.fn, V.features, V.ctx, kQBlock};
  }
  const PineKernelVariant& V = kVariants[p->variant];
  return {V.fn, V.features, kBlock, kBlock};
}

// Local tile -> tile of the film: the host twin of film_tile_of.
static int plan_film_tile(const pine_gpu_plan* p, int ltile) {
  return p->tile_order.empty() ? ltile * p->W.shard_world + p->W.shard_rank : p->tile_order[size_t(ltile)];
}

// ---- plan_build and its phases, in the order it runs them ----
// What assemble_scene leaves for the later phases: host copies of the records it uploaded.
struct SceneParts {
  std::vector<DShape> shapes;
  std::vector<DMaterial> materials;  // literals folded, node programs attached
  std::vector<DNodeOp> node_ops;
  std::vector<float> tex;            // DeviceScene::tex (empty: no program reads an image)
  std::vector<int> packed_prims;     // top-level entries: geometry | emissive | kind (pine_types.h)
  std::vector<DLight> lights;        // + the environment light last (lightsampler.cpp:6-10)
  size_t tri_packet_bytes = 0;        // (0: no triangle packets, build_tri_packets)
  int blob_bytes_plain = 0;           // DeviceScene::blob_bytes without the frame table (equal: the scene has none)
};

// The samples per pixel the plan renders, or -1.
static int check_params(const SceneHost& H, const pine_gpu_render_params* prm) {
  if (!H.has_camera) {
    set_error("scene has no camera");
    return -1;
  }
  if (prm->max_path_length <= 0) {  // path.cpp:12-13
    set_error("`PathIntegrator` expect `max_path_length` to be positive");
    return -1;
  }
  if (prm->max_path_length > kMaxDepth) {
    set_error("max_path_length above the supported fold-stack depth (32)");
    return -1;
  }
  // BlueSampler(n): n rounded up to a power of two, clamped to 256 (sampler.cpp:115-121).  SobolSampler(n):
  // n as given (sampler.h:127-131); the work decomposition here needs a power of two.
  // HaltonSampler(n): n as given too (sampler.h:44-46).  Both run in the F_SOBOL kernel variants.
  const bool halton = prm->sampler == PINE_GPU_SAMPLER_HALTON;
  const bool sobol = prm->sampler == PINE_GPU_SAMPLER_SOBOL || halton;  // (the sampler is not BlueSampler)
  if (prm->sampler != PINE_GPU_SAMPLER_BLUE && !sobol) {
    set_error("unknown sampler kind");
    return -1;
  }
  const int spp = sobol ? prm->spp : effective_spp(prm->spp);
  if (spp <= 0) {
    set_error(halton ? "`HaltonSampler` should have positive samples per pixel"
                     : sobol ? "`SobolSampler` should have positive samples per pixel" : "samples per pixel must be positive");
    return -1;
  }
  if (sobol && spp > kMaxDeviceSpp) {  // (the packed path state holds 12 bits of sample index)
    set_error(halton ? "HaltonSampler on the device: at most 4096 samples per pixel" : "SobolSampler on the device: at most 4096 samples per pixel");
    return -1;
  }
  if (prm->shard_world < 1 || prm->shard_rank < 0 || prm->shard_rank >= prm->shard_world) {
    set_error("bad shard rank/world");
    return -1;
  }
  return spp;
}

// The scene's records on the device: the blob of small records, the triangles and their LDS packets; the traversal stack
// depth, checked with every index before anything is launched.
// `frames`: with the frame table (pine_plan.h build_frame_table) behind everything else that scene-in-LDS variants stage.
static int assemble_scene(pine_gpu_plan* p, SceneHost& H, const pine_gpu_render_params* prm, SceneParts& sp, bool frames) {
  const FlatAccel& A = H.accel;
  std::vector<DShape>& shapes = sp.shapes;
  for (auto& g : H.geometries) shapes.push_back(g.shape);
  // one blob for the small records (16-byte aligned sections), so a workgroup can stage it in LDS
  std::vector<char> blob;
  auto put = [&](const void* src, size_t bytes) {
    size_t off = (blob.size() + 15) & ~size_t(15);
    blob.resize(off + std::max<size_t>(bytes, 16));
    if (bytes) memcpy(blob.data() + off, src, bytes);
    return int(off);
  };
  DeviceScene& S = p->S;
  S.off_nodes = put(A.nodes.data(), A.nodes.size() * sizeof(DNode));
  S.off_shapes = put(shapes.data(), shapes.size() * sizeof(DShape));
  if (!H.compile_node_programs(sp.materials, sp.node_ops, sp.tex)) return -1;
  S.off_materials = put(sp.materials.data(), sp.materials.size() * sizeof(DMaterial));
  S.off_node_ops = put(sp.node_ops.data(), sp.node_ops.size() * sizeof(DNodeOp));
  S.off_bvhs = put(A.bvhs.data(), A.bvhs.size() * sizeof(DBvh));
  std::vector<int>& packed_prims = sp.packed_prims;
  if (!H.packed_prim_words(packed_prims)) return -1;
  S.off_prims = 0;  // (the primitive index list stays on the host: the leaf-ordered record copies below replace it)
  std::vector<DShape> leaf_shapes;  // SceneView::leaf
  for (size_t i = size_t(A.top_prim_begin); i < packed_prims.size(); i++) {
    DShape c = shapes[size_t(packed_prims[i] & kPrimIndexMask)];
    c.kind = packed_prims[i];
    leaf_shapes.push_back(c);
  }
  S.off_leaf = put(leaf_shapes.data(), leaf_shapes.size() * sizeof(DShape));
  S.top_prim_begin = A.top_prim_begin;
  sp.lights = H.lights;
  if (H.has_env) sp.lights.push_back(H.env);
  S.off_lights = put(sp.lights.data(), sp.lights.size() * sizeof(DLight));
  // PINE_GPU_FLAG_ORDER_EMBREE: the hierarchy EmbreeAccel walks over the non-mesh shapes (pine_embree_order.h), the meshes' places
  // in `leaf` (tested first), and -- behind the part of the blob that scene-in-LDS variants copy -- the RCPPS estimates
  const bool order_embree = (prm->flags & PINE_GPU_FLAG_ORDER_EMBREE) != 0;
  S.off_etree = S.off_emesh = S.off_rcpps = 0;
  S.etree_root = kEmbreeNoChild;
  S.num_emesh = 0;
  if (order_embree) {
    if (prm->flags & (PINE_GPU_FLAG_FAST | PINE_GPU_FLAG_VERTEX_LOG)) {
      set_error("PINE_GPU_FLAG_ORDER_EMBREE cannot be combined with PINE_GPU_FLAG_FAST / _VERTEX_LOG");
      return -1;
    }
    const int ntop = int(A.top_boxes.size() / 8);
    std::vector<float> boxes;
    std::vector<int> places, mesh_places;
    for (int t = 0; t < ntop; t++) {  // (FlatAccel::top_boxes: the meshes first, then the other shapes, each in geometry order)
      const float* r = &A.top_boxes[size_t(t) * 8];
      int geom, place = -1;
      memcpy(&geom, &r[3], 4);
      for (size_t i = size_t(A.top_prim_begin); i < A.prims.size(); i++)
        if (A.prims[i] == geom) place = int(i);
      if (place < 0) {
        set_error("internal: a top-level primitive without a leaf entry");
        return -1;
      }
      if (shapes[size_t(geom)].kind == SHAPE_MESH) {
        mesh_places.push_back(place);
      } else {
        boxes.insert(boxes.end(), {r[0], r[1], r[2], r[4], r[5], r[6]});
        places.push_back(place);
      }
    }
    EmbreeOrderTree tree;
    std::string why;
    if (!tree.build(boxes, places, why)) {
      set_error("PINE_GPU_FLAG_ORDER_EMBREE: " + why);
      return -1;
    }
    S.etree_root = tree.root;
    S.off_etree = put(tree.nodes.data(), tree.nodes.size() * sizeof(EmbreeNode));
    S.num_emesh = int(mesh_places.size());
    S.off_emesh = put(mesh_places.data(), mesh_places.size() * sizeof(int));
  }
  // (the RCPPS estimates ride in the part of the blob that scene-in-LDS variants stage when the scene is small enough to stay one
  //  of theirs with them -- three lookups per ray from LDS instead of L2 -- and behind it, in global memory only, otherwise)
  const bool table_in_lds = order_embree && blob.size() + sizeof(kRcppsTable) + 64 <= 32 * 1024;
  if (table_in_lds) S.off_rcpps = put(kRcppsTable, sizeof(kRcppsTable));
  blob.resize((blob.size() + 15) & ~size_t(15));
  sp.blob_bytes_plain = int(blob.size());
  S.off_frames = S.off_frame_base = 0;
  // (only stage S reads a frame, and it shades no emissive surface: a scene whose flat shapes are all lamps gets no table)
  bool shaded_flat = false;
  for (const DShape& sh : shapes) shaded_flat |= frame_faces(sh.kind) != 0 && H.materials[size_t(sh.material)].kind != MAT_EMISSIVE;
  if (frames && shaded_flat) {
    std::vector<float> entries;
    std::vector<int> base;
    build_frame_table(shapes, entries, base);
    {
      S.off_frames = put(entries.data(), entries.size() * sizeof(float));
      S.off_frame_base = put(base.data(), base.size() * sizeof(int));
      blob.resize((blob.size() + 15) & ~size_t(15));
    }
  }
  S.blob_bytes = int(blob.size());
  if (order_embree && !table_in_lds) S.off_rcpps = put(kRcppsTable, sizeof(kRcppsTable));
  const char* const what = "plan creation: the scene's records";
  if (p->d_blob.alloc(blob.size(), what) || p->d_blob.write(blob.data(), blob.size(), what)) return -1;
  if (p->d_tri.upload(A.tri_verts, what) || p->d_tri_leaf.upload(A.tri_leaf, what)) return -1;
  std::vector<uint32_t> tri_packets;
  int tri_packet_entries = 0, tri_packet_verts = 0;
  if (build_tri_packets(A, tri_packets, tri_packet_entries, tri_packet_verts)) {
    if (p->d_tri_packets.upload(tri_packets, what)) return -1;
  }
  sp.tri_packet_bytes = tri_packets.size() * 4;
  if (p->d_tri_attrs.upload(A.tri_attrs, what)) return -1;
  S.env = nullptr;
  if (H.has_env && (H.env.kind == LIGHT_IMAGE_SKY || H.env.kind == LIGHT_ATMOSPHERE)) {
    if (!env_image_valid(H.env, H.env_words)) {
      set_error("internal: inconsistent environment light buffer");
      return -1;
    }
    if (p->d_env.upload(H.env_words, what)) return -1;
    S.env = p->d_env;
  }
  S.tex = nullptr;
  if (!sp.tex.empty()) {
    if (!tex_ops_valid(sp.node_ops, sp.tex.size())) {
      set_error("internal: an image node reads outside the plan's image buffer");
      return -1;
    }
    if (p->d_tex.upload(sp.tex, what)) return -1;
    S.tex = p->d_tex;
  }

  S.blob = reinterpret_cast<const uint4*>(p->d_blob.get());
  S.nodes = reinterpret_cast<const DNode*>(p->d_blob + S.off_nodes);
  S.shapes = reinterpret_cast<const DShape*>(p->d_blob + S.off_shapes);
  S.materials = reinterpret_cast<const DMaterial*>(p->d_blob + S.off_materials);
  S.bvhs = reinterpret_cast<const DBvh*>(p->d_blob + S.off_bvhs);
  S.leaf = reinterpret_cast<const DShape*>(p->d_blob + S.off_leaf) - S.top_prim_begin;
  S.lights = reinterpret_cast<const DLight*>(p->d_blob + S.off_lights);
  S.node_ops = reinterpret_cast<const DNodeOp*>(p->d_blob + S.off_node_ops);
  S.tri_verts = p->d_tri, S.tri_leaf = reinterpret_cast<const float4*>(p->d_tri_leaf.get()), S.tri_attrs = p->d_tri_attrs;
  S.tri_packets = reinterpret_cast<const uint4*>(p->d_tri_packets.get()), S.tri_packet_entries = tri_packet_entries, S.tri_packet_verts = tri_packet_verts;
  S.lds_nodes = 0, S.lds_tris = 0;
  S.num_lights = int(sp.lights.size()), S.env_light = H.has_env ? int(sp.lights.size()) - 1 : -1, S.num_shapes = int(shapes.size());
  S.cam = H.camera;
  S.max_path_length = prm->max_path_length;
  int d_top = 0, d_mesh = 0;
  for (size_t b = 0; b < A.bvhs.size(); b++) {
    if (A.bvhs[b].root_count > 0 || A.bvhs[b].root < 0) continue;
    int d = bvh_depth(A.nodes, A.bvhs[b].root);
    if (b == 0) d_top = d;
    else d_mesh = std::max(d_mesh, d);
  }
  S.stack_top = d_top;
  S.stack_total = std::max(1, d_top + d_mesh);
  return validate_device_scene(A, shapes, sp.materials.size(), sp.lights, S.stack_top, S.stack_total);
}

// BlueSampler's tables (sobol + the selected spp variant), HaltonSampler's, SobolSampler's digit counts: T views what the two
// blocks own on the current device (pine_plan.h).  host_tables: no device is touched, BlueSampler's bytes go there and
// HaltonSampler's are viewed where halton_host_tables() keeps them.
extern "C++" int pine_gpu::fill_sampler_tables(const std::vector<uint8_t>& tables, int kind, int spp, int W, int H, DTables& T, DeviceBuffer<uint8_t>& d_tables,
                                  DeviceBuffer<uint8_t>& d_halton, std::vector<uint8_t>* host_tables) {
  const bool halton = kind == 2;
  const bool sobol = kind == 1 || halton;
  int k = 0;
  while ((1 << k) < spp) k++;
  if (sobol) k = 0;  // (SobolSampler reads no table; any variant keeps the BlueSampler window loads in bounds)
  // device layout: sobolT 64 KiB | scramble 128 KiB | rank 128 KiB | 64 bytes = rank[0..63] again, so
  // a pixel's 40 consecutive ranking bytes never need the reference's modulo wrap
  const char* const what = "plan creation: the sampler's tables";
  const uint8_t* const variant = tables.data() + 65536 + size_t(k) * 262144;
  const uint8_t* base = nullptr;
  if (host_tables) {
    *host_tables = transposed_sobol(tables);
    host_tables->insert(host_tables->end(), variant, variant + 262144);
    host_tables->insert(host_tables->end(), variant + 131072, variant + 131072 + 64);
    base = host_tables->data();
  } else {
    if (d_tables.alloc(65536 + 262144 + 64, what) || d_tables.write(transposed_sobol(tables).data(), 65536, what)) return -1;
    HIP_OK(hipMemcpy(d_tables + 65536, variant, 262144, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_tables + 65536 + 262144, variant + 131072, 64, hipMemcpyHostToDevice));
    base = d_tables;
  }
  T.sobol = base, T.scramble = base + 65536, T.rank = base + 65536 + 131072;
  T.lds_sobol = nullptr, T.lds_tile = nullptr, T.lds_scr = nullptr;
  T.tile_stride = 0, T.win_lo = 0, T.win_len = 0;
  T.kind = halton ? 2 : sobol ? 1 : 0;
  T.halton_primes = nullptr, T.halton_perms = nullptr;
  if (halton) {
    const HaltonHostTables& ht = halton_host_tables();
    const size_t head = size_t(2 * kHaltonDims) * sizeof(int), bytes = head + ht.perms.size() * sizeof(uint16_t);
    if (host_tables) {
      T.halton_primes = ht.primes_and_sums.data(), T.halton_perms = ht.perms.data();
    } else {
      if (d_halton.alloc(bytes, what)) return -1;
      HIP_OK(hipMemcpy(d_halton, ht.primes_and_sums.data(), head, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(d_halton + head, ht.perms.data(), ht.perms.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      T.halton_primes = reinterpret_cast<const int*>(d_halton.get()), T.halton_perms = reinterpret_cast<const uint16_t*>(d_halton + head);
    }
  }
  sobol_sampler_params(T, spp, W, H);
  return 0;
}
static int upload_sampler_tables(pine_gpu_plan* p, const std::vector<uint8_t>& tables, const pine_gpu_render_params* prm, int spp) {
  const int kind = prm->sampler == PINE_GPU_SAMPLER_HALTON ? 2 : prm->sampler == PINE_GPU_SAMPLER_SOBOL ? 1 : 0;
  return fill_sampler_tables(tables, kind, spp, p->S.cam.W, p->S.cam.H, p->S.tables, p->d_tables, p->d_halton, nullptr);
}

// The F_* features the scene needs: kernel specialisation takes the smallest compiled feature set that covers them.
static unsigned scene_features(const SceneParts& sp, const pine_gpu_render_params* prm) {
  unsigned need = 0;
  for (auto& sh : sp.shapes) {
    switch (sh.kind) {
      case SHAPE_AABB: need |= F_AABB; break;
      case SHAPE_OBB: need |= F_OBB; break;
      case SHAPE_SPHERE: need |= F_SPHERE; break;
      case SHAPE_DISK: need |= F_DISK; break;
      case SHAPE_CONE: need |= F_CONE; break;
      case SHAPE_MESH: need |= F_MESH; break;
      case SHAPE_PLANE: case SHAPE_LINE: case SHAPE_CYLINDER: case SHAPE_TRIANGLE: need |= F_XSHAPES; break;
      default: break;
    }
  }
  for (auto& m : sp.materials) {
    if (m.kind == MAT_UBER || m.kind >= MAT_METAL) need |= F_UBER;  // the microfacet lobes
    if (m.kind == MAT_SUBSURFACE) need |= F_SSS;
  }
  if (!sp.node_ops.empty()) need |= F_NODES;
  if (prm->sampler == PINE_GPU_SAMPLER_SOBOL || prm->sampler == PINE_GPU_SAMPLER_HALTON) need |= F_SOBOL;
  if (prm->flags & PINE_GPU_FLAG_ORDER_EMBREE) need |= F_EMBREE;
  // (SobolSampler / HaltonSampler with Subsurface: a BSSRDF walk draws from the sampler at every step and the sampler's dimension
  //  counter outgrows the packed path state -- the F_SSS | F_SOBOL variants keep it in a word of its own: kBigDim)
  for (auto& L : sp.lights)
    if (L.kind != LIGHT_AREA) need |= F_LIGHTS;
  return need;
}

// A stage-queued variant's (exact or declared-tolerance) LDS bytes for this scene before the node and triangle caches; 0 when
// its layout does not fit.
static size_t queue_variant_lds(const PineKernelVariant& V, const DeviceScene& S, size_t num_nodes, bool lds_ok) {
  const unsigned F = V.features;
  if ((F & F_LDS_SCENE) && !lds_ok) return 0;  // (a scene-in-global variant later in the table is the fallback when LDS is short)
  if ((F & F_LDS_TOP) && num_nodes > 65535) return 0;  // 16-bit stack entries
  const size_t rest_bytes = size_t(S.blob_bytes - S.off_shapes);
  if ((F & F_LDS_REST) && rest_bytes > 12 * 1024) return 0;
  const size_t stack_bytes = std::max(V.min_stack, size_t(S.stack_total) * kQBlock * ((F & F_LDS_TOP) ? sizeof(unsigned short) : sizeof(int)));
  const size_t lds = V.fixed_lds + stack_bytes + ((F & F_LDS_SCENE) ? size_t(S.blob_bytes) : 0) + ((F & F_LDS_REST) ? rest_bytes : 0);
  return lds > 160 * 1024 ? 0 : lds;
}

// LDS left after a stage-queued variant's fixed parts goes to the BVH node cache first, then -- when ALL nodes are in and there
// is still room -- to the triangle packets.  Measured on the icosphere scene (profiles/HISTORY.md 6.3): packets in place of the
// 288 deepest nodes change nothing (191.7 vs 190.1 ms), so nodes are never evicted for them.
// PINE_GPU_LDS_TRIS=0 / 1: never / whenever the packets fit, before the nodes (measurement aid).
static void place_lds_caches(pine_gpu_plan* p, unsigned F, size_t lds, const FlatAccel& A, const SceneParts& sp, const PlanKnobs& K) {
  DeviceScene& S = p->S;
  bool tris = false;
  if ((F & F_LDS_TOP) && (F & F_MESH) && sp.tri_packet_bytes > 0 && lds < 160 * 1024 && K.lds_tris != 0) {
    const size_t room = 160 * 1024 - lds;
    tris = K.lds_tris == 1 ? sp.tri_packet_bytes <= room : sp.tri_packet_bytes + A.nodes.size() * sizeof(DNode) <= room;
  }
  p->lds_bytes = lds;
  S.lds_nodes = 0;
  S.lds_tris = tris ? 1 : 0;
  if (S.lds_tris) p->lds_bytes += sp.tri_packet_bytes;
  if (F & F_LDS_TOP) {
    S.lds_nodes = int(std::min<size_t>(A.nodes.size(), (160 * 1024 - p->lds_bytes) / sizeof(DNode)));
    if (K.lds_nodes_cap != kUnset) S.lds_nodes = std::min(S.lds_nodes, std::max(K.lds_nodes_cap, 0));  // (test hook: the cache's edge)
    p->lds_bytes += size_t(S.lds_nodes) * sizeof(DNode);
  }
}

// PINE_GPU_TEST_VARIANT (test hook, tests/test_kernel_matrix.py): the one precompiled variant the knob names, under the rules of
// the first-fit search below -- except that a pinned scene-in-global megakernel variant may take a scene that would fit LDS, and
// a pinned traversal-stage variant a scene without meshes (as PINE_GPU_XSTAGE=1 allows).  One that does not cover the scene
// fails the plan.
static int choose_pinned_variant(pine_gpu_plan* p, const FlatAccel& A, const SceneParts& sp, const pine_gpu_render_params* prm,
                                 unsigned need, bool lds_ok, const PlanKnobs& K) {
  DeviceScene& S = p->S;
  if (K.pin_kind == 2) {
    set_error("PINE_GPU_TEST_VARIANT: expected queue:<order> or mega:<order>");
    return -1;
  }
  if (prm->flags & PINE_GPU_FLAG_FAST) {
    set_error("PINE_GPU_TEST_VARIANT: not with PINE_GPU_FLAG_FAST (the declared-tolerance variants are not pinned)");
    return -1;
  }
  const bool mega = K.pin_kind == 1, order_embree = (prm->flags & PINE_GPU_FLAG_ORDER_EMBREE) != 0;
  const std::vector<PineKernelVariant>& table = mega ? kVariants : kQueueVariants;
  const std::string pin = std::string("PINE_GPU_TEST_VARIANT=") + (mega ? "mega:" : "queue:") + std::to_string(K.pin_order);
  int v = -1;
  for (int i = 0; i < int(table.size()); i++)
    if (table[size_t(i)].order == K.pin_order) v = i;
  if (v < 0) {
    set_error(pin + ": no such kernel variant");
    return -1;
  }
  const PineKernelVariant& V = table[size_t(v)];
  const unsigned F = V.features;
  const char* why = nullptr;
  size_t lds = 0;
  if ((F & need) != need) why = "the scene needs features it lacks";
  else if (((F & F_EMBREE) != 0) != order_embree) why = order_embree ? "not a variant of EmbreeAccel's order" : "a variant of EmbreeAccel's order";
  else if (!mega && ((F & F_VLOG) != 0) != ((prm->flags & PINE_GPU_FLAG_VERTEX_LOG) != 0))
    why = (F & F_VLOG) ? "a per-vertex-log twin: PINE_GPU_FLAG_VERTEX_LOG only" : "no per-vertex log compiled in";
  else if (mega && (F & F_LDS_SCENE) && !lds_ok) why = "the scene does not fit LDS";
  else if (!mega && (lds = queue_variant_lds(V, S, A.nodes.size(), lds_ok)) == 0) why = "its LDS layout does not fit the scene";
  if (why) {
    set_error(pin + ": pinned kernel variant does not cover this scene (" + why + ")");
    return -1;
  }
  if (mega) {
    p->variant = v, p->queue_variant = -1;
    if (F & F_LDS_SCENE) p->lds_bytes += size_t(S.blob_bytes);
  } else {
    p->variant = -1, p->queue_variant = v;
    place_lds_caches(p, F, lds, A, sp, K);
  }
  return 0;
}

// The kernel that renders: the first compiled variant that covers `need` -- of the stage-queued kernel when one fits, else of
// the megakernel; with PINE_GPU_FLAG_FAST one of the few declared-tolerance variants (pine_kernels_fast.hip).
static int choose_variants(pine_gpu_plan* p, const FlatAccel& A, const SceneParts& sp, const pine_gpu_render_params* prm, unsigned need,
                           const PlanKnobs& K) {
  DeviceScene& S = p->S;
  const bool order_embree = (prm->flags & PINE_GPU_FLAG_ORDER_EMBREE) != 0;
  p->lds_bytes = kLdsFixedBytes + size_t(S.stack_total) * kBlock * sizeof(int);
  if (p->lds_bytes > 64 * 1024) {
    set_error("BVH too deep for the LDS traversal stack");
    return -1;
  }
  const bool lds_ok = size_t(S.blob_bytes) <= 32 * 1024 && !K.no_lds_scene;
  if (K.pin_kind >= 0) return choose_pinned_variant(p, A, sp, prm, need, lds_ok, K);
  p->variant = -1;
  for (int v = 0; v < kNumVariants; v++) {
    const unsigned F = kVariants[v].features;
    if ((F & need) != need) continue;
    if (((F & F_LDS_SCENE) != 0) != lds_ok) continue;
    if (((F & F_EMBREE) != 0) != order_embree) continue;  // (the order mode's twin variants: never without the flag)
    p->variant = v;
    break;
  }
  if (p->variant >= 0 && (kVariants[p->variant].features & F_LDS_SCENE)) p->lds_bytes += size_t(S.blob_bytes);
  // The stage-queued kernel is the default whenever a variant covers the scene and its LDS fits;
  // PINE_GPU_KERNEL=mega forces the lane-owns-a-path kernel, which covers every scene.
  p->queue_variant = -1;
  for (int v = 0; v < kNumQueueVariants && !K.mega; v++) {
    const unsigned F = kQueueVariants[v].features;
    if ((F & need) != need) continue;
    if (((F & F_VLOG) != 0) != ((prm->flags & PINE_GPU_FLAG_VERTEX_LOG) != 0)) continue;  // (the test hook's twin variants)
    if (((F & F_EMBREE) != 0) != order_embree) continue;                                   // (the order mode's twin variants)
    const size_t lds = queue_variant_lds(kQueueVariants[v], S, A.nodes.size(), lds_ok);
    if (lds == 0) continue;
    // (measurement aid: PINE_GPU_XSTAGE=1 also passes over the stage-less F_LDS_TOP variants, so that the scene lands on a
    //  traversal-stage variant whose layout its own kernel -- exact feature set, pine_specialize.h -- then inherits)
    if ((F & F_LDS_TOP) && !(F & F_XSTAGE) && K.xstage == 1) continue;
    if (F & F_XSTAGE) {
      // traversal stages only where refilling pays: a scene with meshes, (nearly) all nodes in this variant's LDS.
      // PINE_GPU_XSTAGE=0 / 1: never / always (measurement aid, tools/xstage_ab.py).
      const size_t cached = std::min<size_t>(A.nodes.size(), (160 * 1024 - lds) / sizeof(DNode));
      bool want = (need & F_MESH) != 0 && cached * 10 >= A.nodes.size() * 9;
      if (K.xstage != kUnset) want = K.xstage != 0;
      if (!want) continue;  // (the same feature set without F_XSTAGE follows in the table)
    }
    p->queue_variant = v;
    place_lds_caches(p, F, lds, A, sp, K);
    break;
  }
  if (p->variant < 0 && p->queue_variant < 0) {  // (only experiment builds lack the all-features megakernel)
    set_error("no kernel variant covers this scene");
    return -1;
  }
  if (!(prm->flags & PINE_GPU_FLAG_FAST)) return 0;
  // declared-tolerance arithmetic: one of the few variants pine_kernels_fast.hip compiles, chosen by the same rules
  int nf = 0;
  const PineFastVariant* fv = pine_gpu_fast_variants(&nf);
  p->fast = nullptr;
  for (int v = 0; v < nf && !p->fast; v++) {
    const unsigned F = fv[v].features;
    if ((F & need) != need) continue;
    const size_t lds = queue_variant_lds(fv[v], S, A.nodes.size(), lds_ok);
    if (lds == 0) continue;
    p->fast = &fv[v];
    place_lds_caches(p, F, lds, A, sp, K);
  }
  if (!p->fast) {
    set_error("PINE_GPU_FLAG_FAST: no declared-tolerance kernel variant covers this scene (exact mode renders it)");
    return -1;
  }
  p->queue_variant = -1;
  return 0;
}

// The frame table pays where a hit reads it from LDS, so a plan keeps it only where its kernel stages it there with the rest of
// the blob (F_LDS_SCENE, F_LDS_REST) and is otherwise the kernel the plan would have had: the same variant, the same BVH nodes
// and triangle packets in LDS.  Everywhere else the plan has no table, and its kernel does no per-hit work for one.
static int choose_variants_with_frames(pine_gpu_plan* p, const FlatAccel& A, const SceneParts& sp, const pine_gpu_render_params* prm, unsigned need,
                                       const PlanKnobs& K) {
  DeviceScene& S = p->S;
  const int with_table = S.blob_bytes;
  auto choose = [&](int blob_bytes) {
    S.blob_bytes = blob_bytes;
    return choose_variants(p, A, sp, prm, need, K);
  };
  if (choose(sp.blob_bytes_plain)) return -1;
  if (S.off_frames == 0) return 0;
  const int variant = p->variant, queue_variant = p->queue_variant, lds_nodes = S.lds_nodes, lds_tris = S.lds_tris;
  const unsigned F = queue_variant >= 0 ? kQueueVariants[queue_variant].features : kVariants[variant].features;
  if ((F & (F_LDS_SCENE | F_LDS_REST)) != 0 && choose(with_table) == 0 && p->variant == variant && p->queue_variant == queue_variant &&
      S.lds_nodes == lds_nodes && S.lds_tris == lds_tris)
    return 0;
  // (assemble_scene has uploaded the table already: its bytes stay in d_blob behind blob_bytes, read by nobody and staged by no kernel)
  S.off_frames = S.off_frame_base = 0;
  return choose(sp.blob_bytes_plain);
}

// Tile classes (WorkParams::serial_tiles): in a scene whose only in-path RNG consumer is the BSSRDF channel pick and whose other
// materials are Diffuse / Emissive, a path draws from the pixel's RNG only while it has met nothing but Subsurface surfaces --
// so a pixel none of whose camera rays can reach a Subsurface shape makes NO in-path draw, its samples are independent (RNG
// state of sample s = the seed advanced 4 s steps, as in a scene without in-path draws) and need not form a chain.
// Conservative test per 8x8 tile: the world boxes of the Subsurface shapes projected through the pinhole camera, two pixels of
// margin.  Splits this shard's tiles into those a Subsurface shape may reach (`serial`) and the others (`free_tiles`); false
// (lists empty) when the camera or the materials rule the test out: a thin lens, a box behind the camera, other materials.
static bool tile_classes(const SceneHost& H, const SceneParts& sp, const WorkParams& W, std::vector<int>& serial, std::vector<int>& free_tiles) {
  if (H.camera.len_radius != 0.0f) return false;
  for (auto& m : sp.materials)
    if (m.kind != MAT_EMISSIVE && m.kind != MAT_DIFFUSE && m.kind != MAT_SUBSURFACE) return false;
  // inverse of the camera's linear part (columns x, y, z of c2w), in double
  const float* c = H.camera.c2w;
  const double a[3][3] = {{c[0], c[3], c[6]}, {c[1], c[4], c[7]}, {c[2], c[5], c[8]}};  // a[row][col]
  const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                     a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
  if (!(std::fabs(det) > 1e-12) || !(H.camera.fov2d[0] > 0) || !(H.camera.fov2d[1] > 0)) return false;
  double inv[3][3];
  inv[0][0] = (a[1][1] * a[2][2] - a[1][2] * a[2][1]) / det, inv[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det, inv[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det;
  inv[1][0] = (a[1][2] * a[2][0] - a[1][0] * a[2][2]) / det, inv[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det, inv[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det;
  inv[2][0] = (a[1][0] * a[2][1] - a[1][1] * a[2][0]) / det, inv[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det, inv[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
  // pixel rectangles [x0, x1] x [y0, y1] that the Subsurface shapes can project into
  struct Rect2 { double x0, y0, x1, y1; };
  std::vector<Rect2> rects;
  for (size_t g = 0; g < sp.shapes.size(); g++) {
    if (sp.materials[size_t(sp.shapes[g].material)].kind != MAT_SUBSURFACE) continue;
    const HostAABB b = H.geometry_aabb(int(g));
    Rect2 r{1e300, 1e300, -1e300, -1e300};
    for (int corner = 0; corner < 8; corner++) {
      const double P[3] = {double((corner & 1) ? b.upper.x : b.lower.x) - H.camera.position[0], double((corner & 2) ? b.upper.y : b.lower.y) - H.camera.position[1],
                           double((corner & 4) ? b.upper.z : b.lower.z) - H.camera.position[2]};
      if (!(std::isfinite(P[0]) && std::isfinite(P[1]) && std::isfinite(P[2]))) return false;
      const double qx = inv[0][0] * P[0] + inv[0][1] * P[1] + inv[0][2] * P[2], qy = inv[1][0] * P[0] + inv[1][1] * P[1] + inv[1][2] * P[2],
                   qz = inv[2][0] * P[0] + inv[2][1] * P[1] + inv[2][2] * P[2];
      if (!(qz > 1e-4)) return false;  // a corner at or behind the camera plane: no bounded projection
      const double fx = ((qx / qz) / H.camera.fov2d[0] * 0.5 + 0.5) * H.camera.W, fy = ((qy / qz) / H.camera.fov2d[1] * 0.5 + 0.5) * H.camera.H;
      r.x0 = std::min(r.x0, fx), r.y0 = std::min(r.y0, fy), r.x1 = std::max(r.x1, fx), r.y1 = std::max(r.y1, fy);
    }
    // margin: the pixel's own extent (jitter in [0, 1)) + two pixels for every rounding on the way
    r.x0 -= 3.0, r.y0 -= 3.0, r.x1 += 2.0, r.y1 += 2.0;
    rects.push_back(r);
  }
  for (int lt = 0; lt < W.num_local_tiles; lt++) {
    const int tile = lt * W.shard_world + W.shard_rank;
    const int tx = tile % W.tiles_x, ty = tile / W.tiles_x;
    const double x0 = tx * kTile, y0 = ty * kTile, x1 = x0 + kTile, y1 = y0 + kTile;
    bool touched = false;
    for (const Rect2& r : rects)
      if (x0 <= r.x1 && x1 >= r.x0 && y0 <= r.y1 && y1 >= r.y0) touched = true;
    (touched ? serial : free_tiles).push_back(tile);
  }
  return true;
}

// The work decomposition: tiles of this shard, samples per work item, tile classes.  Scenes whose materials draw from the
// per-pixel RNG inside radiance() (Uber with fractional metallic/transmission: sampler.h:317-324; BSSRDF channel pick:
// bxdf.cpp:335) make a pixel's samples sequentially dependent: one item = the whole pixel (p->serial_rng).
static int choose_items(pine_gpu_plan* p, const SceneHost& H, const SceneParts& sp, const pine_gpu_render_params* prm, int spp, const PlanKnobs& K,
                        bool& uber_rng) {
  bool in_path_rng = false;
  uber_rng = false;  // ... at any Uber vertex of a path, whatever came before it
  for (auto& m : sp.materials) {
    if (m.kind == MAT_SUBSURFACE) in_path_rng = true;
    if (m.kind == MAT_UBER && (m.prog[2] >= 0 || m.prog[3] >= 0)) uber_rng = true;  // value known only at the surface
    if (m.kind == MAT_UBER) {
      if (m.metallic != 0 && m.metallic != 1) uber_rng = true;
      if (m.metallic != 1 && m.transmission != 0 && m.transmission != 1) uber_rng = true;
    }
  }
  in_path_rng |= uber_rng;
  p->serial_rng = in_path_rng;
  const bool spp_pow2 = (spp & (spp - 1)) == 0;  // (BlueSampler's effective spp always is; SobolSampler / HaltonSampler take any count)
  const PathKernel kernel = plan_kernel(p);
  int kspi = prm->samples_per_item;
  if (in_path_rng) kspi = spp;
  else if (kspi <= 0) {
    // stage-queued kernel: two samples per item for the scene-in-LDS variants (cbox-class scenes, all pixels alike: half the
    // checkpoint prepass and hand-outs, C2 13.93 -> 13.75 ms per step, C3 69.9 -> 68.4), one where pixels differ a lot
    // (10 000 cones: 8.06 ms at one, 8.52 at two); the megakernel four
    kspi = kernel.queued() ? ((kernel.features & F_LDS_SCENE) ? std::min(spp, 2) : 1) : std::min(spp, 4);
  }
  if (kspi > spp) kspi = spp;
  if (!spp_pow2) {
    // SobolSampler(12): the work decomposition splits a pixel's samples by shifts and masks, so a count that is not a power
    // of two is ONE item per pixel -- all its samples in sequence, no checkpoints (sampler.cpp:81-113 takes any count)
    kspi = spp;
  } else {  // k must be a power of two dividing spp
    int k2 = 1;
    while (k2 * 2 <= kspi) k2 *= 2;
    kspi = k2;
  }

  WorkParams& W = p->W;
  p->film_w = H.camera.W;
  p->film_h = H.camera.H;
  if (shard_tiles(W, p->film_w, p->film_h, prm)) return -1;
  items_of_k_samples(W, spp, kspi);
  W.total_items = (unsigned long long)W.num_local_tiles * W.items_per_pixel * 64ull;
  W.tile_order = nullptr;
  W.serial_tiles = 0;
  // Everything but the Subsurface variants, Diffuse / Emissive scenes (the megakernel among them) keeps one whole-pixel item
  // per pixel; so does a shard none of whose tiles a Subsurface shape can reach (rare, and a launch without chains would need
  // the checkpoint prepass for every tile).  PINE_GPU_NO_TILE_CLASSES: off (measurement aid).
  std::vector<int> serial, free_tiles;
  if (in_path_rng && !uber_rng && kernel.queued() && (kernel.features & F_SSS) != 0 && !K.no_tile_classes && !K.no_fork && spp > 1 &&
      spp_pow2 &&  // (the independent class splits a pixel's samples by shifts and masks)
      tile_classes(H, sp, W, serial, free_tiles) && !free_tiles.empty() && !serial.empty()) {
    p->tile_order = serial;
    p->tile_order.insert(p->tile_order.end(), free_tiles.begin(), free_tiles.end());
    W.serial_tiles = int(serial.size());
    // the independent class: one sample per item, RNG checkpoints (the Subsurface variants are F_LDS_TOP ones)
    items_of_k_samples(W, spp, 1);
    W.total_items = (unsigned long long)W.serial_tiles * 64ull + (unsigned long long)(W.num_local_tiles - W.serial_tiles) * W.items_per_pixel * 64ull;
  }
  W.free_tile_base = W.serial_tiles;
  if (!plan_passes(W.num_local_tiles, spp, W.samples_per_item, W.serial_tiles, p->pass_samples_req, p->pass_plan)) return -1;
  // the 32-bit sample-buffer index covers one pass: its rows, and the rows before its first sample that decode_item adds to a
  // whole-pixel item's base (one pass: all tiles x 64 x spp)
  const PassPlan& PP = p->pass_plan;
  for (int j = 0; j < PP.n; j++)
    if ((PP.rows(j, spp) + unsigned(PP.pass(j, spp).first_sample)) * 64ull >= (1ull << 32)) {
      set_error(PP.n > 1 ? "film pixels x samples of one pass must stay below 2^32 (fewer samples per pass, or several shards)"
                         : "film pixels x samples per pixel of one shard must stay below 2^32 (render in several shards)");
      return -1;
    }
  return 0;
}

// The work decomposition of pass j: the plan's, with the pass window in place of the whole render.  The only pass of a plan of
// one (slice = the whole-pixel class, samples [0, spp)) gets the plan's W back, field for field.
static WorkParams pass_work(const pine_gpu_plan* p, int j) {
  WorkParams W = p->W;
  const int spp = p->S.spp;
  const PassPlan::Pass a = p->pass_plan.pass(j, spp);
  if (p->W.items_per_pixel == 1) {
    // every pixel is one whole-pixel item (one class, serial_tiles == 0): a slice of the shard's tiles
    W.free_tile_base = a.first_tile;
    W.total_items = (unsigned long long)a.tiles * 64ull;
    return W;
  }
  W.serial_tiles = a.tiles;
  W.pass_first_serial_tile = a.first_tile;
  W.free_tile_base = p->W.serial_tiles;
  W.pass_first_chunk = a.first_sample / W.samples_per_item;
  W.pass_chunks = a.samples / W.samples_per_item;
  W.pass_chunks_magic = W.pass_chunks > 1 ? unsigned(((1ull << 32) + unsigned(W.pass_chunks) - 1) / unsigned(W.pass_chunks)) : 0u;
  W.pass_row_stride = a.samples;
  W.total_items = (unsigned long long)a.tiles * 64ull + (unsigned long long)p->pass_plan.free_tiles * unsigned(W.pass_chunks) * 64ull;
  if (p->W.serial_tiles > 0 && a.tiles == 0) {
    // tile classes, a pass whose slice of whole-pixel tiles is empty: only independent one-sample items, no pixel's chain to
    // hand on and none in flight to bound
    W.fork_sealed = 0;
    W.max_pixels = 1 << 20;
  }
  return W;
}

// The scheduling defaults of the kernels (WorkParams), measurement aids applied.
static void schedule_params(pine_gpu_plan* p, const FlatAccel& A, const pine_gpu_render_params* prm, bool uber_rng, const PlanKnobs& K) {
  WorkParams& W = p->W;
  const bool in_path_rng = p->serial_rng;
  W.idle_budget_ticks = (unsigned long long)(K.idle_budget_s * 100e6);  // wall_clock64(): 100 MHz
  W.debug_force_bail = (prm->flags & PINE_GPU_FLAG_DEBUG_FORCE_BAIL) ? 1 : 0;
  // Traversal stages of the X variants (pine_queue_kernel.h): a wave goes to retire / refill its lanes when fewer than
  // trav_min_lanes of them are still travelling, at the earliest trav_min_trips trips after the last time.  Measured
  // (profiles/HISTORY.md 6.3): refilling pays when (nearly) the whole BVH sits in LDS (icosphere scene: 212 -> 185 ms); when most node
  // fetches go to L2 it costs -- the rays a wave picks up later are not the neighbours of the ones it has, and the
  // traversal waits on memory (10 000 cones: 9.8 ms without, 10.9 ms with) -- so there a wave runs its rays to the end.
  W.trav_min_lanes = (p->S.lds_nodes > 0 && size_t(p->S.lds_nodes) * 10 >= A.nodes.size() * 9) ? 48 : 0;  // (nearly) all nodes in LDS
  W.trav_min_trips = 8;
  // (a kernel with the top level baked in, pine_specialize.h: most rays end in the code part and free their lanes at once;
  //  refilling after three trips instead of eight: C5 107.3 -> 100.2 ms)
  if (p->scene_kernel.baked_top_requested()) W.trav_min_trips = 3;
  if (K.trav_min_lanes != kUnset) W.trav_min_lanes = K.trav_min_lanes;
  if (K.trav_min_trips != kUnset) W.trav_min_trips = K.trav_min_trips > 0 ? K.trav_min_trips : 1;
  // Subsurface is the only in-path user of the RNG and only before a path's first non-delta bounce: such a path hands its
  // pixel's next sample on when it has made that bounce (pine_queue_kernel.h, "sample tokens")
  W.fork_sealed = (in_path_rng && !uber_rng && !K.no_fork) ? 1 : 0;
  // ... and then a workgroup keeps at most 320 pixels in flight (each with one unsealed path; the other contexts trace the
  // sealed rest of earlier samples): when the work-item pool runs dry little is left half-done, so the workgroups end closer
  // together (C5: 178 -> 171 ms; 192 ... 384 within 1 %, 512 and more as without a limit)
  W.max_pixels = W.fork_sealed ? 320 : (1 << 20);
  if (K.max_pixels > 0) W.max_pixels = K.max_pixels;
  // A workgroup claims 512 items at a time; when an item is a pixel's whole sample sequence (serial-RNG scenes) that is
  // tens of milliseconds of its time, and the last claims decide when the launch ends: one 8x8 tile at a time there.
  W.pick_spins = 8;
  W.fair_period = 8;
  if (K.fair_period != kUnset) W.fair_period = K.fair_period;
  W.pool_items = in_path_rng ? 64 : 512;
  if (K.pool_items > 0) W.pool_items = K.pool_items;
  if (W.serial_tiles > 0) W.pool_items = 64;  // tile classes: a claim never straddles the boundary between the classes (a multiple of 64)
  W.progress = nullptr;
  W.vertex_log = nullptr;
}

// The launch shape (grid, work-item claims) and every buffer the launches use.
static int size_and_allocate(pine_gpu_plan* p, const pine_gpu_render_params* prm, int spp, const PlanKnobs& K) {
  const char* const what = "plan creation: the launch buffers";
  WorkParams& W = p->W;
  if (plan_progress_word(p, prm)) return -1;
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, prm->device));
  int blocks_per_cu = 0;
  const PathKernel kernel = plan_kernel(p);
  if (kernel.queued()) {
    blocks_per_cu = 1;  // one 1024-thread workgroup per CU owns the CU's LDS
    if (raise_lds_limit(prm->device, kernel.fn, p->lds_bytes)) return -1;
  } else {
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kernel.fn, kBlock, p->lds_bytes));
  }
  if (blocks_per_cu < 1) blocks_per_cu = 1;
  if (blocks_per_cu > 8) blocks_per_cu = 8;
  // (the launch shape, the claims and the buffers are sized for the plan's largest pass)
  const PassPlan& PP = p->pass_plan;
  unsigned long long launch_items = 0, sample_rows = 0;
  int ckpt_chunks = 0;
  for (int j = 0; j < PP.n; j++) {
    const WorkParams Wj = pass_work(p, j);
    launch_items = std::max(launch_items, Wj.total_items);
    sample_rows = std::max(sample_rows, PP.rows(j, spp));
    ckpt_chunks = std::max(ckpt_chunks, Wj.pass_chunks);
  }
  const unsigned long long want = (launch_items + kernel.ctx - 1) / kernel.ctx;
  p->grid = int(std::min<unsigned long long>(want, (unsigned long long)prop.multiProcessorCount * blocks_per_cu));
  if (p->grid < 1) p->grid = 1;
  if (!p->serial_rng && K.pool_items == kUnset) {
    // work-item claims of the stage-queued kernel: 1/32 of a workgroup's share, between 512 and 2048 (a claim is a run of
    // neighbouring tiles: larger ones keep a workgroup's camera rays together and are fewer -- 10 000 cones 8.00 -> 7.88 ms
    // at 2048, 7.81 at 4096, 8.4 at 8192 where the last claims unbalance the end; cbox indifferent up to 2048)
    unsigned long long share = launch_items / ((unsigned long long)p->grid * 32ull);
    int claim = 512;
    while (claim < 2048 && (unsigned long long)claim * 2ull <= share) claim *= 2;
    W.pool_items = claim;
  }
  // Owned tiles (WorkParams::owned_tiles): the plain variants of the stage-queued kernel, plans of one pass in the shard's
  // natural tile order.  Automatic: every tile but the last two per workgroup -- a whole tile is a large claim (C2: 8192 items,
  // four of today's), and the end of a launch needs small ones: with two tiles' worth of pool_items claims left per workgroup
  // the workgroup that takes the last owned tile still finds the others busy when it is done (the claims that "unbalance the
  // end" above were ALL 8192) -- and none where a tile is a smaller claim than pool_items (that would only multiply the
  // claims) or has fewer items than a workgroup has contexts (it would hand out several tiles at once and run out of slots).
  W.owned_tiles = 0;
  W.pool_items_log2 = 0;
  while ((1 << W.pool_items_log2) < W.pool_items) W.pool_items_log2++;
  W.tile_slots = K.tile_slots != kUnset ? std::max(0, std::min(K.tile_slots, kQTileSlots)) : kQTileSlots;
  const bool can_own = kernel.queued() && !(kernel.features & F_SSS) && !p->fast && PP.n == 1 && W.serial_tiles == 0 && p->tile_order.empty() &&
                       W.free_tile_base == 0 && (1 << W.pool_items_log2) == W.pool_items && W.total_items > 0;
  if (can_own) {
    const long long tile_items = 64ll * W.pass_chunks;
    long long owned = tile_items >= std::max(W.pool_items, kernel.ctx) ? (long long)W.num_local_tiles - 2ll * p->grid : 0;
    if (K.owned_tiles != kUnset) owned = K.owned_tiles;
    W.owned_tiles = int(std::max(0ll, std::min<long long>(owned, W.num_local_tiles)));
  }

  if (W.items_per_pixel > 1) {
    p->bytes_ckpt = (size_t)(W.num_local_tiles - W.serial_tiles) * ckpt_chunks * 64 * sizeof(ulonglong2);
    if (p->d_ckpt.alloc(p->bytes_ckpt / sizeof(ulonglong2), what)) return -1;
    if (PP.n > 1) {
      p->bytes_carry = (size_t)PP.free_tiles * 64 * sizeof(ulonglong2);
      if (p->d_rng_carry.alloc((size_t)PP.free_tiles * 64, what)) return -1;
    }
  }
  if (PP.n > 1) {
    if (p->d_sum.alloc((size_t)W.num_local_tiles * 64, what)) return -1;
    p->bytes_carry += (size_t)W.num_local_tiles * 64 * sizeof(float4);
  }
  p->ckpt_every_launch = K.ckpt_every_launch;
  if (!p->tile_order.empty()) {
    if (p->d_tile_order.upload(p->tile_order, what)) return -1;
    W.tile_order = p->d_tile_order;
  }
  p->bytes_samples = size_t(sample_rows) * 64 * sizeof(float4);
  if (p->d_samples.alloc(size_t(sample_rows) * 64, what)) return -1;
  const size_t fold_slots = size_t(p->grid) * kernel.ctx;
  if (p->d_fold.alloc(size_t(prm->max_path_length) * 8 * fold_slots, what)) return -1;
  if (kernel.queued()) {
    // per-context records, then (Subsurface variants) every workgroup's ring of sample-token slots
    const size_t token_dwords = (kernel.features & F_SSS) ? size_t(p->grid) * (kernel.ctx <= 1024 ? 1024 : 2048) * kQTokenDwords : 0;
    if (p->d_ctxg.alloc(size_t(p->grid) * kernel.ctx * q_ctx_global_dwords(kernel.features) + token_dwords, what)) return -1;
  }
  // (the owned tiles' done marks sit behind the counters: one clear for both)
  if (p->d_counters.alloc_bytes(sizeof(Counters) + (W.owned_tiles > 0 ? size_t(W.num_local_tiles) * sizeof(unsigned) : 0), what)) return -1;
  W.tile_done = W.owned_tiles > 0 ? reinterpret_cast<unsigned*>(p->d_counters + 1) : nullptr;
  return plan_timing_events(p, prm);
}

static int plan_build(pine_gpu_plan* p, pine_gpu_scene* scene, const pine_gpu_render_params* prm) {
  const PlanKnobs K = read_knobs();
  SceneHost& H = scene_host(scene);
  const int spp = check_params(H, prm);
  if (spp < 0) return -1;
  TableBlob tables_blob;
  if (load_tables(tables_blob)) return -1;
  std::chrono::steady_clock::time_point t_build1;
  if (plan_open_device(p, H, prm, "the PathIntegrator hot path", t_build1)) return -1;
  const size_t tally0 = g_alloc_tally;  // (the BVH build takes nothing from the pool)
  const FlatAccel& A = H.accel;

  SceneParts sp;
  // (the declared-tolerance kernels keep their own arithmetic for every normal: no table of exact ones)
  const bool frames = K.frame_table != 0 && !(prm->flags & PINE_GPU_FLAG_FAST);
  if (assemble_scene(p, H, prm, sp, frames) || upload_sampler_tables(p, *tables_blob, prm, spp)) return -1;
  p->S.spp = spp;
  const unsigned need = scene_features(sp, prm);
  if (choose_variants_with_frames(p, A, sp, prm, need, K) || plan_request_scene_kernel(p, A, sp.shapes, sp.packed_prims, prm, need, K)) return -1;
  bool uber_rng = false;
  if (choose_items(p, H, sp, prm, spp, K, uber_rng)) return -1;
  schedule_params(p, A, prm, uber_rng, K);
  if (size_and_allocate(p, prm, spp, K)) return -1;
  p->bytes_total = g_alloc_tally - tally0;
  HIP_OK(hipDeviceSynchronize());
  p->upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_build1).count();
  return 0;
}

static pine_gpu_plan* plan_create(pine_gpu_scene* scene, const pine_gpu_render_params* prm, int pass_samples) {
  return create_object(scene && prm, pine_gpu_plan_destroy, [&](pine_gpu_plan* p) {
    p->pass_samples_req = pass_samples;
    return plan_build(p, scene, prm);
  });
}
pine_gpu_plan* pine_gpu_plan_create(pine_gpu_scene* scene, const pine_gpu_render_params* prm) { return plan_create(scene, prm, 0); }
pine_gpu_plan* pine_gpu_plan_create_passes(pine_gpu_scene* scene, const pine_gpu_render_params* prm, int32_t pass_samples) {
  return plan_create(scene, prm, pass_samples);
}

#include "pine_scene_steps.h"  // the shared step that runs assemble_scene and scene_features: upload_scene_records
#include "pine_ao_host.h"  // AOIntegrator plans: ao_plan_build, ao_launch and the three pine_gpu_ao_* entry points
#include "pine_guides_host.h"  // DenoiseIntegrator's guide images: the pine_gpu_guides_* entry points
#include "pine_accel_host.h"  // Accel's batched ray queries: the pine_gpu_accel_* entry points
#include "pine_shade_host.h"  // Shader's batched path-vertex queries: the pine_gpu_shader_* entry points

// The path kernel of the plan -- the scene's own, or the precompiled one -- over the work decomposition W, its samples going
// to `samples` (+ sample index * 64, decode_item).
static int launch_path_kernel(pine_gpu_plan* p, WorkParams& W, float4* samples, int grid, hipStream_t stream) {
  const ulonglong2* ckpt = p->d_ckpt;
  float* fold = p->d_fold;
  uint32_t* ctxg = p->d_ctxg;
  Counters* counters = p->d_counters;
  const PathKernel kernel = plan_kernel(p);
  // (the kernels of the other translation units: same argument layout, launched untyped; the megakernel has no context records)
  void* queue_args[] = {&p->S, &W, &ckpt, &samples, &fold, &ctxg, &counters};
  void* mega_args[] = {&p->S, &W, &ckpt, &samples, &fold, &counters};
  if (const hipFunction_t own = p->scene_kernel.fn())
    HIP_OK(hipModuleLaunchKernel(own, unsigned(grid), 1, 1, kQBlock, 1, 1, unsigned(p->lds_bytes), stream, queue_args, nullptr));
  else
    HIP_OK(hipLaunchKernel(kernel.fn, dim3(grid), dim3(kernel.block), kernel.queued() ? queue_args : mega_args, p->lds_bytes, stream));
  return 0;
}

// Pass j of a path plan: checkpoint prepass, the path kernel over the pass window, the resolve that continues the running sum
// and writes the film.  A plan of one pass renders the whole film here.
static int path_launch_pass(pine_gpu_plan* p, int j, void* film_dev, hipStream_t stream, bool packed) {
  const PassPlan& PP = p->pass_plan;
  if (launch_begin(p, j, film_dev, stream, packed)) return -1;
  const int spp = p->S.spp;
  const PassPlan::Pass a = PP.pass(j, spp);
  WorkParams W = pass_work(p, j);
  W.film = (float4*)film_dev;
  W.film_packed = packed ? 1 : 0;
  if (launch_mark(p, 0, stream) || checkpoint_prepass(p, W, stream) || launch_mark(p, 1, stream)) return -1;
  // (a shard can own no tile at all -- more ranks than 8x8 tiles: nothing to launch, the film / slab stays zero)
  if (W.total_items > 0) {
    // (the largest pass fills p->grid: the only pass of a plan of one)
    const int ctx = plan_kernel(p).ctx;
    const int grid = int(std::min<unsigned long long>((unsigned long long)p->grid, (W.total_items + ctx - 1) / ctx));
    // (the rows before the pass's first sample are not in the buffer: see decode_item)
    float4* const samples = p->d_samples - size_t(W.pass_first_chunk) * size_t(W.samples_per_item) * 64u;
    if (launch_path_kernel(p, W, samples, grid, stream)) return -1;
  }
  if (launch_mark(p, 2, stream)) return -1;
  if (p->W.num_local_tiles > 0) {
    ResolvePass R;
    R.film_w = p->film_w, R.film_h = p->film_h, R.spp = spp;
    R.whole_tiles = PP.whole_tiles, R.slice_first = a.first_tile, R.slice_tiles = a.tiles;
    R.free_rows = a.samples, R.first_pass = j == 0 ? 1 : 0, R.samples_so_far = a.first_sample + a.samples;
    R.packed = packed ? 1 : 0;
    const unsigned long long n = (unsigned long long)p->W.num_local_tiles * 64ull;
    hipLaunchKernelGGL(resolve_kernel, dim3(unsigned((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, p->W, R, p->d_samples, p->d_sum,
                       (float4*)film_dev, p->d_counters);
  }
  if (launch_end(p, stream)) return -1;
  p->next_pass = j + 1;
  return 0;
}

// Pass j of the plan -- the only place that enqueues a render.  A launch that fails may have left the RNG checkpoints unwritten:
// the next one computes them again.
static int plan_launch_pass(pine_gpu_plan* p, int j, void* film_dev, hipStream_t stream, bool packed) {
  const PassPlan& PP = p->pass_plan;
  if (j < 0 || j >= PP.n || (j != 0 && j != p->next_pass)) {
    set_error("passes run in order: pass " + std::to_string(j) + " asked for, pass " + std::to_string(p->next_pass >= PP.n ? 0 : p->next_pass) +
              (p->next_pass > 0 && p->next_pass < PP.n ? " (or 0, which starts the film afresh)" : "") + " is next; nothing was launched");
    return -1;
  }
  if (p->ao && packed) return set_error("an AOIntegrator plan has no packed launch"), -1;
  const int rc = p->ao ? ao_launch(p, film_dev, stream) : path_launch_pass(p, j, film_dev, stream, packed);
  if (rc) p->ckpt_valid = false;
  return rc;
}

// All passes of the plan, in order.
static int plan_launch(pine_gpu_plan* p, void* film_dev, void* stream, bool packed) {
  if (!p || !film_dev) {
    set_error("null argument");
    return -1;
  }
  for (int j = 0; j < p->pass_plan.n; j++)
    if (plan_launch_pass(p, j, film_dev, (hipStream_t)stream, packed)) return -1;
  return 0;
}

void pine_gpu_release_cached_memory(void) {
  DevicePool::get().release_all();
  LoadedKernels::get().clear();
}

int pine_gpu_plan_launch(pine_gpu_plan* p, void* film_dev, void* stream) { return plan_launch(p, film_dev, stream, false); }
int pine_gpu_plan_launch_pass(pine_gpu_plan* p, int pass, void* film_dev, void* stream) {
  if (!p || !film_dev) {
    set_error("null argument");
    return -1;
  }
  if (p->pass_plan.n == 1 && pass != 0) {
    set_error("this plan has one pass: pass 0");
    return -1;
  }
  return plan_launch_pass(p, pass, film_dev, (hipStream_t)stream, false);
}
int pine_gpu_plan_pass_count(pine_gpu_plan* p) {
  if (!p) {
    set_error("null argument");
    return -1;
  }
  return p->pass_plan.n;
}
int pine_gpu_plan_pass_info(pine_gpu_plan* p, int pass, int32_t out[4]) {
  if (!p || !out) {
    set_error("null argument");
    return -1;
  }
  if (pass < 0 || pass >= p->pass_plan.n) {
    set_error("no such pass");
    return -1;
  }
  const PassPlan::Pass a = p->pass_plan.pass(pass, p->S.spp);
  out[0] = a.first_sample, out[1] = a.samples, out[2] = a.first_tile, out[3] = a.tiles;
  return 0;
}
int pine_gpu_plan_tile_order(pine_gpu_plan* p, int32_t* out, int cap) {
  if (!p || (cap > 0 && !out)) {
    set_error("null argument");
    return -1;
  }
  for (int lt = 0; lt < p->W.num_local_tiles && lt < cap; lt++)
    out[lt] = plan_film_tile(p, lt);
  return p->W.num_local_tiles;
}
int pine_gpu_plan_device_bytes(pine_gpu_plan* p, int64_t out[4]) {
  if (!p || !out) {
    set_error("null argument");
    return -1;
  }
  out[0] = int64_t(p->bytes_samples), out[1] = int64_t(p->bytes_ckpt), out[2] = int64_t(p->bytes_carry), out[3] = int64_t(p->bytes_total);
  return 0;
}
int pine_gpu_plan_launch_packed(pine_gpu_plan* p, void* slab_dev, void* stream) { return plan_launch(p, slab_dev, stream, true); }

int pine_gpu_film_unpack(int film_w, int film_h, int world, int device, const void* slabs_dev, void* film_dev, void* stream_) {
  if (!slabs_dev || !film_dev || film_w <= 0 || film_h <= 0 || world < 1) {
    set_error("bad argument");
    return -1;
  }
  HIP_OK(hipSetDevice(device));
  const int tiles_x = (film_w + kTile - 1) / kTile, tiles_y = (film_h + kTile - 1) / kTile;
  const int total = tiles_x * tiles_y;
  const int per_rank = (total + world - 1) / world;
  const unsigned long long n = (unsigned long long)total * 64ull;
  hipLaunchKernelGGL(unpack_film_kernel, dim3(unsigned((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream_,
                     film_w, film_h, tiles_x, total, world, per_rank, (const float4*)slabs_dev, (float4*)film_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

int pine_gpu_plan_stats_get(pine_gpu_plan* p, pine_gpu_plan_stats* out) {
  if (!p || !out) {
    set_error("null argument");
    return -1;
  }
  memset(out, 0, sizeof *out);
  HIP_OK(hipSetDevice(p->device));
  // tiles on the film border may be partially outside: count real pixels
  {
    unsigned long long px = 0;
    for (int lt = 0; lt < p->W.num_local_tiles; lt++) {
      int tile = plan_film_tile(p, lt);
      int tx = tile % p->W.tiles_x, ty = tile / p->W.tiles_x;
      int w = std::min(kTile, p->film_w - tx * kTile), h = std::min(kTile, p->film_h - ty * kTile);
      px += (unsigned long long)w * h;
    }
    out->camera_samples = px * p->S.spp;
  }
  out->spp_effective = p->S.spp;
  out->samples_per_item = p->W.samples_per_item;
  out->serial_tiles = p->W.serial_tiles;
  const PathKernel kernel = plan_kernel(p);
  p->scene_kernel.poll();
  p->scene_kernel.fill_stats(out, kernel.features);
  out->grid_blocks = p->grid;
  out->block_threads = kernel.block;
  out->lds_bytes = int(p->lds_bytes);
  out->accel_build_ms = p->accel_build_ms;
  out->accel_built_on_device = p->accel_on_device ? 1 : 0;
  out->upload_ms = p->upload_ms;
  if (p->launched) {
    HIP_OK(hipStreamSynchronize(p->last_stream));
    Counters c;
    HIP_OK(hipMemcpy(&c, p->d_counters, sizeof c, hipMemcpyDeviceToHost));
    if (plan_check_counters(c)) return -1;
    out->vertices = c.vertices;
    out->shadow_rays = c.shadow_rays;
    out->walk_steps = c.walk_steps;
    out->tiles_in_kernel = int32_t(c.tiles_summed);
    if (p->timed) {
      // mean over the launches since the previous read (at most the last kEvRing of them)
      unsigned long long first = p->stats_read_upto;
      if (p->launch_count - first > (unsigned long long)pine_gpu_plan::kEvRing) first = p->launch_count - pine_gpu_plan::kEvRing;
      if (first == p->launch_count) first = p->launch_count - 1;  // nothing new: report the last launch again
      // a plan with passes: every pass is a slot of the ring; the timings are those of ONE sequence -- the sum over its last
      // passes (at most kEvRing of them, scaled to the sequence's length when it has more)
      const unsigned long long np = (unsigned long long)p->pass_plan.n;
      if (np > 1) first = p->launch_count - std::min<unsigned long long>({np, p->launch_count, (unsigned long long)pine_gpu_plan::kEvRing});
      double a = 0, b = 0, c3 = 0;
      for (unsigned long long i = first; i < p->launch_count; i++) {
        const EventOwner* ev = p->ev[i % pine_gpu_plan::kEvRing];
        float x = 0, y = 0, z = 0;
        HIP_OK(hipEventElapsedTime(&x, ev[0].get(), ev[1].get()));
        HIP_OK(hipEventElapsedTime(&y, ev[1].get(), ev[2].get()));
        HIP_OK(hipEventElapsedTime(&z, ev[2].get(), ev[3].get()));
        a += x, b += y, c3 += z;
      }
      const double n = np > 1 ? double(p->launch_count - first) / double(np) : double(p->launch_count - first);
      out->prepass_ms = float(a / n);
      out->trace_ms = float(b / n);
      out->resolve_ms = float(c3 / n);
      out->timed_launches = np > 1 ? 1 : int32_t(p->launch_count - first);
      p->stats_read_upto = p->launch_count;
    }
  }
  return 0;
}

int pine_gpu_plan_debug_sections(pine_gpu_plan* p, uint64_t out[16]) {
  if (!p || !out) {
    set_error("null argument");
    return -1;
  }
  HIP_OK(hipSetDevice(p->device));
  HIP_OK(hipDeviceSynchronize());
  Counters c;
  HIP_OK(hipMemcpy(&c, p->d_counters, sizeof c, hipMemcpyDeviceToHost));
  for (int i = 0; i < 16; i++) out[i] = c.section_cycles[i];
#ifdef PINE_PROFILE_SECTIONS
  if (c.t_end > c.t_start && c.t_start)
    fprintf(stderr, "timeline: kernel %.2f ms, work-item pool dry after %.2f ms\n", double(c.t_end - c.t_start) * 1e-5,
            c.t_pool_dry ? double(c.t_pool_dry - c.t_start) * 1e-5 : -1.0);
  if (getenv("PINE_GPU_WG_TIMELINE") && c.t_start) {
    // per workgroup, ms after the launch's start: last whole-pixel item sealed | pool found dry | out | whole-pixel items it claimed
    for (int b = 0; b < p->grid && b < 1024; b++)
      fprintf(stderr, "wg %3d: whole-pixel items done %7.2f  pool dry %7.2f  out %7.2f  pixels %llu\n", b,
              c.wg_t[b][0] ? double(c.wg_t[b][0] - c.t_start) * 1e-5 : -1.0, c.wg_t[b][1] ? double(c.wg_t[b][1] - c.t_start) * 1e-5 : -1.0,
              c.wg_t[b][2] ? double(c.wg_t[b][2] - c.t_start) * 1e-5 : -1.0, c.wg_t[b][3]);
  }
  unsigned long long rl[16] = {0}, rh[16] = {0};
  {
    using RegFn = int (*)(unsigned long long*, unsigned long long*);
    static const RegFn regs[kPineKernelParts] = {pine_gpu_kernel_part_regions_0, pine_gpu_kernel_part_regions_1, pine_gpu_kernel_part_regions_2,
                                                 pine_gpu_kernel_part_regions_3, pine_gpu_kernel_part_regions_4, pine_gpu_kernel_part_regions_5,
                                                 pine_gpu_kernel_part_regions_6, pine_gpu_kernel_part_regions_7};
    for (RegFn f : regs)
      if (f(rl, rh)) return -1;
  }
  if (const hipModule_t own = p->scene_kernel.module()) {
    // the scene's own kernel (a module of its own) keeps its own copies of the REGION counters
    hipDeviceptr_t dl = nullptr, dh = nullptr;
    size_t bl = 0, bh = 0;
    if (hipModuleGetGlobal(&dl, &bl, own, "_ZN8pine_gpuL14g_region_lanesE") == hipSuccess &&
        hipModuleGetGlobal(&dh, &bh, own, "_ZN8pine_gpuL13g_region_hitsE") == hipSuccess && bl == sizeof rl && bh == sizeof rh) {
      unsigned long long ml[16], mh[16];
      if (hipMemcpy(ml, dl, sizeof ml, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(mh, dh, sizeof mh, hipMemcpyDeviceToHost) == hipSuccess)
        for (int i = 0; i < 16; i++) rl[i] += ml[i], rh[i] += mh[i];
    } else {
      (void)hipGetLastError();
    }
  }
  for (int i = 0; i < 16; i++)
    if (rh[i]) fprintf(stderr, "region %2d: entries %llu avg active lanes %.2f\n", i, rh[i], double(rl[i]) / double(rh[i]));
#endif
  return 0;
}

int64_t pine_gpu_plan_vertex_log(pine_gpu_plan* p, float* out, int64_t capacity) {
  if (!p) {
    set_error("null argument");
    return -1;
  }
  if (p->ao) {
    set_error("an AOIntegrator plan has no per-vertex log");
    return -1;
  }
  if (p->queue_variant < 0 || !(kQueueVariants[p->queue_variant].features & F_VLOG)) {
    set_error("the per-vertex log needs a plan created with PINE_GPU_FLAG_VERTEX_LOG (stage-queued kernel, the two variants compiled with the hook)");
    return -1;
  }
  if (p->pass_plan.n > 1) {
    set_error("the per-vertex log is not kept by a plan with passes");
    return -1;
  }
  const int64_t n = int64_t(p->film_w) * p->film_h * p->S.spp * p->S.max_path_length * kVertexLogFloats;
  if (n > (int64_t(1) << 27)) {
    set_error("the per-vertex log is meant for small films (at most 2^27 floats)");
    return -1;
  }
  HIP_OK(hipSetDevice(p->device));
  if (!out) {  // switch the log on: the NEXT launches fill it
    if (!p->d_vertex_log && p->d_vertex_log.alloc(size_t(n), "pine_gpu_plan_vertex_log")) return -1;
    HIP_OK(hipMemset(p->d_vertex_log, 0, size_t(n) * 4));
    p->W.vertex_log = p->d_vertex_log;
    return n;
  }
  if (!p->d_vertex_log || capacity < n) {
    set_error("vertex log not enabled, or capacity too small");
    return -1;
  }
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(out, p->d_vertex_log, size_t(n) * 4, hipMemcpyDeviceToHost));
  return n;
}

int pine_gpu_plan_read_samples(pine_gpu_plan* p, float* out, int64_t capacity) {
  if (!p || !out) {
    set_error("null argument");
    return -1;
  }
  if (p->ao) {
    set_error("an AOIntegrator plan keeps no per-sample rows (its film is a count per pixel)");
    return -1;
  }
  if (p->pass_plan.n > 1) {
    set_error("a plan with passes keeps the sample rows of one pass only: read_samples needs an ordinary plan");
    return -1;
  }
  const int spp = p->S.spp;
  const int64_t need = int64_t(p->film_w) * p->film_h * spp * 4;
  if (capacity < need) {
    set_error("capacity too small");
    return -1;
  }
  HIP_OK(hipSetDevice(p->device));
  HIP_OK(hipDeviceSynchronize());
  std::vector<float> tmp(size_t(p->W.num_local_tiles) * spp * 64 * 4);
  HIP_OK(hipMemcpy(tmp.data(), p->d_samples, tmp.size() * 4, hipMemcpyDeviceToHost));
  memset(out, 0, size_t(need) * 4);
  for (int lt = 0; lt < p->W.num_local_tiles; lt++) {
    int tile = plan_film_tile(p, lt);
    int tx = tile % p->W.tiles_x, ty = tile / p->W.tiles_x;
    for (int q = 0; q < 64; q++) {
      int px = tx * kTile + (q & 7), py = ty * kTile + (q >> 3);
      if (px >= p->film_w || py >= p->film_h) continue;
      for (int s = 0; s < spp; s++)
        memcpy(out + ((size_t(py) * p->film_w + px) * spp + s) * 4,
               tmp.data() + ((size_t(lt) * spp + s) * 64 + q) * 4, 16);
    }
  }
  return 0;
}

int pine_gpu_path_render_passes(pine_gpu_scene* scene, const pine_gpu_render_params* prm, int32_t pass_samples, float* film_out,
                                pine_gpu_pass_callback cb, void* user) {
  if (!scene || !prm || !film_out) {
    set_error("null argument");
    return -1;
  }
  pine_gpu_render_params prm2 = *prm;
  prm2.flags |= PINE_GPU_FLAG_PROGRESS;  // the reference's CLI polls get_progress() while render() runs (src/cli/pine.cpp:36-40)
  pine_gpu_plan* p = pine_gpu_plan_create_passes(scene, &prm2, pass_samples);
  if (!p) return -1;
  const int n = p->pass_plan.n;
  // get_progress() over the whole sequence: the items of the passes done + those the running pass has claimed
  unsigned long long total = 0;
  for (int j = 0; j < n; j++) total += pass_work(p, j).total_items;
  return one_shot_render(p, total, [&](float4* d_film, size_t bytes) {
    for (int j = 0; j < n; j++) {
      if (pine_gpu_plan_launch_pass(p, j, d_film, nullptr)) return -1;
      if (const hipError_t e = hipMemcpy(film_out, d_film, bytes, hipMemcpyDeviceToHost)) return hip_error("film download", e);
      if (pine_gpu_plan_check(p)) return -1;  // a bailed-out path kernel leaves an incomplete film: fail, do not return it as a result
      p->h_progress[0] = 0;  // (the pass has finished: nothing writes the word until the next launch)
      g_progress_base.fetch_add(pass_work(p, j).total_items);
      if (cb && cb(user, j, n, film_out) != 0) return PINE_GPU_RENDER_STOPPED;
    }
    return 0;
  });
}

int pine_gpu_path_render(pine_gpu_scene* scene, const pine_gpu_render_params* prm, float* film_out) {
  return pine_gpu_path_render_passes(scene, prm, 0, film_out, nullptr, nullptr);
}

/* One process, several devices: shard r of n (8x8-pixel tiles dealt round-robin) renders on devices[r];
 * every device writes its tiles into a packed slab, the slabs are copied device-to-device (peer copies over xGMI) into
 * one [rank][slab] buffer on devices[0], scattered into the row-major film there and downloaded.  Bit-identical to the
 * one-device film for any list (the same device may appear more than once).  This is what the C++ facade and the PRL
 * command line use to drive a whole node without torch.distributed. */
int pine_gpu_path_render_devices(pine_gpu_scene* scene, const pine_gpu_render_params* prm, const int* devices, int num_devices,
                                 float* film_out) {
  if (!scene || !prm || !devices || !film_out || num_devices < 1 || num_devices > 64) {
    set_error("bad argument");
    return -1;
  }
  if (num_devices == 1) {
    pine_gpu_render_params one = *prm;
    one.device = devices[0];
    one.shard_rank = 0;
    one.shard_world = 1;
    return pine_gpu_path_render(scene, &one, film_out);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error("no HIP device available: the PathIntegrator hot path requires an AMD GPU (no CPU fallback)");
    return -1;
  }
  for (int r = 0; r < num_devices; r++)
    if (devices[r] < 0 || devices[r] >= ndev) {
      set_error("device ordinal out of range");
      return -1;
    }
  int rc = -1;
  std::string keep;
  {
    // (destroyed in reverse: the plans first -- each waits for its stream, the slab copy on it included -- then slabs and streams)
    DeviceBuffer<char> gathered, d_film;
    std::vector<StreamOwner> streams(static_cast<size_t>(num_devices));
    std::vector<DeviceBuffer<char>> slabs(static_cast<size_t>(num_devices));
    std::vector<PlanOwner> plans(static_cast<size_t>(num_devices));
    rc = [&]() -> int {
      for (int r = 0; r < num_devices; r++) {
        pine_gpu_render_params p = *prm;
        p.device = devices[r];
        p.shard_rank = r;
        p.shard_world = num_devices;
        plans[size_t(r)].reset(pine_gpu_plan_create(scene, &p));
        if (!plans[size_t(r)]) return -1;
      }
      const int w = plans[0]->film_w, h = plans[0]->film_h;
      const int64_t slab_floats = pine_gpu_packed_slab_floats(w, h, num_devices);
      const size_t slab_bytes = size_t(slab_floats) * 4, film_bytes = size_t(w) * h * 16;
      if (const hipError_t e = hipSetDevice(devices[0])) return hip_error("device allocation", e);
      if (gathered.alloc(slab_bytes * size_t(num_devices), "device allocation") || d_film.alloc(film_bytes, "device allocation")) return -1;
      for (int r = 0; r < num_devices; r++) {
        if (const hipError_t e = hipSetDevice(devices[r])) return hip_error("per-device setup", e);
        if (create_stream(streams[size_t(r)], hipStreamNonBlocking, "per-device setup") || slabs[size_t(r)].alloc(slab_bytes, "per-device setup")) return -1;
        if (devices[r] != devices[0]) {
          int can = 0;
          (void)hipDeviceCanAccessPeer(&can, devices[r], devices[0]);
          if (can) (void)hipDeviceEnablePeerAccess(devices[0], 0);  // (already enabled is fine; without peer access the copy is staged)
          (void)hipGetLastError();
        }
      }
      // all devices render concurrently; each slab goes to devices[0] on the rendering device's own stream as soon as it is ready
      for (int r = 0; r < num_devices; r++) {
        char* dst = gathered + size_t(r) * slab_bytes;
        hipStream_t stream = streams[size_t(r)].get();
        if (pine_gpu_plan_launch_packed(plans[size_t(r)].get(), slabs[size_t(r)], stream)) {
          set_error(std::string("launch failed: ") + pine_gpu_last_error());
          return -1;
        }
        // (a peer copy between a device and itself is refused: "invalid device ordinal")
        const hipError_t e = devices[r] == devices[0] ? hipMemcpyAsync(dst, slabs[size_t(r)], slab_bytes, hipMemcpyDeviceToDevice, stream)
                                                      : hipMemcpyPeerAsync(dst, devices[0], slabs[size_t(r)], devices[r], slab_bytes, stream);
        if (e != hipSuccess) return hip_error("slab copy to the first device failed", e);
      }
      for (int r = 0; r < num_devices; r++)
        if (pine_gpu_plan_check(plans[size_t(r)].get())) return -1;  // waits for the stream, reports bail-outs
      if (pine_gpu_film_unpack(w, h, num_devices, devices[0], gathered, d_film, nullptr)) return -1;
      if (const hipError_t e = hipMemcpy(film_out, d_film, film_bytes, hipMemcpyDeviceToHost)) return hip_error("film download", e);
      return 0;
    }();
    if (rc) keep = pine_gpu_last_error();
  }
  (void)hipSetDevice(devices[0]);
  if (rc) set_error(keep);
  return rc;
}

/* SURVEY.md 8(b)'s form: bit d of device_mask selects HIP device d; shards are dealt to the selected devices in
 * ascending order. */
int pine_gpu_path_render_multi(pine_gpu_scene* scene, const pine_gpu_render_params* prm, uint64_t device_mask, float* film_out) {
  int list[64], n = 0;
  for (int d = 0; d < 64; d++)
    if (device_mask & (1ull << d)) list[n++] = d;
  if (n == 0) {
    set_error("empty device mask");
    return -1;
  }
  return pine_gpu_path_render_devices(scene, prm, list, n, film_out);
}
}  // extern "C"
