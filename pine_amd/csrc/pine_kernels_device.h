// pine_amd/csrc/pine_kernels_device.h -- the device side of the PathIntegrator hot path: types shared by host and
// kernels (DeviceScene, WorkParams, Counters, PackedState), the lane-owns-a-path kernel and -- through pine_trav.h /
// pine_queue_kernel.h -- the stage-queued kernel.  What a ray does in the BVHs is in pine_traverse.h.  What a path vertex computes (surface, emission, lobe
// choice, the BSSRDF walk, next-event estimation, fold) is written once, in pine_radiance.h; both kernels call it, and that
// is why their films are the same bits.  The kernel prologue (scene view, LDS staging, sampler slices) is there too.  Included by pine_kernels.hip (exact arithmetic: the parity build) and by
// pine_kernels_fast.hip (declared-tolerance arithmetic, under another namespace).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pine_device.h"

namespace pine_gpu {

constexpr int kBlock = 256;      // 4 waves per workgroup
constexpr int kTile = 8;         // 8x8 pixel tiles = 64 pixels = one wave's worth of items
#ifndef PINE_LDS_FOLD_LEVELS
#define PINE_LDS_FOLD_LEVELS 1
#endif
constexpr int kLdsFoldLevels = PINE_LDS_FOLD_LEVELS;  // fold-stack levels kept in LDS (deeper levels spill to global memory)
constexpr int kPoolItems = 128;  // items a wave claims from the global queue per atomic
constexpr int kMaxDepth = 32;    // max_path_length supported (2 beta bits per level in one u64)
// feature sets that several compiled variants share (pine_variants.h)
constexpr unsigned kFBoxes = F_AABB | F_OBB;
constexpr unsigned kFAnalytic = F_AABB | F_OBB | F_SPHERE | F_DISK | F_CONE | F_UBER;

// Diagnostic section timing: per-wave s_memtime deltas summed per section.  Never compiled into the
// product build; the stamps only go to Counters::section_cycles, which nothing else reads.
#ifdef PINE_PROFILE_SECTIONS
static __device__ unsigned long long g_region_lanes[16], g_region_hits[16];  // (one copy per translation unit: pine_kernels_part.hip reads its own)
// REGION(id): average number of active lanes at a code region's entry (divergence probe;
// -DPINE_PROFILE_REGIONS on top, as its global atomics distort the section times)
#ifndef PINE_PROFILE_REGIONS
#define REGION(id)
#else
#define REGION(id)                                                                  \
  do {                                                                              \
    const unsigned long long m_ = __ballot(1);                                      \
    if ((threadIdx.x & 63) == (unsigned)__ffsll((long long)m_) - 1) {               \
      atomicAdd(&g_region_lanes[id], (unsigned long long)__popcll(m_));             \
      atomicAdd(&g_region_hits[id], 1ull);                                          \
    }                                                                               \
  } while (0)
#endif
#define SEC_DECL unsigned long long sec_t = __builtin_readcyclecounter(), sec_acc[16] = {0}
#define SEC_MARK(id)                                              \
  do {                                                            \
    const unsigned long long t_ = __builtin_readcyclecounter();   \
    sec_acc[id] += t_ - sec_t;                                    \
    sec_t = t_;                                                   \
  } while (0)
#define SEC_FLUSH()                                                                     \
  do {                                                                                  \
    if ((threadIdx.x & 63) == 0)                                                        \
      for (int i_ = 0; i_ < 16; i_++) atomicAdd(&counters->section_cycles[i_], sec_acc[i_]); \
  } while (0)
#else
#define REGION(id)
#define SEC_DECL
#define SEC_MARK(id)
#define SEC_FLUSH()
#endif


struct DeviceScene {
  const DShape* shapes;
  const DMaterial* materials;
  const DNode* nodes;
  const float* env;  // ImageSky, Atmosphere: rotation, density tree, pdf table and texels / colours (pine_device.h EnvImage), or null; plan-owned
  const float* tex;  // image nodes: the u8 table, then every image the node programs read (pine_types.h N_IMAGE), or null; plan-owned
  const DBvh* bvhs;
  const float* tri_verts;
  const DLight* lights;
  const DNodeOp* node_ops;  // shading-node programs (F_NODES variants)
  const DShape* leaf;       // leaf[i] = the shape record of top-level primitive entry prims[i], see SceneView
  int num_lights;           // entries of `lights` (the light sampler's N)
  int env_light;            // index of the environment light in `lights`, or -1
  int num_shapes;
  DCamera cam;
  DTables tables;
  int spp;              // effective
  int max_path_length;
  int stack_top;        // traversal stack entries needed by the top-level BVH
  int stack_total;      // top + deepest mesh BVH
  // the small scene records packed in one 16-byte-aligned blob (for LDS staging):
  const uint4* blob;
  int blob_bytes;
  int off_nodes, off_shapes, off_materials, off_bvhs, off_prims, off_lights, off_node_ops, off_leaf;  // byte offsets in the blob
  int top_prim_begin;  // prims[top_prim_begin ..) are the top-level BVH's entries
  const float4* tri_leaf;  // mesh triangles in leaf order, 3 float4 per entry of `prims` (FlatAccel::tri_leaf)
  const float* tri_attrs;  // per-vertex normals / texcoords per triangle, 16 floats each (FlatAccel::tri_attrs), or null
  int lds_nodes;           // F_LDS_TOP variants: nodes[0 .. lds_nodes) are copied to LDS by every workgroup
  // F_LDS_TOP + F_MESH variants: the mesh triangles as LDS-sized packets (plan_build decides whether they are staged):
  // one 8-byte entry per leaf-ordered triangle (three 16-bit vertex numbers, the 16-bit triangle index) and the
  // scene's DISTINCT vertices as float4 -- the same floats as tri_leaf's 48-byte records, a third of the bytes
  const uint4* tri_packets;   // entries (tri_packet_entries x 8 bytes, padded to 16), then vertices (x 16 bytes)
  int tri_packet_entries, tri_packet_verts;
  int lds_tris;               // 1: every workgroup copies the packets to LDS and the traversal reads them there
  // PINE_GPU_FLAG_ORDER_EMBREE (F_EMBREE variants): the BVH8 the reference's EmbreeAccel walks over the non-mesh shapes
  // (pine_embree_order.h) -- EmbreeNode records at off_etree of the blob, the root's child word (kEmbreeNoChild: no such
  // shape) -- the places in `leaf` of the meshes (num_emesh ints at off_emesh; tested first) and the 2048 RCPPS estimates
  // (off_rcpps: BEHIND blob_bytes, global memory only)
  int off_etree, etree_root, off_emesh, num_emesh, off_rcpps;
  // The frame table (pine_device.h frame_entry), inside the staged part of the blob: the entries at off_frames
  // (0: the plan has no table) and, at off_frame_base, one word per shape -- its first entry, or -1 for a kind without faces.
  int off_frames, off_frame_base;
};

// (EmbreeNode, kEmbreeNoChild, kEmbreeStackEntries: pine_types.h)

// What the traversal and shading code reads.  In the F_LDS_SCENE specialisation every pointer is
// derived from the workgroup's LDS copy of the blob (so the loads are ds_read, ~64-cycle latency,
// instead of L1/L2 round trips); otherwise they point into HBM-backed global memory.
struct SceneView {
  // leaf[i]: a COPY of the shape record of top-level primitive entry i, in BVH leaf order, whose `kind`
  // field holds the packed primitive word (index | emissive | kind).  The leaf loop then needs one memory
  // round trip per primitive (record address = base + 128 i) instead of two dependent ones (word, then
  // shapes[word & mask]).  `leaf` is biased by -top_prim_begin so that the BVH's own indices address it.
  const DShape* leaf;
  const DShape* shapes;
  const DMaterial* materials;
  const DNode* nodes;
  const float* env;  // DeviceScene::env (global memory, never staged)
  const float* tex;  // DeviceScene::tex (global memory, never staged)
  const DBvh* bvhs;
  const DLight* lights;
  const float* tri_verts;
  const DNodeOp* node_ops;
  int stack_top;
  int num_shapes;
  const float4* tri_leaf;
  const float* tri_attrs;
  const DNode* lds_nodes;  // F_LDS_TOP: the workgroup's LDS copy of nodes[0 .. lds_node_count)
  int lds_node_count;
  const uint2* lds_tri_entries;   // DeviceScene::tri_packets in LDS (null: triangles are read from tri_leaf)
  const float4* lds_tri_verts;
  // F_EMBREE variants (PINE_GPU_FLAG_ORDER_EMBREE): DeviceScene::off_etree / etree_root / off_emesh / off_rcpps
  const EmbreeNode* etree;
  int etree_root;
  const int* emesh;
  int num_emesh;
  const unsigned* rcpps;
  const float* frames;    // DeviceScene::off_frames / off_frame_base; read only where has_frames
  const int* frame_base;
  int has_frames;
};


struct WorkParams {
  int tiles_x, tiles_y;
  int num_local_tiles;   // tiles owned by this shard
  int shard_rank, shard_world;
  int samples_per_item;  // k
  int items_per_pixel;   // spp / k (a power of two)
  int log2_items_per_pixel;
  unsigned tiles_x_magic;  // ceil(2^32 / tiles_x): see decode_item
  unsigned long long total_items;  // num_local_tiles * items_per_pixel * 64 (tile classes: see serial_tiles)
  // Tile classes (Subsurface variants of the stage-queued kernel, plan_build): a scene whose materials draw from the
  // pixel's RNG inside radiance() makes a pixel's samples sequentially dependent (one item = the whole pixel) -- but only
  // in pixels whose camera rays can reach such a material.  The host lists the shard's tiles in `tile_order`, those
  // that can first (`serial_tiles` of them, items [0, serial_tiles * 64): one per pixel, all spp samples); the others
  // follow as independent items of samples_per_item samples with RNG checkpoints, like a scene without in-path draws.
  // serial_tiles == 0: one class, as described by samples_per_item / items_per_pixel.
  const int* tile_order;  // local tile -> tile of the film, or null (local tile * shard_world + shard_rank)
  int serial_tiles;
  unsigned long long idle_budget_ticks;  // stage-queued kernel: a wave that finds no work for this long (100 MHz wall clock) bails out
  int debug_force_bail;  // test hook (PINE_GPU_FLAG_DEBUG_FORCE_BAIL): the first wave bails out at once
  int trav_min_lanes, trav_min_trips;  // traversal stages (pine_queue_kernel.h): retire / refill when fewer lanes than this still travel, at the earliest after this many trips
  int fair_period;  // stage-queued kernel, variants with more than two stage queues: every this-many-th pick of a wave serves the shortest non-empty queue (0: never)
  int pick_spins;   // stage-queued kernel: idle polls after which a wave takes a queue's entries although they are fewer than 64
  int pool_items;   // stage-queued kernel: work items a workgroup claims from the global counter at a time
  int max_pixels;   // Subsurface variants: pixels a workgroup has in flight at most
  int fork_sealed;  // Subsurface variants: a path that can make no further RNG draw hands its pixel's next sample to another context
  unsigned long long* progress;  // host-mapped word (or null): work items claimed so far, stored now and then (get_progress)
  // Test hook (pine_gpu_plan_vertex_log; null in every ordinary launch): 16 floats per radiance() invocation at
  // [((py * film_w + px) * spp + sample) * max_path_length + level] -- the layout of `pine_ref vertices` (oracle/ref_driver.cpp):
  // kind | length | direct term (3) | bs.f (3) | cosine | bs.pdf | is_delta | mis | returned light pdf (-1: none) | returned Lo (3)
  float* vertex_log;
  // The pass window (plans created with passes; an ordinary launch: the whole render).  A launch hands out the
  // whole-pixel items of `serial_tiles` tiles (local tiles pass_first_serial_tile ...) and, for every tile of the independent
  // class (local tiles free_tile_base ...), the chunks [pass_first_chunk, pass_first_chunk + pass_chunks) of each pixel.
  // Read by decode_item only: cold, like the rest of the work decomposition.
  int pass_first_chunk;
  int pass_chunks;             // ordinary launch: items_per_pixel
  unsigned pass_chunks_magic;  // ceil(2^32 / pass_chunks)
  int pass_row_stride;         // sample rows a tile of the independent class has in the sample buffer (ordinary launch: spp)
  int free_tile_base;          // ordinary launch: serial_tiles
  int pass_first_serial_tile;  // ordinary launch: 0
  // Owned tiles (stage-queued kernel, plain variants, plans of one pass): the first `owned_tiles` local tiles are
  // claimed one whole tile per claim, so that every sample row of such a tile is written by waves of one workgroup, and the wave
  // that retires the tile's last item sums it (resolve_tile below) instead of resolve_kernel.  The claim counter keeps counting
  // in units of pool_items = 1 << pool_items_log2: claim number c < owned_tiles is local tile c, the later ones are the usual
  // runs of pool_items items behind the owned tiles.  0: every claim is pool_items items, every tile is summed by resolve_kernel.
  int owned_tiles;
  int pool_items_log2;
  int tile_slots;         // slots of a workgroup's table of owned tiles in flight (kQTileSlots; fewer: a test knob)
  int film_packed;        // the launch writes this rank's tile-major slab (ResolvePass::packed)
  float4* film;           // the launch's film or slab
  unsigned* tile_done;    // per local tile: summed inside the path kernel (cleared with the counters); null without owned tiles
};
constexpr int kVertexLogFloats = 16;
// get_progress() (integrator.cpp:17-19): every 16th / 64th pool claim posts the claimed-item count to host memory
__device__ __forceinline__ void post_progress(const WorkParams& W, unsigned long long claimed, unsigned shift) {
  if (W.progress && ((claimed >> shift) & 15ull) == 0ull)
    __hip_atomic_store(W.progress, claimed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace pine_gpu
#include "pine_traverse.h"  // BVH traversal: the nested walks, EmbreeAccel's order, the steps every walk shares
namespace pine_gpu {

// ------------------------------------------------------------------------------------------------
// Item <-> pixel mapping.  Items are ordered [local tile][chunk][pixel in tile] so that the 64
// consecutive items a fresh wave pulls are one 8x8 tile at one sample range: coherent rays,
// contiguous sampler-tile bytes, contiguous sample-buffer rows.
// ------------------------------------------------------------------------------------------------
struct ItemInfo {
  int px, py;
  int chunk;
  unsigned long long sample_base;  // index of sample 0 of this pixel row in the samples buffer / 64-strided
  unsigned long long ckpt_index;   // the item's RNG checkpoint (items of the independent class)
  bool serial;                     // an item of the whole-pixel class of a launch with tile classes
  bool valid;
};
__device__ __forceinline__ int film_tile_of(const WorkParams& W, int ltile) {
  return W.tile_order ? W.tile_order[ltile] : ltile * W.shard_world + W.shard_rank;
}
__device__ __forceinline__ ItemInfo decode_item(const WorkParams& W, int film_w, int film_h, int spp,
                                                unsigned long long item) {
  ItemInfo it;
  const unsigned long long serial_items = (unsigned long long)W.serial_tiles * 64ull;
  it.serial = item < serial_items;
  const unsigned long long rel = it.serial ? item : item - serial_items;
  const int p = int(rel & 63);
  const unsigned long long tc = rel >> 6;
  // (tile of the class, chunk of the pass) = tc / pass_chunks and the remainder: the chunks of a pass need not be a power of
  // two, so -- as for tiles_x below -- a multiplication with the rounded-up reciprocal and one fix-up step instead of a
  // 64-bit division (this runs once per work item; tc < 2^26: a launch has fewer than 2^32 sample rows)
  unsigned q = unsigned(tc), chunk = 0;
  if (!it.serial && W.pass_chunks != 1) {
    q = unsigned((uint64_t(unsigned(tc)) * W.pass_chunks_magic) >> 32);
    if (q * unsigned(W.pass_chunks) > unsigned(tc)) q--;
    chunk = unsigned(tc) - q * unsigned(W.pass_chunks);
  }
  if (!it.serial) chunk += unsigned(W.pass_first_chunk);
  const int ltile = (it.serial ? W.pass_first_serial_tile : W.free_tile_base) + int(q);
  const int tile = film_tile_of(W, ltile);
  it.ckpt_index = rel;
  // tile / tiles_x by multiplication with the rounded-up reciprocal + one fix-up step (exact for any
  // 32-bit tile: the estimate is never more than one too large)
  unsigned ty = unsigned((uint64_t(unsigned(tile)) * W.tiles_x_magic) >> 32);
  if (ty * unsigned(W.tiles_x) > unsigned(tile)) ty--;
  if (W.tiles_x == 1) ty = unsigned(tile);  // (2^32 / 1 does not fit the 32-bit magic)
  const int tx = tile - int(ty) * W.tiles_x;
  it.px = tx * kTile + (p & 7);
  it.py = ty * kTile + (p >> 3);
  it.chunk = int(chunk);
  // The sample buffer of a launch: [whole-pixel tile of the launch][spp rows], then [independent tile][pass_row_stride rows].
  // The kernels store sample s at sample_base + s * 64 with the ABSOLUTE s, and the host hands them the buffer's address
  // less the rows before the pass's first sample: a sample lands in its pass-relative row, a whole-pixel item (all of whose
  // samples are in the launch) gets those rows added here.  An ordinary launch: local tile * spp * 64 + p, no offset.
  const unsigned long long first_row = (unsigned long long)(unsigned(W.pass_first_chunk) * unsigned(W.samples_per_item));
  it.sample_base = it.serial ? ((unsigned long long)q * (unsigned)spp + first_row) * 64ull + (unsigned)p
                             : ((unsigned long long)W.serial_tiles * (unsigned)spp + (unsigned long long)q * (unsigned)W.pass_row_stride) * 64ull + (unsigned)p;
  it.valid = it.px < film_w && it.py < film_h;
  return it;
}

// RNG state at the start of every item: the reference reseeds per pixel (sampler.h:286-290) and
// then draws 4 floats per camera sample (path.cpp:35); when nothing inside radiance() touches the
// RNG the state at sample s is the seed advanced 4*s steps.
// A plan with passes (`carry` not null): the walk is CARRIED from pass to pass -- 16 bytes per pixel of the class, the state
// at the pass's first sample, read here (seeded in the pass that starts at sample 0) and left for the next pass.
static __global__ void __launch_bounds__(kBlock) rng_checkpoint_kernel(WorkParams W, int film_w, int film_h, int spp,
                                                               ulonglong2* ckpt, int free_tiles, ulonglong2* carry) {
  // one thread per (local tile of the independent class, pixel in tile); walks the pixel's samples of the launch, storing at chunk starts
  const unsigned long long t = blockIdx.x * (unsigned long long)kBlock + threadIdx.x;
  const unsigned long long n = (unsigned long long)free_tiles * 64ull;
  if (t >= n) return;
  const int p = int(t & 63);
  const int ptile = int(t >> 6);  // (position among the independent tiles: ItemInfo::ckpt_index counts from there)
  const int tile = film_tile_of(W, W.free_tile_base + ptile);
  const int px = (tile % W.tiles_x) * kTile + (p & 7), py = (tile / W.tiles_x) * kTile + (p >> 3);
  DRng g = rng_seed(hash_pixel(px, py, 0));
  if (carry && W.pass_first_chunk != 0) {
    const ulonglong2 c = carry[t];
    g = DRng{c.x, c.y};
  }
  for (int c = 0; c < W.pass_chunks; c++) {
    const unsigned long long item = ((unsigned long long)ptile * W.pass_chunks + c) * 64ull + p;
    ckpt[item] = make_ulonglong2(g.s0, g.s1);
    for (int i = 0; i < 4 * W.samples_per_item; i++) rng_next64(g);
  }
  if (carry) carry[t] = make_ulonglong2(g.s0, g.s1);
  (void)film_w, (void)film_h, (void)spp;
}

// ------------------------------------------------------------------------------------------------
// Ordered per-pixel sum of one tile: film[p] = (sum_{s=0..spp-1, in order} L_s) / spp  (path.cpp:34-38).
// One wave per tile, lane = pixel in tile: every sample row is one coalesced 1 KiB read.  Called by resolve_kernel
// (pine_kernels.hip) and, for the tiles a workgroup owns, by the stage-queued path kernel itself: one text, the same bits.
// `packed` != 0: the output is this rank's tile-major slab [local tile][pixel in tile] (multi-GPU gather)
// instead of the row-major film.
//
// The sum is CONTINUED from pass to pass: `sum` holds one float4 per local pixel,
// (((L_0 + L_1) + ...) + L_{m-1}) of the samples resolved so far -- the partial result of the loop below, so going on from it
// rounds exactly as one launch over all rows does.  Tiles of the whole-pixel class ([0, whole_tiles) in the plan's tile order)
// get all spp rows in the pass that renders their slice and none in the others: their film pixel is final from then on and
// (0, 0, 0, 0) before.  Tiles of the independent class get `free_rows` rows in every pass; their film pixel is the running
// mean sum / samples_so_far -- after the last pass sum / spp.  A plan of one pass: the slice is the whole class, free_rows =
// samples_so_far = spp, and `sum` is null -- nothing carried, nothing kept.  W is the PLAN's work decomposition.
// ------------------------------------------------------------------------------------------------
struct ResolvePass {
  int film_w, film_h, spp;
  int whole_tiles, slice_first, slice_tiles;  // the whole-pixel class; the slice of it this pass rendered
  int free_rows;                               // sample rows of this pass per tile of the independent class
  int first_pass;                              // ... and whether they are the pixel's first (the sum starts from zero)
  int samples_so_far;                          // ... and the samples of a pixel of that class up to and including this pass
  int packed;
};
// Returns the lane's radiance() invocation count (the .w of its rows).  ROWS sample rows are in flight per lane.
template <int ROWS>
__device__ __forceinline__ unsigned long long resolve_tile(const WorkParams& W, const ResolvePass& R, const float4* samples, float4* sum,
                                                           float4* film, int ltile, int p) {
  const int tile = film_tile_of(W, ltile);
  const int px = (tile % W.tiles_x) * kTile + (p & 7), py = (tile / W.tiles_x) * kTile + (p >> 3);
  const bool inside = px < R.film_w && py < R.film_h;
  const float4* row = nullptr;
  int rows = 0;
  bool carried = false, shown = true;
  float divisor = float(R.spp);
  if (ltile < R.whole_tiles) {
    if (ltile >= R.slice_first && ltile < R.slice_first + R.slice_tiles) {
      row = samples + (unsigned long long)(ltile - R.slice_first) * (unsigned)R.spp * 64ull + p;
      rows = R.spp;
    } else if (ltile < R.slice_first) {
      carried = true;  // an earlier pass finished it
    } else {
      shown = false;
    }
  } else {
    row = samples + ((unsigned long long)R.slice_tiles * (unsigned)R.spp + (unsigned long long)(ltile - R.whole_tiles) * (unsigned)R.free_rows) * 64ull + p;
    rows = R.free_rows;
    carried = !R.first_pass;
    divisor = float(R.samples_so_far);
  }
  if (!inside) rows = 0;
  float4* const acc = sum && inside ? sum + (unsigned long long)ltile * 64ull + p : nullptr;
  f3 L = mk3(0.0f);
  if (carried && acc) {
    const float4 a = *acc;
    L = f3{a.x, a.y, a.z};
  }
  unsigned long long verts = 0;
  // the sum is sequential in s (path.cpp:34-37), the loads need not be: ROWS rows in flight per lane
  int s = 0;
  for (; s + ROWS <= rows; s += ROWS) {
    float4 v[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; j++) v[j] = row[(unsigned long long)(s + j) * 64ull];
#pragma unroll
    for (int j = 0; j < ROWS; j++) {
      L = L + f3{v[j].x, v[j].y, v[j].z};
      verts += (unsigned long long)v[j].w;
    }
  }
  for (; s < rows; s++) {
    const float4 v = row[(unsigned long long)s * 64ull];
    L = L + f3{v.x, v.y, v.z};
    verts += (unsigned long long)v.w;
  }
  if (inside) {
    if (acc && rows > 0) *acc = make_float4(L.x, L.y, L.z, 0.0f);
    const f3 m = L / divisor;
    // (the slab is tile-major in the shard's NATURAL tile order, whatever order the launch works in: tile_order)
    const size_t out_index = R.packed ? size_t(tile / W.shard_world) * 64u + size_t(p) : size_t(py) * R.film_w + px;
    film[out_index] = shown ? make_float4(m.x, m.y, m.z, 1.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  return verts;
}

// ------------------------------------------------------------------------------------------------
// The path kernel
// ------------------------------------------------------------------------------------------------
struct Counters {
  unsigned long long next_item;
  unsigned long long vertices;
  unsigned long long shadow_rays;
  // protocol failure of the stage-queued kernel (a bounded spin or the idle budget ran out): number of
  // bail-outs of the launch, and the code / operands of one of them.  Read by every host entry point
  // that synchronises (plan_check): a launch with bail_count != 0 has an incomplete film and FAILS.
  unsigned long long bail_count;
  unsigned long long bail_code, bail_a, bail_b;
  unsigned long long walk_steps;  // BSSRDF random-walk steps (stage-queued kernel, F_SSS variants)
  unsigned long long tiles_summed;  // owned tiles the path kernel summed itself (WorkParams::owned_tiles)
  unsigned long long section_cycles[16];  // diagnostic builds (-DPINE_PROFILE_SECTIONS) only
  unsigned long long t_start, t_pool_dry, t_end;  // ... 100 MHz wall clock: first workgroup in, the work-item pool found empty, last workgroup out
#ifdef PINE_PROFILE_SECTIONS
  unsigned long long wg_t[1024][4];  // per workgroup: its last whole-pixel item sealed | pool found dry | out | whole-pixel items claimed
#endif
};



__device__ __forceinline__ f3 material_le(const DMaterial* m, f3 n, f3 wo) {  // material.h:22-25
  if (m->kind != MAT_EMISSIVE) return mk3(0.0f);
  if (dot(wo, n) < 0.0f) return mk3(0.0f);
  return ld3(m->color);
}

// LDS layout of the path kernel (dword offsets; everything per-lane is [slot][thread], so a wave's
// accesses are bank-conflict free and one VGPR (thread id) + an immediate offset addresses all of it):
//   fold level(s)   kLdsFoldLevels * 8 x 256      FoldEntry fields of the shallowest level(s)
//   sampler slices  12 x 256                      40 ranking + 8 scrambling bytes of the lane's pixel
//   RNG state       4 x 256                       per-pixel xoroshiro state (only touched at sample start)
//   Sobol rows      40 x 256 bytes                transposed table, dimensions < 40
//   traversal stack stack_total x 256             (runtime depth)
//   scene blob      blob_bytes                    nodes | shapes | materials | bvhs | prims | lights | frame table
constexpr int kOffFold = 0;
constexpr int kOffTile = kLdsFoldLevels * 8 * kBlock;
constexpr int kOffRng = kOffTile + kLdsTileDwords * kBlock;
constexpr int kOffSobol = kOffRng + 4 * kBlock;
constexpr int kOffStack = kOffSobol + kLdsSamplerDims * 256 / 4;
constexpr size_t kLdsFixedBytes = size_t(kOffStack) * 4;

// Packed per-lane path bookkeeping (one VGPR):
//   bits 0-11 sample index within the pixel (BlueSobolSampler::index / the low part of SobolSampler's index),
//   12-20 sampler dimension, 21-26 Vertex::length, 27 Vertex::diffuse_length > 0 (all the path reads of it,
//   path.cpp:93), 28 Vertex::is_delta, 29-30 the stage-queued kernel's BSSRDF walk status of the vertex being shaded
//   (kWalk*), 31 "sealed" (stage-queued kernel, Subsurface variants: the path has released its pixel's sample token, see
//   pine_queue_kernel.h).  0xffffffff marks an empty context (a length of 63 cannot occur: kMaxDepth is 32).
constexpr int kMaxDeviceSpp = 4096;      // 12 bits of sample index
constexpr int kMaxSamplerDimension = 511;  // 9 bits: BlueSampler wraps at 256; SobolSampler counts up to 8 draws per vertex
enum : unsigned { kWalkNone = 0, kWalkRunning = 1, kWalkExited = 2, kWalkFailed = 3 };
struct PackedState {
  unsigned v;
  __device__ __forceinline__ unsigned walk() const { return (v >> 29) & 3u; }
  __device__ __forceinline__ void set_walk(unsigned w) { v = (v & ~(3u << 29)) | (w << 29); }
  __device__ __forceinline__ int s_cur() const { return int(v & 0xfffu); }
  __device__ __forceinline__ int dim() const { return int((v >> 12) & 0x1ffu); }
  __device__ __forceinline__ int length() const { return int((v >> 21) & 0x3fu); }
  __device__ __forceinline__ int diffuse_length() const { return int((v >> 27) & 1u); }  // 0 or "at least 1"
  __device__ __forceinline__ bool is_delta() const { return (v >> 28) & 1u; }
  __device__ __forceinline__ void set_dim(int d) { v = (v & ~(0x1ffu << 12)) | (unsigned(d) << 12); }
  __device__ __forceinline__ void start_sample(int s) { v = unsigned(s) | (1u << 28); }  // dim 0, first_vertex()
  __device__ __forceinline__ void next_vertex(bool delta) {  // Vertex(pv, pdf, is_delta) path.cpp:18-19
    v = (v & 0x801fffffu) + ((unsigned(length()) + 1u) << 21) + (((v >> 27) & 1u) | (delta ? 0u : 1u)) * (1u << 27) +
        (delta ? (1u << 28) : 0u);
  }
  __device__ __forceinline__ bool sealed() const { return (v >> 31) != 0u; }
  __device__ __forceinline__ void set_sealed() { v |= 0x80000000u; }
};

}  // namespace pine_gpu
#include "pine_radiance.h"  // the kernel prologue and the per-vertex steps of radiance(): every kernel runs these
namespace pine_gpu {

template <unsigned F, int WAVES_PER_SIMD>
__global__ void __launch_bounds__(kBlock, WAVES_PER_SIMD)
path_trace_kernel(DeviceScene S, WorkParams W, const ulonglong2* __restrict__ ckpt, float4* __restrict__ samples,
                  float* __restrict__ fold, Counters* __restrict__ counters) {
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  constexpr int kSM = kSmLds | ((F & F_SOBOL) ? kSmSobol : 0);  // sampler front mode (pine_device.h)
  const unsigned tid = threadIdx.x;
  float* const lds_f = reinterpret_cast<float*>(lds_raw);
  uint32_t* const lds_u = reinterpret_cast<uint32_t*>(lds_raw);
  int* const stack = lds_raw + kOffStack + tid;
  stage_sobol_rows(lds_raw + kOffSobol, S.tables, tid, kBlock);
  const DTables T = lane_tables(S.tables, lds_raw + kOffSobol, lds_u + kOffTile, tid);
  SceneView V;
  if constexpr (F & F_LDS_SCENE) V = scene_view_staged(S, reinterpret_cast<uint4*>(lds_raw + kOffStack + S.stack_total * kBlock), tid, kBlock);
  else V = scene_view_global(S);
  __syncthreads();  // Sobol rows (and the scene) staged above
  // Global part of the fold stack: lane-major, one 32-byte entry (two float4) per level, so the
  // bytes a lane touches are only the levels its paths really reach -- the hot set (~2.6 levels x
  // 32 B x resident lanes ~ 22 MB chip-wide, 2.7 MB per XCD) stays in the XCD's 4 MB L2, whereas a
  // [level][field][lane] layout touches all levels of all lanes (58 MB) and thrashes it.
  auto fold_entry = [&](int level) -> float4* {
    return reinterpret_cast<float4*>(fold) + (size_t(blockIdx.x * kBlock + tid) * size_t(S.max_path_length) + size_t(level)) * 2;
  };
  auto fold_store = [&](int level, const float (&e)[8]) {
    if (level < kLdsFoldLevels) {
#pragma unroll
      for (int i = 0; i < 8; i++) lds_f[kOffFold + (level * 8 + i) * kBlock + tid] = e[i];
    } else {
      float4* q = fold_entry(level);
      q[0] = make_float4(e[0], e[1], e[2], e[3]);
      q[1] = make_float4(e[4], e[5], e[6], e[7]);
    }
  };
  auto fold_load = [&](int level, float (&e)[8]) {
    if (level < kLdsFoldLevels) {
#pragma unroll
      for (int i = 0; i < 8; i++) e[i] = lds_f[kOffFold + (level * 8 + i) * kBlock + tid];
    } else {
      const float4* q = fold_entry(level);
      const float4 a = q[0], b = q[1];
      e[0] = a.x, e[1] = a.y, e[2] = a.z, e[3] = a.w, e[4] = b.x, e[5] = b.y, e[6] = b.z, e[7] = b.w;
    }
  };
  // the per-pixel RNG lives in LDS: it is only touched when a sample starts (4 draws, path.cpp:35)
  // and by the few material branches that draw from it inside radiance()
  auto rng_load = [&]() -> DRng {
    const uint32_t a = lds_u[kOffRng + tid], b = lds_u[kOffRng + kBlock + tid], c = lds_u[kOffRng + 2 * kBlock + tid],
                   d = lds_u[kOffRng + 3 * kBlock + tid];
    return DRng{uint64_t(a) | (uint64_t(b) << 32), uint64_t(c) | (uint64_t(d) << 32)};
  };
  auto rng_store = [&](const DRng& g) {
    lds_u[kOffRng + tid] = uint32_t(g.s0);
    lds_u[kOffRng + kBlock + tid] = uint32_t(g.s0 >> 32);
    lds_u[kOffRng + 2 * kBlock + tid] = uint32_t(g.s1);
    lds_u[kOffRng + 3 * kBlock + tid] = uint32_t(g.s1 >> 32);
  };

  // ---- lane state (kept small on purpose: the kernel sits at the 128-VGPR / 4-waves-per-SIMD edge) ----
  bool lane_done = false;  // queue exhausted for this lane
  bool have_item = false;
  bool alive = false;      // a path is in flight
  f3 ray_o = mk3(0.0f), ray_d = mk3(0.0f);
  float ray_tmax = 0.0f;   // every ray on this path has tmin == 0
  unsigned pxy = 0;        // px | py << 16
  unsigned sample_base = 0;
  PackedState st{0};
  unsigned shadow_count = 0;
  unsigned long long beta_flags = 0;  // 2 bits per level (BSSRDF beta channel); dead code without F_SSS
  constexpr bool kBigDim = big_sampler_dimension<F>();  // the sampler's dimension counter in a register of its own
  int big_dim = 0;
  (void)big_dim;
  // wave-uniform private item pool [pool_next, pool_end)
  unsigned long long pool_next = 0, pool_end = 0;
  bool queue_empty = false;
  const int kspi = W.samples_per_item;

  SEC_DECL;
  while (true) {
    SEC_MARK(0);  // loop overhead
    // ---------------- regeneration ----------------
    // Lanes whose item is exhausted take the next items of the wave's private pool (a range of
    // kPoolItems consecutive items claimed from the global queue with ONE atomic by one lane);
    // ranks inside the wave come from a ballot prefix count, so there is no per-lane atomic.
    // (A per-iteration wave-aggregated atomic on one word saturates at ~90 M dequeues/s chip-wide,
    // MI355X_MICROARCH.md "dequeue" -- that was the first bottleneck measured.)
    {
      bool need_item = !alive && !lane_done && !have_item;
      while (true) {
        const unsigned long long mask = __ballot(need_item);
        if (mask == 0) break;
        if (pool_next == pool_end) {
          if (queue_empty) {
            if (need_item) lane_done = true;
            break;
          }
          unsigned long long base = 0;
          if ((tid & 63) == 0) base = atomicAdd(&counters->next_item, (unsigned long long)kPoolItems);
          base = __shfl(base, 0);
          if (base >= W.total_items) {
            queue_empty = true;
          } else {
            if ((tid & 63) == 0) post_progress(W, base, 9);
            pool_next = base;
            pool_end = base + kPoolItems < W.total_items ? base + kPoolItems : W.total_items;
          }
          continue;
        }
        const unsigned lane = tid & 63;
        const unsigned rank = __popcll(mask & ((1ull << lane) - 1ull));
        const unsigned long long avail = pool_end - pool_next;
        const unsigned want = __popcll(mask);
        const unsigned take = want < avail ? want : unsigned(avail);
        if (need_item && rank < take) {
          const unsigned long long item = pool_next + rank;
          need_item = false;
          const ItemInfo it = decode_item(W, S.cam.W, S.cam.H, S.spp, item);
          if (it.valid) {
            have_item = true;
            pxy = unsigned(it.px) | (unsigned(it.py) << 16);
            st.start_sample(it.chunk * kspi);
            sample_base = unsigned(it.sample_base);
            load_lane_slice(S.tables, it.px, it.py, lds_u + kOffTile, tid);
            if (W.items_per_pixel == 1) {
              rng_store(rng_seed(hash_pixel(it.px, it.py, 0)));  // Sampler::start_pixel
            } else {
              const ulonglong2 c = ckpt[it.ckpt_index];
              rng_store(DRng{c.x, c.y});
            }
          }  // else: pixel outside the film (partial border tile): ask again next trip
        }
        pool_next += take;
      }
      if (!alive && !lane_done && have_item) {
        REGION(0);  // camera ray generation
        // start sample s_cur: BlueSobolSampler index = s, dimension = 0 (sampler.h:174-181)
        st.start_sample(st.s_cur());
        if constexpr (F & F_SOBOL)
          if (S.tables.kind == 2) st.set_dim(2);  // HaltonSampler::start_pixel / start_next_sample: dimension = 2
        if constexpr (kBigDim) big_dim = S.tables.kind == 2 ? 2 : 0;
        const int px = int(pxy & 0xffffu), py = int(pxy >> 16);
        DRng g = rng_load();
        const DRay r = camera_sample(S.cam, px, py, g);
        rng_store(g);
        ray_o = r.o;
        ray_d = r.d;
        ray_tmax = r.tmax;
        if constexpr (F & F_SSS) beta_flags = 0;
        alive = true;
      }
    }
    SEC_MARK(1);  // regeneration
    if (__all(lane_done && !alive)) break;
    if (!alive) continue;

    // ---------------- one radiance() invocation (path.cpp:42-124) ----------------
    DSampler sampler = sampler_of<F>(st, pxy, S.tables.kind, [&] { return big_dim; });
    const int pv_length = st.length();
    int geom = -1, prim = 0;
    bool hit;
    {
      DRay ray{ray_o, ray_d, 0.0f, ray_tmax};
      hit = scene_traverse<false, F>(V, ray, stack, geom, prim);
      if (hit) geom &= kPrimIndexMask;  // (the packed word's flag bits are used by the queue kernel only)
      ray_tmax = ray.tmax;
    }
    SEC_MARK(2);  // closest-hit traversal

    // terminal result of this vertex, if it terminates
    bool terminal = false;
    f3 Lo = mk3(0.0f);
    bool has_light_pdf = false;
    float light_pdf = 0.0f;

    DSurface it{};
    const DShape* shape = nullptr;
    const DMaterial* mat = nullptr;
    int frame = -1;  // (hit_surface: the hit's entry of the frame table)
    if (!hit) {
      terminal = true;
      Lo = terminal_radiance<F>(V, S.env_light, S.num_lights, false, shape, it, ray_o, ray_d, ray_tmax, st.is_delta(), has_light_pdf, light_pdf);
    } else {
      REGION(3);  // surface info
      shape = &V.shapes[geom];
      mat = &V.materials[shape->material];
      frame = hit_surface<F>(V, shape, prim, ray_o, ray_d, ray_tmax, it);
      if (mat->kind == MAT_EMISSIVE) {
        Lo = terminal_radiance<F>(V, S.env_light, S.num_lights, true, shape, it, ray_o, ray_d, ray_tmax, st.is_delta(), has_light_pdf, light_pdf);
        terminal = true;
      } else if (pv_length + 1 >= S.max_path_length) {  // path.cpp:89
        terminal = true;
      }
    }

    SEC_MARK(3);  // surface info + emissive/terminal test
    if (!terminal) {
      REGION(6);  // non-terminal shading
      const f3 wi = -ray_d;
      m3 l2w = surface_frame(V, frame, it.n);
      m3 w2l = transpose(l2w);
      const MatParams mp = material_params<F>(mat, V.node_ops, V.tex, it.p, it.n, it.uv);
      DBxdf bx;
      choose_lobe<F, kSM>(mat, mp, wi, it.n, st.diffuse_length() > 0, false, rng_load, rng_store, T, sampler, bx);
      bx.wi = mul(w2l, wi);  // material.h:119

      // ---- BSSRDF random walk inside the same shape (bxdf.cpp:329-353, :375-382) ----
      int beta_channel = 0;
      bool do_walk = false;
      if constexpr (F & F_SSS) do_walk = bx.kind == BX_BSSRDF;
      int channel = 0;
      DRay wr{};
      if (do_walk && walk_begin(wi, it, bx, rng_load, rng_store, channel, wr)) {
        auto inside = [&](DRay& r, int& wprim) -> bool {
          bool walk_mesh = false;
          if constexpr (F & F_MESH) walk_mesh = shape->kind == SHAPE_MESH;
          if (walk_mesh) return mesh_traverse<false>(V, V.bvhs[as_int(shape->f[2])], r, make_oct(r), stack, 0, wprim);
          return shape_intersect<F>(shape, r);
        };
        for (;;) {  // (ends without an exit when a ray finds no surface: sample_p returns nullopt, nothing changes)
          DRay next;
          DSurface sit;
          const unsigned status = walk_step<F, kSM>(V, shape, mat, channel, wr, inside, T, sampler, next, sit);
          if (status == kWalkExited) walk_exit(sit.p, sit.n, wr.d, channel, it, l2w, w2l, bx, beta_channel);
          if (status != kWalkRunning) break;
          wr = next;
        }
      }

      SEC_MARK(4);  // sample_bxdf (+ BSSRDF walk)
      // ---- next-event estimation (path.cpp:98-113) ----
      f3 nee = mk3(0.0f);
      if (!bxdf_is_delta<F>(bx)) {
        nee = sample_direct<F, kSM>(V, S.num_lights, it, w2l, bx, mp, T, sampler, shadow_count, [&](const DRay& sr) -> bool {
          REGION(7);  // shadow ray cast
          DRay r = sr;
          int g2, p2;
          SEC_MARK(5);  // light sampling
          const bool occluded = scene_traverse<true, F>(V, r, stack, g2, p2);
          SEC_MARK(6);  // shadow traversal
          return occluded;
        });
      }

      SEC_MARK(7);  // NEE evaluation (and light sampling of lanes without a shadow ray)
      // ---- BSDF sampling + continuation (path.cpp:114-120) ----
      bx.albedo = mp.albedo;
      bx.albedo_over_pi = mp.albedo_over_pi;
      DBsdfSample bs;
      if (bxdf_sample<F, kSM>(bx, T, sampler, bs)) {
        const f3 wo_world = mul(l2w, bs.wo);
        const float cosine = absdot(wo_world, it.n);
        const int level = pv_length;
        const float entry[8] = {nee.x, nee.y, nee.z, bs.f.x, bs.f.y, bs.f.z, cosine / bs.pdf, bs.pdf};
        fold_store(level, entry);
        if constexpr (F & F_SSS)
          beta_flags = (beta_flags & ~(3ull << (2 * level))) | ((unsigned long long)beta_channel << (2 * level));
        const DRay nr = spawn_ray(it.p, it.n, wo_world, kFloatMax);
        ray_o = nr.o;
        ray_d = nr.d;
        ray_tmax = nr.tmax;
        st.set_dim(sampler.dimension & 0x1ff);
        if constexpr (kBigDim) big_dim = sampler.dimension;
        st.next_vertex(bs.is_delta);
      } else {
        // no continuation: this vertex resolves now with lo = nee (path.cpp:121)
        Lo = clamp_radiance(beta_channel, nee);
        terminal = true;
      }
    }

    SEC_MARK(8);  // BSDF sample + push
    if (terminal) {
      // ---- backward fold through the pending levels (path.cpp:114-121, Appendix A1) ----
      f3 Li = Lo;
      bool lp_valid = has_light_pdf;
      float lp = light_pdf;
      REGION(8);  // terminal fold entry
      for (int level = pv_length - 1; level >= 0; level--) {
        REGION(9);  // fold level
        float e[8];
        fold_load(level, e);
        fold_level<F>(e, beta_flags, level, Li, lp_valid, lp);
      }
      // .w = radiance() invocations of this sample (= depth reached + 1); resolve_kernel sums them
      const int s_now = st.s_cur();
      samples[size_t(sample_base) + size_t(s_now) * 64u] = make_float4(Li.x, Li.y, Li.z, float(pv_length + 1));
      st.v = unsigned(s_now + 1);
      if (closes_item(kspi, s_now + 1)) have_item = false;
      alive = false;
    }
    SEC_MARK(9);  // fold + sample store
  }

  SEC_FLUSH();
  // per-wave reduction of the shadow-ray counter, one atomic per wave
  unsigned long long sc = shadow_count;
  for (int off = 32; off > 0; off >>= 1) sc += __shfl_down(sc, off);
  if ((tid & 63) == 0) atomicAdd(&counters->shadow_rays, sc);
}

}  // namespace pine_gpu
#ifdef PINE_BAKED_SCENE
// generated at plan creation (pine_specialize.h) and found on the include path of that compile: namespace-less text
// that defines scene_traverse_baked<ANY, F>(ray, geom_out)
namespace pine_gpu {
#include "pine_baked_scene.inc"
}
#endif
#include "pine_trav.h"
#include "pine_queue_kernel.h"
