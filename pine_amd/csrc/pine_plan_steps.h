// pine_amd/csrc/pine_plan_steps.h -- the host steps that building and launching a plan of any kind share: path plans (plan_build,
// path_launch_pass in pine_kernels.hip), AOIntegrator plans (pine_ao_host.h) and the guide pass (pine_guides_host.h).  Each is
// one free function that does one thing; an integrator calls the ones it needs in its own order, between its own decisions
// (refusals, kernel choice, work items, buffers).  Accel's and Shader's query objects (pine_accel_host.h, pine_shade_host.h)
// take the build steps too, and are one SceneQuery underneath: one launch, one destroy.  Included by pine_kernels.hip behind
// g_progress; the step that needs plan_build's phases (upload_scene_records) is in pine_scene_steps.h, included after them.

// The device check every hot path starts with (`who` names it in the error), then the caller's device made current.
static int open_device(const pine_gpu_render_params* prm, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error(std::string("no HIP device available: ") + who + " requires an AMD GPU (no CPU fallback)");
    return -1;
  }
  HIP_OK(hipSetDevice(prm->device));
  return 0;
}

// open_device, the plan's device and parameters, and the scene's BVH if nobody built it yet (accel_build_ms, accel_on_device).
// `built`: when that was done -- upload_ms counts from there.
static int plan_open_device(pine_gpu_plan* p, SceneHost& H, const pine_gpu_render_params* prm, const char* who,
                            std::chrono::steady_clock::time_point& built) {
  if (open_device(prm, who)) return -1;
  p->device = prm->device;
  p->params = *prm;
  const auto t0 = std::chrono::steady_clock::now();
  if (!H.accel.built) {
    H.build_on_device = (prm->flags & PINE_GPU_FLAG_DEVICE_BVH) ? prm->device : -1;
    H.build_accel();
  }
  built = std::chrono::steady_clock::now();
  p->accel_build_ms = std::chrono::duration<float, std::milli>(built - t0).count();
  p->accel_on_device = H.built_on_device;
  return 0;
}

// The first variant of `table` whose features cover `need` -- scene-in-LDS variants only if the blob fits (`lds_ok`); the
// environment variable `pin_env`=<index> considers that variant only (tests).  The index, or -1: `family` names the kernels in
// the error ("AO", "guide", "Accel", "Shader").
template <class Variant>
static int pick_variant(const Variant* table, int count, unsigned need, bool lds_ok, const char* pin_env, const char* family) {
  const char* pin = getenv(pin_env);
  for (int i = 0; i < count; i++) {
    if (pin && *pin && atoi(pin) != i) continue;
    const unsigned F = table[i].features;
    if ((need & ~F) == 0 && (!(F & F_LDS_SCENE) || lds_ok)) return i;
  }
  set_error(pin && *pin ? std::string("$") + pin_env + " names no " + family + " kernel variant that covers this scene"
                        : std::string("no ") + family + " kernel variant covers this scene");
  return -1;
}

// The dynamic LDS of a kernel whose lanes keep their traversal stacks there: `extra` bytes of the kernel's own, a stack per lane
// of a block, and the scene's blob if the variant stages it (F_LDS_SCENE).  More than a CU's 160 KiB is refused in `who`'s name.
static int lane_stack_lds_bytes(const DeviceScene& S, unsigned features, size_t extra, const char* who, size_t& lds_bytes) {
  lds_bytes = extra + size_t(S.stack_total) * kBlock * sizeof(int) + ((features & F_LDS_SCENE) ? size_t(S.blob_bytes) : 0);
  if (lds_bytes > 160 * 1024) {
    set_error(std::string(who) + ": the traversal stack of this scene does not fit LDS");
    return -1;
  }
  return 0;
}

// hipFuncAttributeMaxDynamicSharedMemorySize of kernel `fn` on `device` (the current one), raised to `lds_bytes` and never
// lowered: the attribute belongs to the function on that device, not to the plan or query object that asks, and a later,
// smaller object must not lower it under an earlier one's launches.  So the limit is the largest size any object, live or
// gone, has asked for: never below what a launch needs.
static int raise_lds_limit(int device, const void* fn, size_t lds_bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> limit;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = limit[{device, fn}];
  if (lds_bytes <= have) return 0;
  HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds_bytes)));
  have = lds_bytes;
  return 0;
}

// The film's 8x8 tiles and this shard's share of them (local tile t is film tile t * shard_world + shard_rank).  Pixel
// coordinates travel as 16 + 16 bits in the kernels: larger films are refused.
static int shard_tiles(WorkParams& W, int film_w, int film_h, const pine_gpu_render_params* prm) {
  if (film_w > 65535 || film_h > 65535) {
    set_error("film sides above 65535 are not supported");
    return -1;
  }
  W.tiles_x = (film_w + kTile - 1) / kTile, W.tiles_y = (film_h + kTile - 1) / kTile;
  W.tiles_x_magic = unsigned(((1ull << 32) + unsigned(W.tiles_x) - 1) / unsigned(W.tiles_x));  // tiles_x >= 1
  W.shard_rank = prm->shard_rank, W.shard_world = prm->shard_world;
  W.num_local_tiles = (W.tiles_x * W.tiles_y - prm->shard_rank + prm->shard_world - 1) / prm->shard_world;
  return 0;
}

// Work items of k samples (k divides spp): the per-pixel item fields, and the pass window of a plan's W -- the whole render
// (pass_work narrows it to a pass).
static void items_of_k_samples(WorkParams& W, int spp, int k) {
  W.samples_per_item = k;
  W.items_per_pixel = spp / k;
  W.log2_items_per_pixel = 0;
  while ((1 << W.log2_items_per_pixel) < W.items_per_pixel) W.log2_items_per_pixel++;
  W.pass_first_chunk = 0;
  W.pass_chunks = W.items_per_pixel;
  W.pass_chunks_magic = W.pass_chunks > 1 ? unsigned(((1ull << 32) + unsigned(W.pass_chunks) - 1) / unsigned(W.pass_chunks)) : 0u;
  W.pass_row_stride = spp;
  W.pass_first_serial_tile = 0;
}

// PINE_GPU_FLAG_PROGRESS: the host-mapped word the kernel counts claimed items in (WorkParams::progress).
static int plan_progress_word(pine_gpu_plan* p, const pine_gpu_render_params* prm) {
  if (!(prm->flags & PINE_GPU_FLAG_PROGRESS)) return 0;
  if (alloc_pinned(p->h_progress, 1, hipHostMallocMapped, "plan creation: the progress word")) return -1;
  p->h_progress[0] = 0;
  HIP_OK(hipHostGetDevicePointer((void**)&p->W.progress, p->h_progress.get(), 0));
  return 0;
}

// PINE_GPU_FLAG_TIMING: the ring of per-launch events.
static int plan_timing_events(pine_gpu_plan* p, const pine_gpu_render_params* prm) {
  p->timed = (prm->flags & PINE_GPU_FLAG_TIMING) != 0;
  if (p->timed)
    for (auto& slot : p->ev)
      for (auto& e : slot)
        if (create_event(e, hipEventDefault, "plan creation: the timing events")) return -1;
  return 0;
}

// A new object -- a plan, an accel, a shader -- that `build(object)` fills, or null with build's error: what the failed build
// left is destroyed with the object.  `have_args`: none of the caller's pointers is null.
template <class Object, class Build>
static Object* create_object(bool have_args, void (*destroy)(Object*), Build build) {
  if (!have_args) {
    set_error("null argument");
    return nullptr;
  }
  Object* o = new Object();
  if (build(o)) {
    std::string keep = pine_gpu_last_error();
    destroy(o);
    set_error(keep);
    return nullptr;
  }
  return o;
}

// What an accel and a shader are: the scene's records on a device -- held in a pine_gpu_plan that is never launched, so that
// the buffers have the owners and the pool every plan's have -- read by kernels that write the caller's buffers only.
struct SceneQuery {
  PlanOwner plan;  // S: the scene view; the d_* blocks behind it
  int device = 0;
  size_t lds_bytes = 0;  // of the kernels that read the scene
  bool has_camera = false;
  std::atomic<bool> launched{false};  // a launch may still be reading the records: destroy waits for the device first

  // One launch of `fn` over n lanes on `stream`; nothing is waited for.
  int launch(const void* fn, void** args, int64_t n, size_t lds, void* stream) {
    HIP_OK(hipSetDevice(device));
    (void)hipGetLastError();
    launched.store(true);
    HIP_OK(hipLaunchKernel(fn, dim3(unsigned((n + kBlock - 1) / kBlock)), dim3(kBlock), args, lds, static_cast<hipStream_t>(stream)));
    return 0;
  }
};

// The records go back to the pool with the plan: every launch that reads them, on whatever stream, must have finished.
template <class Query>
static void destroy_query(Query* q) {
  if (!q) return;
  if (q->launched.load()) {
    (void)hipSetDevice(q->device);
    (void)hipDeviceSynchronize();
  }
  delete q;
}

// A launch is: launch_begin, [the integrator's own clears], mark 0, checkpoint_prepass, mark 1, [its kernel], mark 2, [its film
// pass], launch_end.
// Pass j (0: the only one, or the first of a sequence) starts: the plan's device, HIP's sticky error out of the way (what
// launch_end reports must come from THIS launch's calls), the scene's own kernel adopted if its background build has finished
// (between two passes too: the same bits; a plan that asked for none has nothing to poll), the film cleared for an unpacked
// shard, the counters cleared.
static int launch_begin(pine_gpu_plan* p, int j, void* film_dev, hipStream_t stream, bool packed) {
  HIP_OK(hipSetDevice(p->device));
  (void)hipGetLastError();
  p->scene_kernel.poll();
  if (j == 0) g_progress.store(0.0f);
  if (p->W.shard_world > 1 && !packed) HIP_OK(hipMemsetAsync(film_dev, 0, size_t(p->film_w) * p->film_h * sizeof(float4), stream));
  // the counters of the sequence start with pass 0 -- with them the owned tiles' done marks, which sit behind them (plans of one
  // pass); every pass hands out its own items from zero
  static_assert(offsetof(Counters, next_item) == 0, "the per-pass reset clears next_item");
  const size_t done_bytes = p->W.tile_done ? size_t(p->W.num_local_tiles) * sizeof(unsigned) : 0;
  HIP_OK(hipMemsetAsync(p->d_counters, 0, j == 0 ? sizeof(Counters) + done_bytes : sizeof(unsigned long long), stream));
  return 0;
}

// Timing point i of this launch (0 prepass start, 1 kernel start, 2 film pass start, 3 end), if the plan is timed.
static int launch_mark(const pine_gpu_plan* p, int i, hipStream_t stream) {
  if (p->timed) HIP_OK(hipEventRecord(p->ev[p->launch_count % pine_gpu_plan::kEvRing][i].get(), stream));
  return 0;
}

// The RNG checkpoints of the items of W (the plan's, or a pass's window of it), where a pixel is more than one item.  A plan of
// one pass computes them once and keeps them (pine_plan.h ckpt_valid): later launches reuse the table, waiting for `ckpt_done`
// when they run on another stream.  A pass of a longer sequence walks on from the carried states, every time.  The table counts
// as there only once its kernel is known to be launched and the event behind it recorded.
static int checkpoint_prepass(pine_gpu_plan* p, const WorkParams& W, hipStream_t stream) {
  const PassPlan& PP = p->pass_plan;
  if (W.total_items == 0 || p->W.items_per_pixel <= 1 || PP.free_tiles <= 0) return 0;
  const bool keep = PP.n == 1;
  if (keep && p->ckpt_valid && !p->ckpt_every_launch) {
    if (stream != p->ckpt_stream) HIP_OK(hipStreamWaitEvent(stream, p->ckpt_done.get(), 0));
    return 0;
  }
  p->ckpt_valid = false;
  const unsigned long long n = (unsigned long long)PP.free_tiles * 64ull;
  hipLaunchKernelGGL(rng_checkpoint_kernel, dim3(unsigned((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, W, p->film_w, p->film_h, p->S.spp,
                     p->d_ckpt, PP.free_tiles, p->d_rng_carry);
  if (!keep) return 0;
  HIP_OK(hipGetLastError());
  if (!p->ckpt_done && create_event(p->ckpt_done, hipEventDisableTiming, "launch: the checkpoint event")) return -1;
  HIP_OK(hipEventRecord(p->ckpt_done.get(), stream));
  p->ckpt_stream = stream;
  p->ckpt_valid = true;
  return 0;
}

// The launch is enqueued: mark 3, whatever its kernel launches left as HIP's last error, the plan's launch record.
static int launch_end(pine_gpu_plan* p, hipStream_t stream) {
  if (launch_mark(p, 3, stream)) return -1;
  HIP_OK(hipGetLastError());
  p->launched = true, p->launch_count++, p->last_stream = stream;
  return 0;
}
