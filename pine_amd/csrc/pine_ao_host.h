// pine_amd/csrc/pine_ao_host.h -- the host side of AOIntegrator plans (kernels: pine_ao_kernel.h).  Included by
// pine_kernels.hip after plan_build's phases.  Of those an AO plan runs check_params and upload_sampler_tables itself, and
// between them the shared steps (pine_plan_steps.h, pine_scene_steps.h), in its own order: upload_scene_records, pick_variant,
// lane_stack_lds_bytes, raise_lds_limit, shard_tiles, items_of_k_samples, plan_progress_word, plan_timing_events to build
// (create_object around them); launch_begin, launch_mark, checkpoint_prepass, launch_end to launch.  Its refusals, the chunks of
// k samples and its buffers are its own.  An AO plan is a pine_gpu_plan with `ao` set: pine_gpu_plan_launch / _stats_get /
// _check / _destroy take it as they take any plan.

// The AO sample count (ao.cpp:13) of a sampler whose own count is `sampler_spp`.
static int ao_effective_spp(int sampler_spp) { return std::max(sampler_spp / 8, 1); }

static int ao_plan_build(pine_gpu_plan* p, pine_gpu_scene* scene, const pine_gpu_render_params* prm_in) {
  SceneHost& H = scene_host(scene);
  if (prm_in->flags & (PINE_GPU_FLAG_FAST | PINE_GPU_FLAG_ORDER_EMBREE | PINE_GPU_FLAG_VERTEX_LOG | PINE_GPU_FLAG_SPECIALIZE)) {
    set_error((prm_in->flags & PINE_GPU_FLAG_ORDER_EMBREE)
                  ? "AOIntegrator renders in pine-BVH order only, AOIntegrator(BVH(), sampler): EmbreeAccel answers hit8 with Embree's packet "
                    "traversal, which is not restated (PINE_GPU_FLAG_ORDER_EMBREE refused)"
                  : "AOIntegrator: PINE_GPU_FLAG_FAST / _VERTEX_LOG / _SPECIALIZE are not available (exact arithmetic, precompiled kernels only)");
    return -1;
  }
  pine_gpu_render_params prm = *prm_in;
  prm.max_path_length = 1;  // (ignored by AOIntegrator; check_params wants a valid one)
  prm.samples_per_item = 0;
  const int sampler_spp = check_params(H, &prm);
  if (sampler_spp < 0) return -1;
  const int spp = ao_effective_spp(sampler_spp);
  TableBlob tables_blob;
  if (load_tables(tables_blob)) return -1;
  std::chrono::steady_clock::time_point t_build1;
  const size_t tally0 = g_alloc_tally;  // (the BVH build takes nothing from the pool)
  SceneRecords R;
  if (upload_scene_records(p, H, &prm, "the AOIntegrator hot path", t_build1, R)) return -1;
  p->ao = true;
  // (the sampler keeps its ORIGINAL count -- BlueSampler's table, SobolSampler's index stride -- only fewer indices are drawn)
  if (upload_sampler_tables(p, *tables_blob, &prm, sampler_spp)) return -1;
  p->S.spp = spp;
  if (pine_gpu_ao_constants(scene, &p->ao_params.radius)) return -1;
  static_assert(offsetof(AoParams, dir) == sizeof(float) && sizeof(AoParams) == 26 * sizeof(float), "radius, then directions[8]");
  p->ao_params.spp = spp;

  // the kernel: the first variant that covers the scene's shape kinds and sampler, in the schedule $PINE_GPU_AO_KERNEL names
  // (serial, the default: lane = sample; regroup: the wave's occlusion rays regrouped); $PINE_GPU_AO_VARIANT=<index> considers that variant only (tests)
  int count = 0;
  const PineAoVariant* table = pine_gpu_ao_variants(&count);
  p->ao_variant = pick_variant(table, count, R.need & (kFAoShapes | F_SOBOL), R.lds_ok, "PINE_GPU_AO_VARIANT", "AO");
  if (p->ao_variant < 0) return -1;
  p->ao_serial = true;  // (the faster of the two on two of the three measured scenes: DESIGN.md 4.11, profiles/ao_speed.txt)
  if (const char* e = getenv("PINE_GPU_AO_KERNEL")) {
    if (!strcmp(e, "regroup")) p->ao_serial = false;
    else if (*e && strcmp(e, "serial")) {
      set_error("$PINE_GPU_AO_KERNEL is `serial` or `regroup`");
      return -1;
    }
  }
  const PathKernel kernel = plan_kernel(p);
  if (lane_stack_lds_bytes(p->S, kernel.features, size_t(ao_off_stack(!p->ao_serial)) * 4, "AOIntegrator", p->lds_bytes) ||
      raise_lds_limit(prm.device, kernel.fn, p->lds_bytes))
    return -1;

  // work items: [local tile][chunk of k samples][pixel in tile]; k the largest power of two dividing the AO count that
  // still leaves 2^20 items (a lane walks its k samples in sequence; the chunks start from RNG checkpoints)
  WorkParams& W = p->W;
  p->film_w = H.camera.W, p->film_h = H.camera.H;
  if (shard_tiles(W, p->film_w, p->film_h, &prm)) return -1;
  int k = 1;
  while (spp % (2 * k) == 0 && (unsigned long long)W.num_local_tiles * 64ull * unsigned(spp / (2 * k)) >= (1ull << 20)) k *= 2;
  items_of_k_samples(W, spp, k);
  W.total_items = (unsigned long long)W.num_local_tiles * unsigned(W.items_per_pixel) * 64ull;
  if (W.total_items >= (1ull << 32)) {  // (decode_item's tile-and-chunk number is 32 bits less the pixel's six)
    set_error("film pixels x AO samples per pixel of one shard must stay below 2^32 (render in several shards)");
    return -1;
  }
  W.tile_order = nullptr;
  W.serial_tiles = 0;
  W.free_tile_base = 0;
  W.debug_force_bail = (prm.flags & PINE_GPU_FLAG_DEBUG_FORCE_BAIL) ? 1 : 0;
  W.progress = nullptr;
  W.vertex_log = nullptr;
  p->pass_plan = PassPlan();
  p->pass_plan.free_tiles = W.num_local_tiles;
  if (plan_progress_word(p, &prm)) return -1;
  const char* const what = "plan creation: the launch buffers";
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, prm.device));
  int blocks_per_cu = 0;
  HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kernel.fn, kBlock, p->lds_bytes));
  blocks_per_cu = std::min(std::max(blocks_per_cu, 1), 8);
  p->grid = int(std::min<unsigned long long>((W.total_items + kBlock - 1) / kBlock, (unsigned long long)prop.multiProcessorCount * blocks_per_cu));
  if (p->grid < 1) p->grid = 1;
  if (W.items_per_pixel > 1) {
    p->bytes_ckpt = W.total_items * sizeof(ulonglong2);
    if (p->d_ckpt.alloc(W.total_items, what)) return -1;
  }
  if (p->d_ao_counts.alloc(size_t(p->film_w) * p->film_h, what) || p->d_counters.alloc(1, what)) return -1;
  if (plan_timing_events(p, &prm)) return -1;
  p->bytes_total = g_alloc_tally - tally0;
  HIP_OK(hipDeviceSynchronize());
  p->upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_build1).count();
  return 0;
}

// One AO render into film_dev: counters and counts cleared, checkpoint prepass (first launch), the AO kernel, the film from the counts.
static int ao_launch(pine_gpu_plan* p, void* film_dev, hipStream_t stream) {
  WorkParams& W = p->W;
  if (launch_begin(p, 0, film_dev, stream, false)) return -1;
  HIP_OK(hipMemsetAsync(p->d_ao_counts, 0, size_t(p->film_w) * p->film_h * sizeof(unsigned), stream));
  if (launch_mark(p, 0, stream) || checkpoint_prepass(p, W, stream) || launch_mark(p, 1, stream)) return -1;
  if (W.total_items > 0) {
    const PathKernel kernel = plan_kernel(p);
    const ulonglong2* ckpt = p->d_ckpt;
    unsigned* counts = p->d_ao_counts;
    Counters* counters = p->d_counters;
    void* args[] = {&p->S, &W, &p->ao_params, &ckpt, &counts, &counters};
    HIP_OK(hipLaunchKernel(kernel.fn, dim3(p->grid), dim3(kBlock), args, p->lds_bytes, stream));
  }
  if (launch_mark(p, 2, stream)) return -1;
  if (W.num_local_tiles > 0) {
    const unsigned long long n = (unsigned long long)W.num_local_tiles * 64ull;
    hipLaunchKernelGGL(ao_film_kernel, dim3(unsigned((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, W, p->film_w, p->film_h, p->S.spp,
                       p->d_ao_counts.get(), (float4*)film_dev);
  }
  return launch_end(p, stream);
}

pine_gpu_plan* pine_gpu_ao_plan_create(pine_gpu_scene* scene, const pine_gpu_render_params* prm) {
  return create_object(scene && prm, pine_gpu_plan_destroy, [&](pine_gpu_plan* p) { return ao_plan_build(p, scene, prm); });
}

// AOIntegrator(BVH(), sampler).render(scene) in one call: upload, launch, download.  Fails if there is no GPU.
int pine_gpu_ao_render(pine_gpu_scene* scene, const pine_gpu_render_params* prm, float* film_out) {
  if (!scene || !prm || !film_out) {
    set_error("null argument");
    return -1;
  }
  pine_gpu_render_params prm2 = *prm;
  prm2.flags |= PINE_GPU_FLAG_PROGRESS;
  pine_gpu_plan* p = pine_gpu_ao_plan_create(scene, &prm2);
  if (!p) return -1;
  return one_shot_render(p, p->W.total_items, [&](float4* d_film, size_t bytes) {
    if (pine_gpu_plan_launch(p, d_film, nullptr)) return -1;
    if (const hipError_t e = hipMemcpy(film_out, d_film, bytes, hipMemcpyDeviceToHost)) return hip_error("film download", e);
    return pine_gpu_plan_check(p);  // (a launch that gave up leaves an incomplete film: fail)
  });
}
