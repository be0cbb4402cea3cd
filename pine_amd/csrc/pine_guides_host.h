// pine_amd/csrc/pine_guides_host.h -- the host side of DenoiseIntegrator's guide images (kernels: pine_guides_kernel.h).  Included
// by pine_kernels.hip after plan_build's phases, of which the guide pass runs check_params itself; of the shared steps
// (pine_plan_steps.h, pine_scene_steps.h) it takes shard_tiles, upload_scene_records (open_device alone for the output buffers),
// pick_variant, lane_stack_lds_bytes and raise_lds_limit.  The pass has no plan of its own and no launch frame: the scene's
// records are uploaded into a pine_gpu_plan that lives for the length of the call, one kernel is launched and waited for.

static int guides_render_device(pine_gpu_scene* scene, const pine_gpu_render_params* prm_in, float* albedo_dev, float* normal_dev, hipStream_t stream) {
  SceneHost& H = scene_host(scene);
  if (prm_in->flags & PINE_GPU_FLAG_ORDER_EMBREE) {
    set_error("DenoiseIntegrator's guide images are rendered in pine-BVH order only, DenoiseIntegrator(BVH(), ...): EmbreeAccel's order would "
              "need fixtures of the Embree build and its tie pixels (PINE_GPU_FLAG_ORDER_EMBREE refused)");
    return -1;
  }
  if (prm_in->flags & (PINE_GPU_FLAG_FAST | PINE_GPU_FLAG_VERTEX_LOG | PINE_GPU_FLAG_SPECIALIZE)) {
    set_error((prm_in->flags & PINE_GPU_FLAG_FAST)
                  ? "guide images: PINE_GPU_FLAG_FAST is not available (the guide images are exact; there is no declared-tolerance kernel)"
                  : "guide images: PINE_GPU_FLAG_SPECIALIZE / _VERTEX_LOG are not available (precompiled kernels only)");
    return -1;
  }
  if (prm_in->shard_world != 1 || prm_in->shard_rank != 0) {
    set_error("guide images: sharded films are not supported (shard_world must be 1)");
    return -1;
  }
  pine_gpu_render_params prm = *prm_in;
  prm.spp = 1, prm.sampler = PINE_GPU_SAMPLER_BLUE;  // (the pass draws nothing; check_params wants valid ones)
  prm.max_path_length = 1;
  prm.samples_per_item = 0;
  if (check_params(H, &prm) < 0) return -1;
  PlanOwner p(new pine_gpu_plan());
  std::chrono::steady_clock::time_point built;
  SceneRecords R;
  // (the film-size refusal comes before the device check)
  if (shard_tiles(p->W, H.camera.W, H.camera.H, &prm) || upload_scene_records(p.get(), H, &prm, "the guide images' hot path", built, R)) return -1;

  // the kernel: the first variant that covers the scene's shape kinds and node programs; $PINE_GPU_GUIDES_VARIANT=<index>
  // considers that variant only (tests)
  int count = 0;
  const PineGuidesVariant* table = pine_gpu_guides_variant_table(&count);
  const int chosen = pick_variant(table, count, R.need & (kFGuidesShapes | F_NODES), R.lds_ok, "PINE_GPU_GUIDES_VARIANT", "guide");
  if (chosen < 0) return -1;
  const PineGuidesVariant& K = table[chosen];
  size_t lds_bytes = 0;
  if (lane_stack_lds_bytes(p->S, K.features, 0, "guide images", lds_bytes) || raise_lds_limit(prm.device, K.fn, lds_bytes)) return -1;
  int tiles_x = p->W.tiles_x, num_tiles = p->W.num_local_tiles;  // (shard_world is 1: every tile of the film)
  void* args[] = {&p->S, &tiles_x, &num_tiles, &albedo_dev, &normal_dev};
  const unsigned grid = unsigned((num_tiles + kBlock / 64 - 1) / (kBlock / 64));
  HIP_OK(hipLaunchKernel(K.fn, dim3(grid), dim3(kBlock), args, lds_bytes, stream));
  // the scene's records go back to the pool with `p`: the launch that reads them must have finished
  HIP_OK(hipStreamSynchronize(stream));
  return 0;
}

int pine_gpu_guides_render_device(pine_gpu_scene* scene, const pine_gpu_render_params* prm, void* albedo_dev, void* normal_dev, void* stream) {
  if (!scene || !prm || !albedo_dev || !normal_dev) {
    set_error("null argument");
    return -1;
  }
  return guides_render_device(scene, prm, static_cast<float*>(albedo_dev), static_cast<float*>(normal_dev), static_cast<hipStream_t>(stream));
}

// DenoiseIntegrator's guide pass in one call: upload, launch, download.  Fails if there is no GPU.
int pine_gpu_guides_render(pine_gpu_scene* scene, const pine_gpu_render_params* prm, float* albedo_out, float* normal_out) {
  if (!scene || !prm || !albedo_out || !normal_out) {
    set_error("null argument");
    return -1;
  }
  SceneHost& H = scene_host(scene);
  if (!H.has_camera) {
    set_error("scene has no camera");
    return -1;
  }
  if (open_device(prm, "the guide images' hot path")) return -1;  // (for the output buffers)
  const size_t n = size_t(H.camera.W) * size_t(H.camera.H) * 3;
  const char* const what = "guide images: the output buffers";
  DeviceBuffer<float> d_albedo(kFromPool), d_normal(kFromPool);
  if (d_albedo.alloc(n, what) || d_normal.alloc(n, what)) return -1;
  if (guides_render_device(scene, prm, d_albedo, d_normal, nullptr)) return -1;
  return d_albedo.download(albedo_out, n, "guide images: download") || d_normal.download(normal_out, n, "guide images: download") ? -1 : 0;
}

int pine_gpu_guides_variants(uint32_t* features, int cap) {
  int count = 0;
  const PineGuidesVariant* table = pine_gpu_guides_variant_table(&count);
  for (int i = 0; i < count && i < cap; i++)
    if (features) features[i] = table[i].features;
  return count;
}
