// pine_amd/csrc/pine_shade_host.h -- the host side of Shader's batched path-vertex queries (kernels: pine_shade_kernel.h).
// Included by pine_kernels.hip behind pine_accel_host.h.  Like an accel, a shader is the scene's records on the device, held in a
// pine_gpu_plan that is never launched -- of the steps of pine_plan_steps.h it takes plan_open_device and pick_variant, of
// plan_build's phases assemble_scene (without a frame table: the hit record carries no entry), scene_features and the sampler's
// tables -- and the vertex kernel chosen for them.  The records are a snapshot.  Nothing on the device is written after creation:
// paths live in the caller's buffers, so calls on several streams may run at once.

struct pine_gpu_shader : SceneQuery {  // (plan->S: the sampler's tables too)
  int variant = 0;
  const PineShadeVariant* kernel = nullptr;
  int spp = 0;  // effective
};

static int shader_build(pine_gpu_shader* s, pine_gpu_scene* scene, const pine_gpu_render_params* prm) {
  if (prm->flags != 0) {
    const int32_t fl = prm->flags;
    set_error(std::string("Shader: the flags must be 0; ") +
              ((fl & PINE_GPU_FLAG_FAST)          ? "PINE_GPU_FLAG_FAST is not available (the vertex steps are exact; there is no declared-tolerance kernel)"
               : (fl & PINE_GPU_FLAG_SPECIALIZE)  ? "PINE_GPU_FLAG_SPECIALIZE is not available (precompiled kernels only)"
               : (fl & PINE_GPU_FLAG_VERTEX_LOG)  ? "PINE_GPU_FLAG_VERTEX_LOG is not available (pine_gpu_shader_fold_device writes the log)"
               : (fl & PINE_GPU_FLAG_ORDER_EMBREE) ? "PINE_GPU_FLAG_ORDER_EMBREE is the Accel's business (a shader shades hits of either order)"
                                                   : "no flag applies to a shader"));
    return -1;
  }
  if (prm->shard_world != 1 || prm->shard_rank != 0) {
    set_error("Shader: shard_world must be 1 (and shard_rank 0): the paths are the caller's to divide");
    return -1;
  }
  if (prm->max_path_length <= 0) {  // path.cpp:12-13
    set_error("`PathIntegrator` expect `max_path_length` to be positive");
    return -1;
  }
  if (prm->max_path_length > kMaxDepth) {
    set_error("Shader: max_path_length above the supported depth (32)");
    return -1;
  }
  // the plan's rules (check_params): BlueSampler(n) rounds n up to a power of two and clamps it at 256; SobolSampler(n) and
  // HaltonSampler(n) take n as given, up to the 12 bits of sample index in the packed path state
  const bool halton = prm->sampler == PINE_GPU_SAMPLER_HALTON;
  const bool sobol = prm->sampler == PINE_GPU_SAMPLER_SOBOL || halton;
  if (prm->sampler != PINE_GPU_SAMPLER_BLUE && !sobol) {
    set_error("unknown sampler kind");
    return -1;
  }
  const int spp = sobol ? prm->spp : effective_spp(prm->spp);
  if (spp <= 0) {
    set_error("Shader: samples per pixel must be positive");
    return -1;
  }
  if (spp > kMaxDeviceSpp) {
    set_error("Shader: SobolSampler / HaltonSampler on the device: at most 4096 samples per pixel");
    return -1;
  }
  SceneHost& H = scene_host(scene);
  for (size_t m = 0; m < H.materials.size(); m++)
    if (H.materials[m].kind == MAT_SUBSURFACE) {
      set_error("Shader: Subsurface material `" + (m < H.material_names.size() ? H.material_names[m] : std::string("?")) +
                "` is not available: its BSSRDF walk traverses inside the vertex, which is not one step");
      return -1;
    }
  if (H.has_camera && (H.camera.W > 65535 || H.camera.H > 65535)) {
    set_error("film sides above 65535 are not supported");
    return -1;
  }
  TableBlob tables_blob;
  if (load_tables(tables_blob)) return -1;
  s->plan.reset(new pine_gpu_plan());
  pine_gpu_plan* p = s->plan.get();
  std::chrono::steady_clock::time_point built;
  SceneRecords R;
  // (without a frame table: the hit record carries no entry)
  if (upload_scene_records(p, H, prm, "Shader's vertex queries", built, R)) return -1;
  s->device = prm->device;
  s->has_camera = H.has_camera;
  s->spp = spp;
  if (upload_sampler_tables(p, *tables_blob, prm, spp)) return -1;
  p->S.spp = spp;

  // the vertex kernel: the first variant that covers the scene; $PINE_GPU_SHADER_VARIANT=<index> considers that variant only (tests)
  int count = 0;
  const PineShadeVariant* table = pine_gpu_shade_variant_table(&count);
  const int chosen = pick_variant(table, count, R.need, R.lds_ok, "PINE_GPU_SHADER_VARIANT", "Shader");
  if (chosen < 0) return -1;
  s->variant = chosen;
  s->kernel = &table[chosen];
  s->lds_bytes = (s->kernel->features & F_LDS_SCENE) ? size_t(p->S.blob_bytes) : 0;
  HIP_OK(hipDeviceSynchronize());  // (the uploads)
  return 0;
}

pine_gpu_shader* pine_gpu_shader_create(pine_gpu_scene* scene, const pine_gpu_render_params* prm) {
  return create_object(scene && prm, pine_gpu_shader_destroy, [&](pine_gpu_shader* s) { return shader_build(s, scene, prm); });
}

void pine_gpu_shader_destroy(pine_gpu_shader* s) { destroy_query(s); }

int pine_gpu_shader_layout(int32_t out[4]) {
  if (!out) {
    set_error("null argument");
    return -1;
  }
  out[0] = kShadeStateWords * 4, out[1] = kShadeRecordWords * 4, out[2] = kAccelRayFloats, out[3] = kVertexLogFloats;
  return 0;
}

int pine_gpu_shader_info(pine_gpu_shader* s, int32_t out[8]) {
  if (!s || !out) {
    set_error("null argument");
    return -1;
  }
  const DeviceScene& S = s->plan->S;
  out[0] = s->has_camera ? S.cam.W : 0, out[1] = s->has_camera ? S.cam.H : 0;
  out[2] = s->spp, out[3] = S.max_path_length, out[4] = s->variant, out[5] = int32_t(s->kernel->features);
  out[6] = int32_t(s->lds_bytes), out[7] = S.tables.kind;
  return 0;
}

// What every call checks first: the shader, the path count, then -- unless there is no path -- the buffers.
static int shader_check(pine_gpu_shader* s, int64_t n, std::initializer_list<const void*> buffers) {
  if (!s) {
    set_error("null argument");
    return -1;
  }
  if (n < 0 || n > int64_t(INT_MAX)) {
    set_error("Shader: the number of paths must lie in [0, 2^31 - 1]");
    return -1;
  }
  if (n == 0) return 0;  // (nothing is read or written: an empty tensor's pointer may be null)
  for (const void* b : buffers) {
    if (!b) {
      set_error("null argument");
      return -1;
    }
    if (reinterpret_cast<uintptr_t>(b) & 15u) {
      set_error("Shader: every buffer must be a 16-byte aligned device pointer");
      return -1;
    }
  }
  return 0;
}
static int shader_check_sample(const pine_gpu_shader* s, int sample) {
  if (sample < 0 || sample >= s->spp) {
    set_error("Shader: the sample index must lie in [0, spp = " + std::to_string(s->spp) + ")");
    return -1;
  }
  return 0;
}

int pine_gpu_shader_begin_device(pine_gpu_shader* s, int sample, void* states_dev, void* rays_dev, void* stream) {
  if (shader_check(s, 1, {states_dev, rays_dev})) return -1;
  if (!s->has_camera) {
    set_error("scene has no camera");
    return -1;
  }
  if (shader_check_sample(s, sample)) return -1;
  DCamera cam = s->plan->S.cam;
  int kind = s->plan->S.tables.kind;
  void* args[] = {&cam, &kind, &sample, &states_dev, &rays_dev};
  return s->launch(pine_gpu_shade_begin_fn(), args, int64_t(cam.W) * cam.H, 0, stream);
}

int pine_gpu_shader_vertex_device(pine_gpu_shader* s, const void* rays_dev, const void* hits_dev, int64_t n, void* states_dev, void* records_dev,
                                  void* shadow_rays_dev, void* next_rays_dev, void* stream) {
  if (shader_check(s, n, {rays_dev, hits_dev, states_dev, records_dev, shadow_rays_dev, next_rays_dev})) return -1;
  if (n == 0) return 0;
  long long count = n;
  void* args[] = {&s->plan->S, (void*)&rays_dev, (void*)&hits_dev, &count, &states_dev, &records_dev, &shadow_rays_dev, &next_rays_dev};
  return s->launch(s->kernel->vertex, args, n, s->lds_bytes, stream);
}

int pine_gpu_shader_fold_device(pine_gpu_shader* s, const void* records_dev, const void* occluded_dev, int levels, int64_t n, int sample, void* sum_dev,
                                void* log_dev_or_null, void* stream) {
  // (one byte per vertex: the occlusion answers need no alignment)
  if (shader_check(s, n, {records_dev, sum_dev})) return -1;
  if (levels < 1 || levels > s->plan->S.max_path_length) {
    set_error("Shader: the number of levels must lie in [1, max_path_length = " + std::to_string(s->plan->S.max_path_length) + "]");
    return -1;
  }
  if (shader_check_sample(s, sample)) return -1;
  if (n == 0) return 0;
  if (!occluded_dev) {
    set_error("null argument");
    return -1;
  }
  if (reinterpret_cast<uintptr_t>(log_dev_or_null) & 15u) {
    set_error("Shader: every buffer must be a 16-byte aligned device pointer");
    return -1;
  }
  long long count = n;
  void* args[] = {(void*)&records_dev, (void*)&occluded_dev, &levels, &count, &sample, &sum_dev, &log_dev_or_null};
  return s->launch(pine_gpu_shade_fold_fn(), args, n, 0, stream);
}

int pine_gpu_shader_resolve_device(pine_gpu_shader* s, const void* sum_dev, int64_t n, void* film_dev, void* stream) {
  if (shader_check(s, n, {sum_dev, film_dev})) return -1;
  if (n == 0) return 0;
  long long count = n;
  int spp = s->spp;
  void* args[] = {(void*)&sum_dev, &count, &spp, &film_dev};
  return s->launch(pine_gpu_shade_resolve_fn(), args, n, 0, stream);
}
