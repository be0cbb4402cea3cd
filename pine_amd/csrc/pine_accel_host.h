// pine_amd/csrc/pine_accel_host.h -- the host side of Accel's batched ray queries (kernels: pine_accel_kernel.h).  Included by
// pine_kernels.hip after plan_build's phases; of the shared steps (pine_plan_steps.h, pine_scene_steps.h) it takes
// upload_scene_records, pick_variant, lane_stack_lds_bytes, raise_lds_limit and create_object.  An accel has no film, no sampler
// and no work items: it is a SceneQuery -- the scene's records on the device, its launch and its destroy -- and the kernel pair
// chosen for the records.  The records are a snapshot: a geometry added to the scene later is not in them.  Nothing on the device
// is written after creation, so queries may run on several streams at once.

struct pine_gpu_accel : SceneQuery {
  const PineAccelVariant* kernel = nullptr;
};

// What every query checks before it looks at the accel: the ray count, then -- unless there is no ray -- the two buffers
// (`out_name` names the second).
static int accel_check_query(int64_t n, const void* rays, const void* out, bool device_pointers, const char* out_name) {
  if (n < 0 || n > int64_t(INT_MAX)) {
    set_error("Accel: the number of rays must lie in [0, 2^31 - 1]");
    return -1;
  }
  if (n == 0) return 0;  // (nothing is read or written: an empty tensor's pointer may be null)
  if (!rays || !out) {
    set_error("null argument");
    return -1;
  }
  if (device_pointers && ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(out)) & 15u)) {
    set_error(std::string("Accel: the rays and the ") + out_name + " must be 16-byte aligned device pointers");
    return -1;
  }
  return 0;
}

static int accel_build(pine_gpu_accel* a, pine_gpu_scene* scene, int device, uint32_t flags) {
  if (flags & (PINE_GPU_FLAG_FAST | PINE_GPU_FLAG_SPECIALIZE | PINE_GPU_FLAG_VERTEX_LOG)) {
    set_error((flags & PINE_GPU_FLAG_FAST)
                  ? "Accel: PINE_GPU_FLAG_FAST is not available (the ray queries are exact; there is no declared-tolerance kernel)"
                  : "Accel: PINE_GPU_FLAG_SPECIALIZE / _VERTEX_LOG are not available (precompiled kernels only)");
    return -1;
  }
  if (flags & ~uint32_t(PINE_GPU_FLAG_ORDER_EMBREE)) {
    set_error("Accel: the flags are 0 or PINE_GPU_FLAG_ORDER_EMBREE");
    return -1;
  }
  SceneHost& H = scene_host(scene);
  pine_gpu_render_params prm{};
  prm.spp = 1, prm.max_path_length = 1, prm.device = device, prm.shard_rank = 0, prm.shard_world = 1;
  prm.flags = int32_t(flags);
  a->plan.reset(new pine_gpu_plan());
  pine_gpu_plan* p = a->plan.get();
  std::chrono::steady_clock::time_point built;
  SceneRecords R;
  // (PINE_GPU_FLAG_ORDER_EMBREE: EmbreeAccel's hierarchy is built and checked against the per-ray stack in there)
  if (upload_scene_records(p, H, &prm, "Accel's ray queries", built, R)) return -1;
  a->device = device;
  a->has_camera = H.has_camera;

  // the kernels: the first variant that covers the scene's shape kinds in the order asked for; $PINE_GPU_ACCEL_VARIANT=<index>
  // considers that variant only (tests)
  const unsigned need = R.need & (kFAccelShapes | F_EMBREE);
  int count = 0;
  const PineAccelVariant* table = pine_gpu_accel_variant_table(&count);
  const int chosen = pick_variant(table, count, need, R.lds_ok, "PINE_GPU_ACCEL_VARIANT", "Accel");
  if (chosen < 0) return -1;
  if (((table[chosen].features ^ need) & F_EMBREE) != 0) {  // (a pinned variant of the other order)
    set_error("$PINE_GPU_ACCEL_VARIANT names a variant of the other traversal order");
    return -1;
  }
  a->kernel = &table[chosen];
  if (lane_stack_lds_bytes(p->S, a->kernel->features, 0, "Accel", a->lds_bytes)) return -1;
  return raise_lds_limit(device, a->kernel->intersect, a->lds_bytes) || raise_lds_limit(device, a->kernel->hit, a->lds_bytes) ? -1 : 0;
}

pine_gpu_accel* pine_gpu_accel_create(pine_gpu_scene* scene, int device, uint32_t flags) {
  return create_object(scene != nullptr, pine_gpu_accel_destroy, [&](pine_gpu_accel* a) { return accel_build(a, scene, device, flags); });
}

void pine_gpu_accel_destroy(pine_gpu_accel* a) { destroy_query(a); }

// One launch of `fn` over n rays on `stream`; nothing is waited for.
static int accel_launch(pine_gpu_accel* a, const void* fn, const void* rays_dev, int64_t n, void* out_dev, void* stream) {
  long long count = n;
  void* args[] = {&a->plan->S, (void*)&rays_dev, &count, &out_dev};
  return a->launch(fn, args, n, a->lds_bytes, stream);
}

int pine_gpu_accel_intersect_device(pine_gpu_accel* a, const void* rays_dev, int64_t n, void* hits_dev, void* stream) {
  if (accel_check_query(n, rays_dev, hits_dev, true, "hit records")) return -1;
  if (!a) {
    set_error("null argument");
    return -1;
  }
  if (n == 0) return 0;
  return accel_launch(a, a->kernel->intersect, rays_dev, n, hits_dev, stream);
}

int pine_gpu_accel_hit_device(pine_gpu_accel* a, const void* rays_dev, int64_t n, void* occluded_dev, void* stream) {
  // (one byte per ray: only the rays need the alignment)
  if (accel_check_query(n, rays_dev, occluded_dev, false, "")) return -1;
  if (n > 0 && (reinterpret_cast<uintptr_t>(rays_dev) & 15u)) {
    set_error("Accel: the rays must be a 16-byte aligned device pointer");
    return -1;
  }
  if (!a) {
    set_error("null argument");
    return -1;
  }
  if (n == 0) return 0;
  return accel_launch(a, a->kernel->hit, rays_dev, n, occluded_dev, stream);
}

// The host forms: upload, launch on the null stream, wait, download.
static int accel_query_host(pine_gpu_accel* a, const void* fn, const float* rays, int64_t n, void* out, size_t out_bytes_per_ray) {
  HIP_OK(hipSetDevice(a->device));
  const char* const what = "Accel: the query's buffers";
  DeviceBuffer<float> d_rays(kFromPool);
  DeviceBuffer<uint8_t> d_out(kFromPool);
  if (d_rays.upload(rays, size_t(n) * kAccelRayFloats, what) || d_out.alloc(size_t(n) * out_bytes_per_ray, what)) return -1;
  if (accel_launch(a, fn, d_rays.get(), n, d_out.get(), nullptr)) return -1;
  HIP_OK(hipStreamSynchronize(nullptr));
  return d_out.download(static_cast<uint8_t*>(out), size_t(n) * out_bytes_per_ray, "Accel: download");
}

int pine_gpu_accel_intersect(pine_gpu_accel* a, const float* rays_host, int64_t n, void* hits_host) {
  if (accel_check_query(n, rays_host, hits_host, false, "")) return -1;
  if (!a) {
    set_error("null argument");
    return -1;
  }
  if (n == 0) return 0;
  return accel_query_host(a, a->kernel->intersect, rays_host, n, hits_host, kAccelHitWords * sizeof(uint32_t));
}

int pine_gpu_accel_hit(pine_gpu_accel* a, const float* rays_host, int64_t n, uint8_t* occluded_host) {
  if (accel_check_query(n, rays_host, occluded_host, false, "")) return -1;
  if (!a) {
    set_error("null argument");
    return -1;
  }
  if (n == 0) return 0;
  return accel_query_host(a, a->kernel->hit, rays_host, n, occluded_host, 1);
}

int pine_gpu_accel_camera_rays_device(pine_gpu_accel* a, void* rays_dev, void* stream) {
  if (!rays_dev) {
    set_error("null argument");
    return -1;
  }
  if (reinterpret_cast<uintptr_t>(rays_dev) & 15u) {
    set_error("Accel: the rays must be a 16-byte aligned device pointer");
    return -1;
  }
  if (!a) {
    set_error("null argument");
    return -1;
  }
  if (!a->has_camera) {
    set_error("scene has no camera");
    return -1;
  }
  DCamera& cam = a->plan->S.cam;
  void* args[] = {&cam, &rays_dev};
  return a->launch(pine_gpu_accel_camera_rays_fn(), args, int64_t(cam.W) * cam.H, 0, stream);
}

int pine_gpu_accel_info(pine_gpu_accel* a, int32_t out[4]) {
  if (!a || !out) {
    set_error("null argument");
    return -1;
  }
  out[0] = int32_t(a->kernel->features), out[1] = int32_t(a->lds_bytes);
  out[2] = a->has_camera ? a->plan->S.cam.W : 0, out[3] = a->has_camera ? a->plan->S.cam.H : 0;
  return 0;
}
