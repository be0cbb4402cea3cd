// pine_amd/csrc/pine_scene_steps.h -- the one shared build step that needs plan_build's phases (assemble_scene, scene_features),
// so it cannot stand with the others in pine_plan_steps.h.  Included by pine_kernels.hip after plan_build, before the hosts that
// call it: pine_ao_host.h, pine_guides_host.h, pine_accel_host.h, pine_shade_host.h.

// What upload_scene_records hands back beside the records in the plan.
struct SceneRecords {
  SceneParts parts;     // host copies of what was uploaded
  unsigned need = 0;    // the scene's feature word: the caller masks it to its family's bits
  bool lds_ok = false;  // the blob fits where a scene-in-LDS variant stages it (pick_variant)
};

// The scene's records on the caller's device: plan_open_device (`who`, `built`), then assemble_scene without a frame table.
static int upload_scene_records(pine_gpu_plan* p, SceneHost& H, const pine_gpu_render_params* prm, const char* who,
                                std::chrono::steady_clock::time_point& built, SceneRecords& R) {
  if (plan_open_device(p, H, prm, who, built) || assemble_scene(p, H, prm, R.parts, false)) return -1;
  R.need = scene_features(R.parts, prm);
  R.lds_ok = size_t(p->S.blob_bytes) <= 32 * 1024;
  return 0;
}
