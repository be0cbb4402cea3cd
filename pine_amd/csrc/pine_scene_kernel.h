// pine_amd/csrc/pine_scene_kernel.h -- a plan's scene kernel and its one owner (SceneKernel): request, build, load, adopt.
// The half that needs HIP (pine_plan.h includes it after HIP_OK); the generator, the cache, the compile step and the background
// queue are pine_specialize.h.
//
// Scene-specialised kernels: the stage-queued kernel compiled FOR THIS SCENE.
//  (1) its exact feature set: the precompiled variants are a handful of supersets (pine_variants.h) -- a scene of spheres
//      under a point light runs the everything-but-Subsurface kernel and pays for every shape kind, node programs and the
//      Sobol sampler in registers (38 spilled VGPRs).
//  (2) if the scene has no meshes and its BVH is small enough to unroll: the BVH and primitive records baked in; one mesh
//      under a small top level: the top level as code (bake_scene).
// Nothing to gain (the variant IS the exact set, nothing to bake): the precompiled kernel runs.
//
// Modes.  AUTOMATIC (no flag): never in the caller's way -- a code object already in the cache is loaded at plan creation (about a
// millisecond); otherwise the compiler runs in the BACKGROUND (a process-wide queue of at most kSpecWorkers compiler children,
// keyed by content, shared by every plan that wants the same kernel and outliving the plan that asked first) while the precompiled
// kernel renders; the first launch after the build has finished -- of this plan or of any later plan of the same geometry -- runs
// the scene's own kernel.  Nothing can fail because of it: no compiler, no headers, no cache directory, a full queue all leave
// the precompiled kernel in place (plan stats: specialized 0 or -1).  EXPLICIT, PINE_GPU_FLAG_SPECIALIZE (or $PINE_GPU_SPECIALIZE=1):
// the caller WANTS the scene's kernel -- plan creation waits for the compiler and a kernel that cannot be built fails the plan;
// EXPLICIT ASYNC, with _ASYNC: the build runs in the background as above but a failure is still reported (specialized == -1).
// PINE_GPU_FLAG_NO_SPECIALIZE / $PINE_GPU_SPECIALIZE=0: precompiled only (nothing is requested).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pine_gpu.h"
#include "pine_device.h"
#include "pine_specialize.h"
#include "pine_variants.h"

namespace pine_gpu {
static_assert(kBakedFeature == F_BAKED, "pine_specialize.h restates the bit for host code that cannot include pine_device.h");
enum : int { kSpecSourceNone = 0, kSpecSourceCache = 1, kSpecSourceCompiledHere = 2, kSpecSourceBackground = 3 };  // plan stats' specialize_source

// A code object loaded into a device's context, shared by the plans that run it: hipModuleLoadData of a scene's kernel is a
// millisecond or two, which a one-shot render (create, launch, destroy) of the same geometry would pay on every call.  The
// process keeps the last kMaxLoaded of them per (device, content key); a module is unloaded when the table has dropped it and
// the last plan that launches it is gone.
struct LoadedKernel {
  int device = 0;
  std::string key, image;  // (the image is kept for the module's lifetime: the runtime may build the program lazily from it)
  hipModule_t module = nullptr;
  hipFunction_t fn = nullptr;
  ~LoadedKernel() {
    if (module) {
      int keep = 0;
      (void)hipGetDevice(&keep);
      (void)hipSetDevice(device);
      (void)hipModuleUnload(module);
      (void)hipSetDevice(keep);
    }
  }
};
struct LoadedKernels {
  static constexpr size_t kMaxLoaded = 16;
  std::mutex mu;
  std::deque<std::shared_ptr<LoadedKernel>> recent;
  static LoadedKernels& get() {
    static LoadedKernels* q = new LoadedKernels();  // (never destroyed: unloading modules while the runtime goes down is not safe)
    return *q;
  }
  std::shared_ptr<LoadedKernel> find(int device, const std::string& key) {
    std::lock_guard<std::mutex> lock(mu);
    for (auto& k : recent)
      if (k->device == device && k->key == key) return k;
    return nullptr;
  }
  void remember(const std::shared_ptr<LoadedKernel>& k) {
    std::lock_guard<std::mutex> lock(mu);
    recent.push_front(k);
    if (recent.size() > kMaxLoaded) recent.pop_back();
  }
  void clear() {  // (a module is unloaded when the last plan that launches it is gone)
    std::lock_guard<std::mutex> lock(mu);
    recent.clear();
  }
};

// The scene kernel of one plan.  Used by the thread that uses the plan (a plan is rendered from one thread at a time,
// pine_gpu.h); what crosses threads is a job's state, which the queue's workers publish through SpecJob's atomics.
class SceneKernel {
 public:
  enum class Mode { kAutomatic, kExplicitAsync, kExplicit };
  // Plan creation, once, with what it has decided: the mode, the chosen stage-queued variant `V`, the features `need` that
  // plan_build found in the scene, whether the scene may be baked, $PINE_GPU_SPECIALIZE_FORCE (experiments through
  // $PINE_GPU_SPECIALIZE_EXTRA).  Decides whether the scene has a kernel of its own to gain, generates and looks it up, then
  // adopts it from the cache, compiles it here (kExplicit) or queues a background build.  -1 with the error set only where the
  // caller asked for the kernel: it cannot be looked up, or (kExplicit) built or loaded.  `words`: SceneHost::packed_prim_words.
  int request(Mode mode, int device, const PineKernelVariant& V, unsigned need, bool may_bake, bool force, const FlatAccel& A,
              const std::vector<DShape>& shapes, const std::vector<int>& words) {
    t0_ = std::chrono::steady_clock::now();
    // (the LDS layout flags, and F_SSS, which sizes the per-context records, stay the variant's: every buffer size computed from it stays right)
    const unsigned kLayout = F_LDS_SCENE | F_LDS_TOP | F_LDS_REST | F_XSTAGE | F_SSS;
    unsigned exact = (V.features & kLayout) | need;
    BakedScene baked;
    if (may_bake) baked = bake_scene(A, shapes, words, (V.features & F_XSTAGE) != 0);
    if (baked.form == BakedForm::kNone && exact == V.features && !force) return 0;
    if (baked.form != BakedForm::kNone) exact |= F_BAKED;
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, device));
    std::string arch = prop.gcnArchName;  // "gfx950:sramecc+:xnack-" -> "gfx950"
    if (arch.find(':') != std::string::npos) arch = arch.substr(0, arch.find(':'));
    mode_ = mode, device_ = device, form_ = baked.form;
    request_.baked = std::move(baked.text), request_.features = exact, request_.ctx = V.ctx, request_.arch = arch;
    std::string err;
    const int found = kernel_cache_lookup(request_, err);
    if (found >= 0) return obtain(found);
    if (mode_ != Mode::kAutomatic) return set_error(err), -1;
    request_ = KernelRequest(), form_ = BakedForm::kNone;  // (no headers / no cache directory: the precompiled kernel it is)
    return 0;
  }
  // Has the background build finished?  Called by every launch and by stats_get: the next launch runs the scene's kernel.
  // (A build that failed, or a code object the runtime refuses, leaves the precompiled kernel in place: same film.)
  void poll() {
    if (state_ != State::kBuilding || waiter_->state.load() == kSpecBuilding) return;
    if (waiter_->state.load() == kSpecBuilt && load() == hipSuccess) adopted();
    else state_ = State::kFailed;
    waiter_.reset();
  }
  hipFunction_t fn() const { return loaded_ ? loaded_->fn : nullptr; }  // null: the precompiled variant launches
  hipModule_t module() const { return loaded_ ? loaded_->module : nullptr; }
  hipModule_t baked_module() const { return form_ != BakedForm::kNone ? module() : nullptr; }  // (test hook: pine_baked_traverse_test)
  // the kernel asked for -- adopted yet or not -- has the top level as code: schedule_params sets the traversal stages up for it
  bool baked_top_requested() const { return form_ == BakedForm::kTop; }
  // specialized, specialize_source, specialize_pending, kernel_features, specialize_ms (`precompiled`: the variant's features)
  void fill_stats(pine_gpu_plan_stats* out, unsigned precompiled) const {
    const bool building = state_ == State::kBuilding;
    out->specialized = loaded_ ? (form_ != BakedForm::kNone ? 2 : 1) : state_ == State::kFailed ? -1 : 0;
    out->specialize_source = loaded_ || building ? source_ : kSpecSourceNone;
    out->specialize_pending = building ? 1 : 0;
    out->kernel_features = loaded_ ? request_.features : precompiled;
    out->specialize_ms = ms_;
  }

 private:
  // kNone: nothing asked for, or nothing to be had without getting in the caller's way.  kBuilding: `waiter_` holds a job of the
  // background queue.  kAdopted: `loaded_` launches.  kFailed: the precompiled kernel stays, and stats say so.
  enum class State { kNone, kBuilding, kAdopted, kFailed };
  // From kernel_cache_lookup's answer `found` (0 / 1) to a kernel that launches, a queued build, or a failure.
  // A cached code object the runtime refuses (cut short by a full disk, another ROCm's output) is, once, dropped and unlinked
  // -- a packaged one that cannot be removed (a read-only install) is bypassed for the user's cache -- and looked up again;
  // then the modes go their ways as after any lookup: a file that is there is loaded; one that is not is compiled here
  // (kExplicit, failing the plan if that cannot be done or the result is refused) or built in the background.
  int obtain(int found) {
    const bool wait = mode_ == Mode::kExplicit;
    source_ = found == 1 ? kSpecSourceCache : kSpecSourceCompiledHere;
    for (int attempt = 0; found == 1 || wait; attempt++) {
      std::string err;
      const bool from_cache = found == 1;
      if (!from_cache && !kernel_compile(request_, err)) return set_error(err), -1;
      const hipError_t e = load();
      if (e == hipSuccess) return adopted(), 0;
      err = "scene specialisation: the runtime does not load " + request_.path + " (" + hipGetErrorString(e) + ")";
      if (attempt == 0 && from_cache) {
        const bool skip_packaged = unlink(request_.path.c_str()) != 0;
        found = kernel_cache_lookup(request_, err, skip_packaged);
        if (found >= 0) continue;
      }
      set_error(err);
      if (!wait) state_ = State::kFailed;
      return wait ? -1 : 0;
    }
    // the compiler runs beside the first renders (host work only: files and a child process); a launch adopts the kernel once
    // it is there.  Until then -- and for good if the build fails -- the precompiled kernel renders the same film.
    source_ = kSpecSourceBackground;
    waiter_ = SpecQueue::get().submit(request_, mode_ != Mode::kAutomatic);
    // (a full queue: the automatic mode says nothing, a caller who asked is told)
    state_ = waiter_ ? State::kBuilding : mode_ != Mode::kAutomatic ? State::kFailed : State::kNone;
    return 0;
  }
  // request_.path into this device's context (or the copy already there)
  hipError_t load() {
    if ((loaded_ = LoadedKernels::get().find(device_, request_.key))) return hipSuccess;
    auto k = std::make_shared<LoadedKernel>();
    k->device = device_, k->key = request_.key;
    hipError_t e = hipErrorInvalidImage;
    if (read_file(request_.path, k->image) && code_object_is_whole(k->image)) {
      e = hipModuleLoadData(&k->module, k->image.data());
      if (e == hipSuccess) e = hipModuleGetFunction(&k->fn, k->module, kernel_symbol(request_.features, request_.ctx).c_str());
    }
    if (e == hipSuccess) LoadedKernels::get().remember(loaded_ = k);
    else (void)hipGetLastError();  // (k unloads what was loaded)
    return e;
  }
  void adopted() { state_ = State::kAdopted, ms_ = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0_).count(); }
  Mode mode_ = Mode::kAutomatic;
  State state_ = State::kNone;
  int device_ = 0, source_ = kSpecSourceNone;  // (source: where the kernel came / comes from)
  KernelRequest request_;                      // what to compile, and where its code object lives
  BakedForm form_ = BakedForm::kNone;
  std::shared_ptr<LoadedKernel> loaded_;  // (shared with every plan of this geometry on this device: LoadedKernels)
  SpecWaiter waiter_;                     // the plan's share of a background job, given back when the job ends or the plan does
  std::chrono::steady_clock::time_point t0_;
  float ms_ = 0.0f;  // generating + compiling (or fetching from the cache) + loading: from request() to adoption
};

}  // namespace pine_gpu
