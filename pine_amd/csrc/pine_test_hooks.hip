// pine_amd/csrc/pine_test_hooks.hip -- the device unit-test hooks of the C ABI (include/pine_gpu.h): the building blocks
// of the path kernels (scalar math, samplers, RNG, traversal, shapes) run on their own and read back, for the parity
// tests.  Built with the path kernels' flags (Makefile CXXFLAGS, -ffp-contract=off): tests/test_device_math.py relies on
// it.  The host-only hooks live in pine_host.cpp.
#include <hip/hip_runtime.h>

#include <array>
#include <cstring>
#include <type_traits>
#include <utility>

#include "pine_plan.h"
#include "pine_math_check.h"

namespace pine_gpu {

// ------------------------------------------------------------------------------------------------
// Device-side unit-test kernels (parity of the building blocks against the oracle)
// ------------------------------------------------------------------------------------------------
__global__ void test_sincos_kernel(const float* x, long long n, float* s, float* c) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i < n) {
    // the branch-free shared-reduction form the kernels call, cross-checked against the two single functions
    float sn, cs;
    psincos(x[i], sn, cs);
    const float s1 = psin(x[i]), c1 = pcos(x[i]);
    const bool same = __float_as_uint(s1) == __float_as_uint(sn) && __float_as_uint(c1) == __float_as_uint(cs);
    s[i] = same ? sn : __uint_as_float(0x7fc00001u);
    c[i] = same ? cs : __uint_as_float(0x7fc00001u);
  }
}
__global__ void test_powlog_kernel(const float* x, const float* y, long long n, float* p, float* l) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i < n) {
    p[i] = ppow(x[i], y[i]);
    l[i] = plog(x[i]);
  }
}
__global__ void test_atan_kernel(const float* y, const float* x, long long n, float* at2, float* ac) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i < n) {
    at2[i] = patan2(y[i], x[i]);
    ac[i] = pacos(x[i]);
  }
}
// pine_gpu_test_math_*: the scalar functions of pine_math.h on bit patterns (pine_math_check.h has math_eval<FN>).
// inputs from arrays (a != NULL; b, c as the arity needs) or generated: argument `swept` = first + i * stride, the others
// `fixed`.  out: n * math_width(FN) words.
template <int FN>
__global__ void test_math_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t fixed, int swept,
                                 uint32_t first, uint32_t stride, long long n, uint32_t* out) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t ua, ub = fixed, uc = fixed;
  if (a) {
    ua = a[i];
    if (math_arity(FN) > 1) ub = b[i];
    if (math_arity(FN) > 2) uc = c[i];
  } else {
    const uint32_t v = first + uint32_t(i) * stride;
    ua = swept == 0 ? v : fixed;
    ub = swept == 1 ? v : fixed;
    uc = swept == 2 ? v : fixed;
  }
  math_eval<FN>(ua, ub, uc, out + i * math_width(FN));
}
__constant__ int kTestPixels[6][2] = {{0, 0}, {1, 0}, {3, 5}, {127, 127}, {128, 5}, {639, 639}};
__global__ void test_sampler_kernel(DTables T, int spp, float* out) {
  // one thread per (pixel, pass); layout identical to oracle_sampler_stream
  const int pix = blockIdx.x;
  if (threadIdx.x != 0) return;
  float* o = out + size_t(pix) * spp * (260 + 270);
  DSampler s;
  s.px = kTestPixels[pix][0];
  s.py = kTestPixels[pix][1];
  s.dimension = 0;
  s.index = 0;
  size_t k = 0;
  for (int i = 0; i < spp; i++) {
    for (int d = 0; d < 130; d++) {
      const f2 v = sampler_get2d(T, s);
      o[k++] = v.x;
      o[k++] = v.y;
    }
    s.dimension = 0;
    s.index++;
  }
  s.index = 0;
  for (int i = 0; i < spp; i++) {
    for (int d = 0; d < 90; d++) {
      o[k++] = sampler_get1d(T, s);
      const f2 v = sampler_get2d(T, s);
      o[k++] = v.x;
      o[k++] = v.y;
    }
    s.dimension = 0;
    s.index++;
  }
}
__global__ void test_rng_kernel(unsigned long long* out) {
  const int pix = threadIdx.x;
  if (pix >= 6) return;
  unsigned long long* o = out + pix * 19;
  const uint64_t h = hash_pixel(kTestPixels[pix][0], kTestPixels[pix][1], 0);
  o[0] = h;
  DRng g = rng_seed(h);
  o[1] = g.s0;
  o[2] = g.s1;
  for (int i = 0; i < 16; i++) o[3 + i] = (unsigned long long)(uint32_t)as_int(rng_nextf(g));
}
// The primitives a ray's traversal tests, in order, and its result: the nested loops of the scene-in-LDS variants
// (FLAT = false: scene_traverse / mesh_traverse) or the flat state machine of the F_LDS_TOP variants (pine_trav.h).
// One thread per ray, 64 per block; out: per ray `cap` words closest (count, words...), 4 result words (hit, geometry,
// triangle, tmax bits), `cap` words any-hit, 1 result word.
// (MODE 2: the closest-hit query in EmbreeAccel's order, PINE_GPU_FLAG_ORDER_EMBREE; the any-hit query is the nested loops')
template <int MODE>
__global__ void __launch_bounds__(64) test_traverse_kernel(DeviceScene S, const float* rays, long long nrays, int cap, unsigned* out) {
  constexpr bool FLAT = MODE == 1;
  constexpr unsigned F = FLAT ? (F_ALL | F_LDS_TOP) : MODE == 2 ? (F_ALL | F_EMBREE) : F_ALL;
  using StackT = typename std::conditional<FLAT, unsigned short, int>::type;
  extern __shared__ __attribute__((aligned(16))) int lds_raw[];
  StackT* const stack = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;
  const SceneView V = scene_view_global(S);
  const long long i = blockIdx.x * 64ll + threadIdx.x;
  const bool live = i < nrays;
  const float* q = rays + (live ? i : 0) * 8;
  unsigned* o = out + (live ? i : 0) * (2ll * cap + 5);
  for (int pass = 0; pass < 2; pass++) {
    DRay ray{f3{q[0], q[1], q[2]}, f3{q[3], q[4], q[5]}, q[6], q[7]};
    TravLog log{o + (pass ? cap + 4 : 0) + 1, 0, cap - 1};
    bool hit = false;
    int geom = 0, prim = 0;
    if constexpr (FLAT) {
      TravState ts;
      trav_begin(V, ts);
      if (!live) ts.done = 1;
      const DRayOct oct = make_oct(ray);
      if (pass == 0) trav_trips<false, F, 64>(V, ray, oct, ts, stack, 0, 1 << 30, nullptr, &log);
      else trav_trips<true, F, 64>(V, ray, oct, ts, stack, 0, 1 << 30, nullptr, &log);
      hit = ts.hit_geom >= 0;
      geom = ts.hit_geom, prim = ts.hit_prim;
    } else if (live) {
      hit = pass == 0 ? scene_traverse<false, F, 64>(V, ray, stack, geom, prim, &log) : scene_traverse<true, F, 64>(V, ray, stack, geom, prim, &log);
    }
    if (live) {
      o[pass ? cap + 4 : 0] = unsigned(log.n);
      if (pass == 0) {
        o[cap] = hit ? 1u : 0u;
        o[cap + 1] = hit ? unsigned(geom & kPrimIndexMask) : 0u;
        // (a mesh hit reports the triangle's index within its mesh, as the reference does; elsewhere the word is unused: 0)
        const bool on_mesh = hit && (geom >> kPrimKindShift) == SHAPE_MESH;
        o[cap + 2] = on_mesh ? unsigned(prim - S.bvhs[as_int(S.shapes[geom & kPrimIndexMask].f[2])].prim_base) : 0u;
        o[cap + 3] = __float_as_uint(ray.tmax);
      } else {
        o[2 * cap + 4] = hit ? 1u : 0u;
      }
    }
  }
}
__global__ void test_shapes_kernel(const DShape* shapes, int num_shapes, const float* rays, long long nrays,
                                   float* out) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= nrays * num_shapes) return;
  const int g = int(i / nrays);
  const long long r = i % nrays;
  const float* q = rays + r * 8;
  DRay ray{f3{q[0], q[1], q[2]}, f3{q[3], q[4], q[5]}, q[6], q[7]};
  float* o = out + i * 11;
  const DShape* S = &shapes[g];
  o[0] = shape_hit(S, ray) ? 1.0f : 0.0f;
  DRay r2 = ray;
  const bool h = shape_intersect(S, r2);
  o[1] = h ? 1.0f : 0.0f;
  o[2] = r2.tmax;
  DSurface it;
  it.p = it.n = mk3(0.0f);
  it.uv = f2{0, 0};
  if (h) shape_surface_info(S, ray_at(r2, r2.tmax), it);
  o[3] = it.p.x, o[4] = it.p.y, o[5] = it.p.z;
  o[6] = it.n.x, o[7] = it.n.y, o[8] = it.n.z;
  o[9] = it.uv.x, o[10] = it.uv.y;
}
}  // namespace pine_gpu

using namespace pine_gpu;

extern "C" {

int pine_gpu_plan_test_traverse_baked(pine_gpu_plan* p, const float* rays, int64_t nrays, uint32_t* out) {
  if (!p || !rays || !out || nrays <= 0) {
    set_error("null argument");
    return -1;
  }
  if (!p->spec_module || !p->spec_baked) {
    set_error("the plan has no baked scene (PINE_GPU_FLAG_SPECIALIZE, a scene that qualifies)");
    return -1;
  }
  HIP_OK(hipSetDevice(p->device));
  hipFunction_t fn;
  HIP_OK(hipModuleGetFunction(&fn, p->spec_module, "pine_baked_traverse_test"));
  float* dr = nullptr;
  unsigned* dout = nullptr;
  int rc = -1;
  do {
    if (hipMalloc((void**)&dr, size_t(nrays) * 32) != hipSuccess || hipMalloc((void**)&dout, size_t(nrays) * 16) != hipSuccess) break;
    if (hipMemcpy(dr, rays, size_t(nrays) * 32, hipMemcpyHostToDevice) != hipSuccess) break;
    long long n = nrays;
    void* args[] = {&dr, &n, &dout};
    if (hipModuleLaunchKernel(fn, unsigned((nrays + 63) / 64), 1, 1, 64, 1, 1, 0, nullptr, args, nullptr) != hipSuccess) break;
    if (hipMemcpy(out, dout, size_t(nrays) * 16, hipMemcpyDeviceToHost) != hipSuccess) break;
    rc = 0;
  } while (0);
  if (rc) set_error(std::string("pine_gpu_plan_test_traverse_baked: ") + hipGetErrorString(hipGetLastError()));
  (void)hipFree(dr);
  (void)hipFree(dout);
  return rc;
}

// ---- device unit-test hooks -------------------------------------------------------------------
int pine_gpu_test_sincos(int device, const float* x, int64_t n, float* s, float* c) {
  if (need_device(device)) return -1;
  float *dx, *ds, *dc;
  HIP_OK(hipMalloc((void**)&dx, n * 4));
  HIP_OK(hipMalloc((void**)&ds, n * 4));
  HIP_OK(hipMalloc((void**)&dc, n * 4));
  HIP_OK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(test_sincos_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, 0, dx, (long long)n, ds, dc);
  HIP_OK(hipMemcpy(s, ds, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(c, dc, n * 4, hipMemcpyDeviceToHost));
  hipFree(dx);
  hipFree(ds);
  hipFree(dc);
  return 0;
}
int pine_gpu_test_powlog(int device, const float* x, const float* y, int64_t n, float* pw, float* lg) {
  if (need_device(device)) return -1;
  float *dx, *dy, *dp, *dl;
  HIP_OK(hipMalloc((void**)&dx, n * 4));
  HIP_OK(hipMalloc((void**)&dy, n * 4));
  HIP_OK(hipMalloc((void**)&dp, n * 4));
  HIP_OK(hipMalloc((void**)&dl, n * 4));
  HIP_OK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dy, y, n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(test_powlog_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, 0, dx, dy, (long long)n, dp, dl);
  HIP_OK(hipMemcpy(pw, dp, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(lg, dl, n * 4, hipMemcpyDeviceToHost));
  hipFree(dx);
  hipFree(dy);
  hipFree(dp);
  hipFree(dl);
  return 0;
}
int pine_gpu_test_atan(int device, const float* y, const float* x, int64_t n, float* at2, float* ac) {
  if (need_device(device)) return -1;
  float *dy, *dx, *da, *dc;
  HIP_OK(hipMalloc((void**)&dy, n * 4));
  HIP_OK(hipMalloc((void**)&dx, n * 4));
  HIP_OK(hipMalloc((void**)&da, n * 4));
  HIP_OK(hipMalloc((void**)&dc, n * 4));
  HIP_OK(hipMemcpy(dy, y, n * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(test_atan_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, 0, dy, dx, (long long)n, da, dc);
  HIP_OK(hipMemcpy(at2, da, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(ac, dc, n * 4, hipMemcpyDeviceToHost));
  hipFree(dy);
  hipFree(dx);
  hipFree(da);
  hipFree(dc);
  return 0;
}

// ---- pine_gpu_test_math_*: the scalar functions over bit patterns against their references (pine_math_check.h) -----
extern "C++" {
namespace {
template <int FN>
void math_launch(const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t fixed, int swept, uint32_t first,
                 uint32_t stride, long long n, uint32_t* out) {
  hipLaunchKernelGGL(test_math_kernel<FN>, dim3(unsigned((n + 255) / 256)), dim3(256), 0, 0, a, b, c, fixed, swept, first,
                     stride, n, out);
}
using MathLaunch = void (*)(const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, int, uint32_t, uint32_t, long long,
                            uint32_t*);
template <int... FN>
constexpr std::array<MathLaunch, sizeof...(FN)> math_launch_table(std::integer_sequence<int, FN...>) {
  return {math_launch<FN>...};
}
constexpr std::array<MathLaunch, PINE_GPU_MATH_COUNT> kMathLaunch =
    math_launch_table(std::make_integer_sequence<int, PINE_GPU_MATH_COUNT>());
}  // namespace
}  // extern "C++"

int pine_gpu_test_math_eval(int device, int fn, const uint32_t* a, const uint32_t* b, const uint32_t* c, int64_t n, uint32_t* got) {
  if (device < 0) return math_check::eval_host_arrays(fn, a, b, c, n, got);
  if (math_check::bad_args(fn, n, a, b, c)) return -1;
  if (!got) {
    set_error("bad argument");
    return -1;
  }
  if (need_device(device)) return -1;
  const int w = math_width(fn), ar = math_arity(fn);
  const int64_t m = std::max<int64_t>(1, std::min(n, math_check::kChunk));
  uint32_t* d[4] = {nullptr, nullptr, nullptr, nullptr};
  int rc = 0;
  for (int k = 0; k < 4 && !rc; k++)
    if ((k < ar || k == 3) && hipMalloc((void**)&d[k], m * 4 * (k == 3 ? w : 1)) != hipSuccess) rc = -1;
  const uint32_t* src[3] = {a, b, c};
  for (int64_t i0 = 0; i0 < n && !rc; i0 += m) {
    const int64_t len = std::min(m, n - i0);
    for (int k = 0; k < ar && !rc; k++)
      if (hipMemcpy(d[k], src[k] + i0, len * 4, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    if (rc) break;
    kMathLaunch[size_t(fn)](d[0], d[1], d[2], 0u, 0, 0u, 0u, (long long)len, d[3]);
    if (hipGetLastError() != hipSuccess || hipMemcpy(got + i0 * w, d[3], len * 4 * w, hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
  }
  for (int k = 0; k < 4; k++)
    if (d[k]) hipFree(d[k]);
  if (rc) {
    set_error(std::string("pine_gpu_test_math_eval: ") + hipGetErrorString(hipGetLastError()));
    return -1;
  }
  return 0;
}

int pine_gpu_test_math_sweep(int device, int fn, uint32_t fixed_bits, int swept_arg, uint32_t first, uint64_t count, uint32_t stride,
                             int64_t* stats, uint32_t* examples, int cap) {
  if (device < 0) return math_check::sweep_host(fn, fixed_bits, swept_arg, first, count, stride, stats, examples, cap);
  if (math_check::bad_sweep_args(fn, swept_arg, count, stats, examples, cap) || need_device(device)) return -1;
  const int w = math_width(fn);
  const int64_t m = std::max<int64_t>(1, std::min<int64_t>(int64_t(count), math_check::kChunk));
  uint32_t* h = nullptr;  // one chunk's results, pinned for the copies
  uint32_t* d = nullptr;
  HIP_OK(hipHostMalloc((void**)&h, m * w * 4, hipHostMallocDefault));
  if (hipMalloc((void**)&d, m * w * 4) != hipSuccess) {
    hipHostFree(h);
    set_error("pine_gpu_test_math_sweep: out of device memory");
    return -1;
  }
  const math_check::ChunkEval on_device = [&](uint32_t start, int64_t len, uint32_t* out) {
    kMathLaunch[size_t(fn)](nullptr, nullptr, nullptr, fixed_bits, swept_arg, start, stride, (long long)len, d);
    if (hipGetLastError() != hipSuccess || hipMemcpy(out, d, len * w * 4, hipMemcpyDeviceToHost) != hipSuccess) {
      set_error(std::string("pine_gpu_test_math_sweep: ") + hipGetErrorString(hipGetLastError()));
      return -1;
    }
    return 0;
  };
  const int rc = math_check::sweep(fn, fixed_bits, swept_arg, first, count, stride, on_device, h, stats, examples, cap);
  hipFree(d);
  hipHostFree(h);
  return rc;
}

int pine_gpu_test_sampler(int device, int spp_req, float* out, int64_t capacity) {
  if (need_device(device)) return -1;
  TableBlob tables_blob;
  if (load_tables(tables_blob)) return -1;
  const std::vector<uint8_t>& g_tables = *tables_blob;
  const int spp = effective_spp(spp_req);
  const int64_t need = int64_t(6) * spp * (260 + 270);
  if (capacity < need) {
    set_error("capacity too small");
    return -1;
  }
  int k = 0;
  while ((1 << k) < spp) k++;
  uint8_t* dt;
  float* dout;
  HIP_OK(hipMalloc((void**)&dt, 65536 + 262144));
  {
    const std::vector<uint8_t> st = transposed_sobol(g_tables);
    HIP_OK(hipMemcpy(dt, st.data(), 65536, hipMemcpyHostToDevice));
  }
  HIP_OK(hipMemcpy(dt + 65536, g_tables.data() + 65536 + size_t(k) * 262144, 262144, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc((void**)&dout, need * 4));
  DTables T{dt, dt + 65536, dt + 65536 + 131072, nullptr, nullptr, 0};
  hipLaunchKernelGGL(test_sampler_kernel, dim3(6), dim3(64), 0, 0, T, spp, dout);
  HIP_OK(hipMemcpy(out, dout, need * 4, hipMemcpyDeviceToHost));
  hipFree(dt);
  hipFree(dout);
  return 0;
}
int pine_gpu_test_rng(int device, uint64_t* out, int64_t capacity) {
  if (need_device(device)) return -1;
  if (capacity < 6 * 19) {
    set_error("capacity too small");
    return -1;
  }
  unsigned long long* d;
  HIP_OK(hipMalloc((void**)&d, 6 * 19 * 8));
  hipLaunchKernelGGL(test_rng_kernel, dim3(1), dim3(64), 0, 0, d);
  HIP_OK(hipMemcpy(out, d, 6 * 19 * 8, hipMemcpyDeviceToHost));
  hipFree(d);
  return 0;
}
int pine_gpu_test_traverse(pine_gpu_scene* scene, int device, const float* rays, int64_t nrays, int flat, int cap, uint32_t* out) {
  if (!scene || !rays || !out || cap < 2 || nrays < 0) {
    set_error("bad argument");
    return -1;
  }
  if (need_device(device)) return -1;
  // the scene as the kernels see it: a plan's device records (nothing is rendered)
  pine_gpu_render_params prm{};
  prm.spp = 1, prm.max_path_length = 2, prm.device = device, prm.shard_rank = 0, prm.shard_world = 1;
  prm.flags = PINE_GPU_FLAG_NO_SPECIALIZE | (flat == 2 ? PINE_GPU_FLAG_ORDER_EMBREE : 0);
  pine_gpu_plan* p = pine_gpu_plan_create(scene, &prm);
  if (!p) return -1;
  int rc = -1;
  float* dr = nullptr;
  unsigned* dout = nullptr;
  const size_t words = size_t(nrays) * (2 * size_t(cap) + 5);
  do {
    if (flat == 1 && p->S.stack_total > 0 && scene_host(scene).accel.nodes.size() > 65535) {
      set_error("the flat traversal keeps 16-bit node ids");
      break;
    }
    if (hipMalloc((void**)&dr, std::max<int64_t>(nrays, 1) * 32) != hipSuccess || hipMalloc((void**)&dout, std::max<size_t>(words, 1) * 4) != hipSuccess) break;
    if (hipMemcpy(dr, rays, nrays * 32, hipMemcpyHostToDevice) != hipSuccess || hipMemset(dout, 0, std::max<size_t>(words, 1) * 4) != hipSuccess) break;
    const size_t lds = size_t(std::max(1, p->S.stack_total)) * 64 * (flat == 1 ? sizeof(unsigned short) : sizeof(int));
    if (nrays > 0) {
      if (flat == 1) hipLaunchKernelGGL(test_traverse_kernel<1>, dim3(unsigned((nrays + 63) / 64)), dim3(64), lds, 0, p->S, dr, (long long)nrays, cap, dout);
      else if (flat == 2) hipLaunchKernelGGL(test_traverse_kernel<2>, dim3(unsigned((nrays + 63) / 64)), dim3(64), lds, 0, p->S, dr, (long long)nrays, cap, dout);
      else hipLaunchKernelGGL(test_traverse_kernel<0>, dim3(unsigned((nrays + 63) / 64)), dim3(64), lds, 0, p->S, dr, (long long)nrays, cap, dout);
    }
    if (hipMemcpy(out, dout, words * 4, hipMemcpyDeviceToHost) != hipSuccess) break;
    rc = 0;
  } while (0);
  if (rc) set_error(std::string("pine_gpu_test_traverse: ") + hipGetErrorString(hipGetLastError()));
  (void)hipFree(dr);
  (void)hipFree(dout);
  pine_gpu_plan_destroy(p);
  return rc;
}

int pine_gpu_test_shapes(pine_gpu_scene* scene, int device, const float* rays, int64_t nrays, float* out,
                         int64_t capacity) {
  if (!scene || !rays || !out) {
    set_error("null argument");
    return -1;
  }
  if (need_device(device)) return -1;
  SceneHost& H = scene_host(scene);
  std::vector<DShape> shapes;
  for (auto& g : H.geometries)
    if (g.shape.kind != SHAPE_MESH) shapes.push_back(g.shape);
  const int64_t need = int64_t(shapes.size()) * nrays * 11;
  if (capacity < need) {
    set_error("capacity too small");
    return -1;
  }
  DShape* ds;
  float *dr, *dout;
  if (upload(ds, shapes)) return -1;
  HIP_OK(hipMalloc((void**)&dr, nrays * 32));
  HIP_OK(hipMemcpy(dr, rays, nrays * 32, hipMemcpyHostToDevice));
  HIP_OK(hipMalloc((void**)&dout, std::max<int64_t>(need, 1) * 4));
  const long long total = (long long)shapes.size() * nrays;
  if (total > 0)
    hipLaunchKernelGGL(test_shapes_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, 0, ds,
                       int(shapes.size()), dr, (long long)nrays, dout);
  HIP_OK(hipMemcpy(out, dout, need * 4, hipMemcpyDeviceToHost));
  hipFree(ds);
  hipFree(dr);
  hipFree(dout);
  return 0;
}

}  // extern "C"
