// pine_amd/csrc/pine_radiance.h -- the kernel prologue and the per-vertex steps of radiance() (path.cpp:42-124), written once.
//
// The prologue (scene_view_global / _staged, stage_sobol_rows, lane_tables, load_lane_slice) serves every kernel that
// traces: the two path kernels, the AO kernel and the traversal test hook.
//
// Every film has to match the reference bit for bit: each path vertex runs the same floating-point operations, the same
// sampler draws and the same RNG draws in the same order as the reference.  That sequence lives HERE; the two path kernels
// (path_trace_kernel in pine_kernels_device.h, path_queue_body in pine_queue_kernel.h) only decide when a step runs and
// where its state is kept -- a step of the BSSRDF walk included (walk_begin, walk_step, walk_exit).  The functions take what they need as arguments -- SceneView, scalar fields of DeviceScene,
// DTables, DSampler&, DRng& or load / store callables -- and know nothing about queues, contexts, LDS layouts or lane
// state.  All are force-inlined: a caller's constant arguments fold, and a callable costs nothing.
// Included by pine_kernels_device.h after SceneView, PackedState and material_le.
#pragma once

namespace pine_gpu {

// ---- the kernel prologue: the scene view and the sampler's LDS front, for every kernel that traces ----

// EmbreeAccel's hierarchy and mesh list (F_EMBREE variants read them) in a scene blob at `base`.
__device__ __forceinline__ void view_of_embree_order(const char* base, const DeviceScene& S, SceneView& V) {
  V.etree = reinterpret_cast<const EmbreeNode*>(base + S.off_etree);
  V.emesh = reinterpret_cast<const int*>(base + S.off_emesh);
}

// SceneView over a scene blob (DeviceScene::blob and its off_* offsets) staged at `base`.  The nodes and the reciprocal
// table are the caller's: not every kernel stages them with the rest.
__device__ __forceinline__ void view_of_blob(const char* base, const DeviceScene& S, SceneView& V) {
  V.shapes = reinterpret_cast<const DShape*>(base + S.off_shapes);
  V.materials = reinterpret_cast<const DMaterial*>(base + S.off_materials);
  V.bvhs = reinterpret_cast<const DBvh*>(base + S.off_bvhs);
  V.lights = reinterpret_cast<const DLight*>(base + S.off_lights);
  V.node_ops = reinterpret_cast<const DNodeOp*>(base + S.off_node_ops);
  V.leaf = reinterpret_cast<const DShape*>(base + S.off_leaf) - S.top_prim_begin;
  view_of_embree_order(base, S, V);
  V.frames = reinterpret_cast<const float*>(base + S.off_frames);
  V.frame_base = reinterpret_cast<const int*>(base + S.off_frame_base);
}

// The scene where the host put it: every field of the view from the DeviceScene's global-memory pointers, nothing in LDS.
// Every kernel's view starts here, so a new SceneView field is set in this one place.
__device__ __forceinline__ SceneView scene_view_global(const DeviceScene& S) {
  SceneView V;
  V.leaf = S.leaf;
  V.shapes = S.shapes;
  V.materials = S.materials;
  V.nodes = S.nodes;
  V.env = S.env;
  V.tex = S.tex;
  V.bvhs = S.bvhs;
  V.lights = S.lights;
  V.tri_verts = S.tri_verts;
  V.node_ops = S.node_ops;
  V.stack_top = S.stack_top;
  V.num_shapes = S.num_shapes;
  V.tri_leaf = S.tri_leaf;
  V.tri_attrs = S.tri_attrs;
  V.lds_nodes = nullptr;
  V.lds_node_count = 0;
  V.lds_tri_entries = nullptr;
  V.lds_tri_verts = nullptr;
  view_of_embree_order(reinterpret_cast<const char*>(S.blob), S, V);
  V.etree_root = S.etree_root;
  V.num_emesh = S.num_emesh;
  V.frames = reinterpret_cast<const float*>(reinterpret_cast<const char*>(S.blob) + S.off_frames);
  V.frame_base = reinterpret_cast<const int*>(reinterpret_cast<const char*>(S.blob) + S.off_frame_base);
  V.has_frames = S.off_frames != 0;
  V.rcpps = reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(S.blob) + S.off_rcpps);
  return V;
}

// F_LDS_SCENE: the workgroup copies the scene blob to `dst` (LDS, 16-byte words, thread tid of nthreads) and gets the view
// over the copy.  The reciprocal table moves with it when the host put it inside the staged part.  The caller's
// __syncthreads() comes before the first read.
__device__ __forceinline__ SceneView scene_view_staged(const DeviceScene& S, uint4* dst, unsigned tid, int nthreads) {
  const int n16 = S.blob_bytes >> 4;
  for (int i = tid; i < n16; i += nthreads) dst[i] = S.blob[i];
  SceneView V = scene_view_global(S);
  const char* base = reinterpret_cast<const char*>(dst);
  V.nodes = reinterpret_cast<const DNode*>(base + S.off_nodes);
  view_of_blob(base, S, V);
  if (S.off_rcpps < S.blob_bytes) V.rcpps = reinterpret_cast<const unsigned*>(base + S.off_rcpps);
  return V;
}

// The transposed Sobol table's rows of the dimensions the LDS front serves, to `dst` (LDS) over the workgroup.
__device__ __forceinline__ void stage_sobol_rows(int* dst, const DTables& tables, unsigned tid, int nthreads) {
  const uint4* src = reinterpret_cast<const uint4*>(tables.sobol);
  for (int i = tid; i < kLdsSamplerDims * 256 / 16; i += nthreads) reinterpret_cast<uint4*>(dst)[i] = src[i];
}

// The sampler tables as a lane of a 256-thread workgroup sees them: the staged Sobol rows, and the lane's own slice
// ([dword][lane] from lds_tile_base: 10 dwords of ranking bytes, 2 of scrambling bytes) that load_lane_slice fills.
__device__ __forceinline__ DTables lane_tables(const DTables& tables, const int* lds_sobol, uint32_t* lds_tile_base, unsigned tid) {
  DTables T = tables;
  T.lds_sobol = reinterpret_cast<const uint8_t*>(lds_sobol);
  T.lds_tile = lds_tile_base + tid;
  T.lds_scr = lds_tile_base + tid + 10 * kLdsLaneStride;
  T.tile_stride = kLdsLaneStride;
  T.win_lo = 0;
  T.win_len = kLdsSamplerDims;
  return T;
}

// This lane's sampler slice for pixel (px, py): its 40 ranking bytes and 8 scrambling bytes.
__device__ __forceinline__ void load_lane_slice(const DTables& tables, int px, int py, uint32_t* lds_tile_base, unsigned tid) {
  const int pix = (px & 127) + (py & 127) * 128;
  const uint2* rsrc = reinterpret_cast<const uint2*>(tables.rank + size_t(pix) * 8);
  const uint2 sc = *reinterpret_cast<const uint2*>(tables.scramble + size_t(pix) * 8);
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const uint2 r = rsrc[j];
    lds_tile_base[(2 * j) * kLdsLaneStride + tid] = r.x;
    lds_tile_base[(2 * j + 1) * kLdsLaneStride + tid] = r.y;
  }
  lds_tile_base[10 * kLdsLaneStride + tid] = sc.x;
  lds_tile_base[11 * kLdsLaneStride + tid] = sc.y;
}

// SobolSampler / HaltonSampler in a scene with Subsurface: a BSSRDF walk draws three dimensions per step and has no bound on
// its steps, SobolSampler's dimension counter does not wrap (sampler.h:143-155) and HaltonSampler's wraps at 1000 -- more
// than the nine bits of the packed state hold.  These variants keep the counter in a word of its own.
template <unsigned F>
constexpr bool big_sampler_dimension() { return (F & F_SSS) != 0 && (F & F_SOBOL) != 0; }

// The sampler of the path in `st` at pixel pxy (px | py << 16).  `big_dim()` yields the caller's own dimension counter; it
// is called only where that counter is the live one (big_sampler_dimension<F>(), and the sampler is not BlueSampler).
template <unsigned F, class BigDim>
__device__ __forceinline__ DSampler sampler_of(PackedState st, unsigned pxy, int sampler_kind, BigDim big_dim) {
  DSampler sampler;
  sampler.px = int(pxy & 0xffffu);
  sampler.py = int(pxy >> 16);
  sampler.index = st.s_cur();
  sampler.dimension = st.dim();
  if constexpr (big_sampler_dimension<F>())
    if (sampler_kind != 0) sampler.dimension = big_dim();
  return sampler;
}

// "Sample index s_next closes its item / chain": an item is `spi` consecutive samples -- a power of two that divides spp,
// or (another SobolSampler / HaltonSampler count) the whole pixel, which then starts at sample 0.
__device__ __forceinline__ bool closes_item(int spi, int s_next) {
  return (spi & (spi - 1)) == 0 ? (s_next & (spi - 1)) == 0 : s_next == spi;
}

// The camera ray of one sample (path.cpp:34-36): four RNG draws, then Camera::gen_ray.
__device__ __forceinline__ DRay camera_sample(const DCamera& cam, int px, int py, DRng& g) {
  // g++ evaluates gen_ray's arguments right to left (path.cpp:35): lens first, then jitter
  const float lx = rng_nextf(g);
  const float ly = rng_nextf(g);
  const float jx = rng_nextf(g);
  const float jy = rng_nextf(g);
  const f2 pf{(float(px) + jx) / float(cam.W), (float(py) + jy) / float(cam.H)};
  return camera_gen_ray(cam, pf, f2{lx, ly});
}

// The surface at the hit of ray (ray_o, ray_d) at tmax with primitive `prim` of `shape`.  Returns the index of the frame-table
// entry of the face that was hit, or a negative number (no table, or a hit that has no entry): surface_frame takes it.
template <unsigned F>
__device__ __forceinline__ int hit_surface(const SceneView& V, const DShape* shape, int prim, f3 ray_o, f3 ray_d, float tmax, DSurface& it) {
  it.p = it.n = mk3(0.0f);
  it.uv = f2{0, 0};
  const f3 ph = ray_o + tmax * ray_d;
  bool on_mesh = false;
  if constexpr (F & F_MESH) on_mesh = shape->kind == SHAPE_MESH;
  int entry = -1;
  if (on_mesh) {
    if constexpr (F & F_EMBREE) mesh_surface_info_embree(V.rcpps, V.tri_verts, V.tri_attrs, as_int(shape->f[4]), prim, ray_o, ray_d, it);
    else mesh_surface_info(V.tri_verts, V.tri_attrs, as_int(shape->f[4]), prim, ph, it);
  } else {
    // (has_frames is the same in every lane: a plan without a table does no more here than carry the face along; with one, only
    //  a Rect, an AABB or an OBB loads its base word.  A face is -1 ... 5, so `kNoFrame + face` stays negative.)
    constexpr int kNoFrame = -8;
    const float* frames = nullptr;
    int base = kNoFrame;
    if (V.has_frames) {
      frames = V.frames;
      if (frame_faces(shape->kind) != 0) base = V.frame_base[shape - V.shapes];
    }
    entry = base + shape_surface_info<F>(shape, ph, it, frames, base);
  }
  return entry;
}

// The tangent frame at a surface with normal n (interaction.h:14-17): the table's n, t, b where the hit has an entry
// (`entry`, from hit_surface), coordinate_system(n) elsewhere -- the same bits, by how the table is built.  A plan without a table
// runs coordinate_system as if there were no such thing as a table; with one, a wave none of whose lanes lacks an entry only
// loads, and a mixed wave computes and then loads over the result where a lane has an entry.
__device__ __forceinline__ m3 surface_frame(const SceneView& V, int entry, f3 n) {
#ifdef PINE_DUP_FRAME  /* cost measurement only: coordinate_system once more on an opaque copy of n (same film; the extra time is its cost) */
  {
    f3 nn = n;
    asm volatile("" : "+v"(nn.x), "+v"(nn.y), "+v"(nn.z));
    const m3 d = coordinate_system(nn);
    float sink = d.x.x + d.x.y + d.x.z + d.y.x + d.y.y + d.y.z;
    asm volatile("" : : "v"(sink));
  }
#endif
  auto load = [&]() {
    const float4 *q = reinterpret_cast<const float4*>(V.frames) + (kFrameFloats / 4) * entry, en = q[0], et = q[1], eb = q[2];
    return m3{f3{et.x, et.y, et.z}, f3{eb.x, eb.y, eb.z}, f3{en.x, en.y, en.z}};
  };
  if (V.has_frames && __ballot(entry < 0) == 0) return load();
  m3 m = coordinate_system(n);
  if (V.has_frames && entry >= 0) m = load();
  return m;
}

// What a path's last vertex returns, and the pdf of having picked it by light sampling (for the MIS weight one level up)
// unless the bounce that led here was a delta one.  hit = false: the ray left the scene (path.cpp:75-81); hit = true: it
// met the emissive `shape` at the surface `it` (path.cpp:83-87).  Callers pass `hit` as a constant.
template <unsigned F>
__device__ __forceinline__ f3 terminal_radiance(const SceneView& V, int env_light, int num_lights, bool hit, const DShape* shape, const DSurface& it,
                                                f3 ray_o, f3 ray_d, float tmax, bool is_delta, bool& has_light_pdf, float& light_pdf) {
  f3 Lo = mk3(0.0f);
  if (!hit) {
    if constexpr (F & F_LIGHTS)
      if (env_light >= 0) {
        const DLight* E = &V.lights[env_light];
        const bool image = E->kind == LIGHT_IMAGE_SKY, atmosphere = E->kind == LIGHT_ATMOSPHERE;
        if (image) Lo = mk3(1.0f) * image_sky_color(E, V.env, ray_d);
        else if (atmosphere) Lo = mk3(1.0f) * atmosphere_sky_color(E, ray_d);
        else Lo = mk3(1.0f) * sky_color_of(ld3(E->color), ray_d);
        if (!is_delta) {
          has_light_pdf = true;
          light_pdf = 1 / (4 * kPi);  // Sky::pdf -- not divided by the light count
          if (image || atmosphere) light_pdf = image_sky_pdf(E, V.env, ray_d);  // ImageSky::pdf, Atmosphere::pdf -- neither
        }
      }
  } else {
    Lo = mk3(1.0f) * material_le(&V.materials[shape->material], it.n, -ray_d);
    if (!is_delta) {
      has_light_pdf = true;
      const DRay ray{ray_o, ray_d, 0.0f, tmax};
      light_pdf = shape_pdf<F>(shape, ray, it.n);  // lightsampler.cpp:27-29: / lights.size()
      if (num_lights != 1) light_pdf = light_pdf / float(size_t(num_lights));  // x / 1.0f == x exactly
    }
  }
  return Lo;
}

// material.sample_bxdf (material.h:30-131, material.cpp:9-28): the lobe this vertex is shaded with -- kind, roughness and
// ior of `bx`; the caller sets the rest.  The pixel's RNG is loaded and stored (rng_load() -> DRng, rng_store(const DRng&))
// in the Uber branch only.  after_walk: the vertex was here before and started a BSSRDF walk; the lobe was chosen (and
// its draw made) then.
template <unsigned F, int SM, class RngLoad, class RngStore>
__device__ __forceinline__ void choose_lobe(const DMaterial* mat, const MatParams& mp, f3 wi, f3 n, bool diffused, bool after_walk, RngLoad rng_load,
                                            RngStore rng_store, const DTables& T, DSampler& sampler, DBxdf& bx) {
  const float min_roughness = diffused ? 0.6f : 0.0f;  // bxdf.h:15
  bx.kind = BX_DIFFUSE;
  bx.roughness = 0.0f;
  bx.ior = 1.0f;
  bool is_uber = false, is_sss = false, is_lobe = false;
  if constexpr (F & F_UBER) is_uber = mat->kind == MAT_UBER;
  if constexpr (F & F_UBER) is_lobe = mat->kind >= MAT_METAL;  // Metal / Glossy / Glass: one fixed lobe
  if constexpr (F & F_SSS) is_sss = mat->kind == MAT_SUBSURFACE;
  if (is_uber) {
    DRng g = rng_load();
    if (with_probability(mp.metallic, g)) {
      bx.kind = BX_CONDUCTOR;
      bx.roughness = mp.roughness;
    } else if (with_probability(mp.transmission, g)) {
      bx.kind = BX_REFR_DIEL;
      bx.roughness = mp.roughness;
      bx.ior = mp.ior;
    } else {
      bx.kind = BX_DIFF_DIEL;
      bx.roughness = mp.roughness;
      bx.ior = mp.ior;
    }
    rng_store(g);
  } else if (is_lobe) {  // material.h:39-78
    bx.kind = mat->kind == MAT_METAL ? BX_CONDUCTOR : mat->kind == MAT_GLOSSY ? BX_DIFF_DIEL : BX_REFR_DIEL;
    bx.roughness = pmax(mp.roughness, min_roughness);
    bx.ior = mp.ior;
  } else if (is_sss) {
    if (after_walk) {
      bx.kind = BX_BSSRDF;
      bx.ior = mat->ior;
    } else {
      const float fr = FrDielectric(dot(wi, n), mat->ior);
      if (sampler_get1d<SM>(T, sampler) < fr) {
        bx.kind = BX_REFRACTIVE;
        bx.roughness = pmax(mp.roughness, min_roughness);
        bx.ior = mat->ior;
      } else if (diffused) {
        bx.kind = BX_DIFFUSE;
      } else {
        bx.kind = BX_BSSRDF;
        bx.ior = mat->ior;
      }
    }
  }
}

// ---- the BSSRDF random walk inside the shape that was hit (SeparableBSSRDF::sample_p, bxdf.cpp:329-353, :375-382) ----
// walk_begin, then walk_step until it answers something other than kWalkRunning, then (kWalkExited) walk_exit.  Where
// the walk's state lives between steps -- registers of a loop, or a context's record between passes of a stage -- is the
// kernel's business.  Each function sets ALL its outputs on every path: an output left undefined on one path reaches the
// kernels' merged control flow as an undefined value, and that cost the queue kernel's Subsurface variants up to 29 spilled
// VGPRs (profiles/prologue_and_walk_once.txt).

// Refraction into the shape, the colour channel (one draw from the pixel's RNG), the first ray.  false is the reference's
// nullopt: nothing was drawn, nothing changes, the vertex is shaded where it was hit.
template <class RngLoad, class RngStore>
__device__ __forceinline__ bool walk_begin(f3 wi, const DSurface& it, const DBxdf& bx, RngLoad rng_load, RngStore rng_store, int& channel, DRay& first_ray) {
  channel = 0;
  first_ray = DRay{};
  f3 w = -wi;
  if (!Refract(wi, it.n, bx.ior, w, nullptr)) return false;
  DRng g = rng_load();
  channel = int(rng_nextf(g) * 3);
  rng_store(g);
  first_ray = spawn_ray_raw(it.p, it.n, w);  // (later rays start AT the scattering point, with tmax = float max)
  return true;
}

// One free-flight step along `wr`.  `inside(DRay& wr, int& prim) -> bool` is the closest-hit query against `shape` alone
// (it shortens wr.tmax); each kernel passes its own traversal call.  Answers a PackedState walk status:
//   kWalkFailed   the ray found no surface (nullopt: nothing changes);
//   kWalkExited   the free flight ends beyond the surface: sit.p / .n are the exit point and its normal;
//   kWalkRunning  scattered: next_ray leaves the scattering point in a uniformly drawn direction.
// Draws one sampler dimension, and two more when it scatters.
template <unsigned F, int SM, class Inside>
__device__ __forceinline__ unsigned walk_step(const SceneView& V, const DShape* shape, const DMaterial* mat, int channel, DRay wr, Inside inside,
                                              const DTables& T, DSampler& sampler, DRay& next_ray, DSurface& sit) {
  next_ray = wr;
  // Shape::intersect fills it.p / it.n for meshes only: non-mesh shapes leave them zero
  sit.p = sit.n = mk3(0.0f);
  sit.uv = f2{0, 0};
  int prim = 0;
  if (!inside(wr, prim)) return kWalkFailed;
  const float t = -plog(1 - sampler_get1d<SM>(T, sampler)) * (1 / mat->sigma_s[channel]);
  if (wr.tmax < t) {
    bool walk_mesh = false;
    if constexpr (F & F_MESH) walk_mesh = shape->kind == SHAPE_MESH;
    if (walk_mesh) mesh_surface_info(V.tri_verts, V.tri_attrs, as_int(shape->f[4]), prim, ray_at(wr, wr.tmax), sit);
    return kWalkExited;
  }
  const f3 p = ray_at(wr, t);
  next_ray = DRay{p, uniform_sphere(sampler_get2d<SM>(T, sampler)), 0.0f, kFloatMax};
  return kWalkRunning;
}

// The walk left the shape in `channel`: the vertex moves to the exit point and is shaded there, its incoming direction the
// reversed last walk direction (bxdf.cpp:375-382); beta becomes 3 in that channel (clamp_radiance).
__device__ __forceinline__ void walk_exit(f3 exit_p, f3 exit_n, f3 last_dir, int channel, DSurface& it, m3& l2w, m3& w2l, DBxdf& bx, int& beta_channel) {
  beta_channel = channel + 1;
  it.p = exit_p;
  it.n = exit_n;
  l2w = coordinate_system(it.n);
  w2l = transpose(l2w);
  bx.wi = mul(w2l, -last_dir);
}

// Next-event estimation (path.cpp:98-113) at a vertex whose lobe is not a delta one: the light sampler's draws, the light
// sample, the shadow ray, the direct term.  `occluded(const DRay&) -> bool` is the visibility test: a caller that traces
// here and now answers the truth and the term of an occluded light is never evaluated; a caller that defers the trace
// records the ray, answers "visible" and clears the term itself.  No draw depends on the answer.  Counts the ray in
// shadow_count.  Sets bx.albedo / albedo_over_pi.
template <unsigned F, int SM, class Occluded>
__device__ __forceinline__ f3 sample_direct(const SceneView& V, int num_lights, const DSurface& it, const m3& w2l, DBxdf& bx, const MatParams& mp,
                                            const DTables& T, DSampler& sampler, unsigned& shadow_count, Occluded occluded) {
  f3 nee = mk3(0.0f);
  // g++ order for LightSampler::sample's arguments (lightsampler.h:27): get2d, then get1d
  const f2 u2 = sampler_get2d<SM>(T, sampler);
  float u1 = sampler_get1d<SM>(T, sampler);
  if (num_lights > 0) {  // UniformLightSampler::sample lightsampler.cpp:12-26
    if (num_lights != 1) u1 *= float(num_lights);  // x * 1.0f == x exactly
    const int index = int(u1);
    const DLight* L = &V.lights[index];
    int lkind = LIGHT_AREA;  // (no other light kinds without F_LIGHTS)
    if constexpr (F & F_LIGHTS) lkind = L->kind;
    bool lvalid = false;
    f3 lw = mk3(0.0f), lle = mk3(0.0f);
    float ldist = 0.0f, lpdf = 0.0f;
    if (lkind == LIGHT_AREA) {  // AreaLight::sample light.cpp:55-69
      const DShape* lshape = &V.shapes[L->geom];
      DShapeSample gs;
      if (shape_sample<F>(lshape, V.tri_verts, it.p, u2, u1 - float(index), gs)) {
        lle = material_le(&V.materials[lshape->material], gs.n, -gs.w);
        lvalid = !is_zero(lle);
        lw = gs.w;
        ldist = gs.distance;
        lpdf = gs.pdf;
      }
    } else {  // light.cpp:11-84, 109-119, 146-163: point, spot, directional, Sky, Atmosphere, ImageSky
      if constexpr (F & F_LIGHTS) lvalid = light_sample_other(L, V.env, it.p, u2, lw, ldist, lpdf, lle);
    }
    const bool ldelta = lkind == LIGHT_POINT || lkind == LIGHT_SPOT || lkind == LIGHT_DIRECTIONAL;  // light.h:111-113
    if (lvalid) {
      const float ls_pdf = num_lights != 1 ? lpdf / float(num_lights) : lpdf;
      shadow_count++;
      const DRay sr = spawn_ray(it.p, it.n, lw, ldist);
      if (!occluded(sr)) {
        bx.albedo = mp.albedo;
        bx.albedo_over_pi = mp.albedo_over_pi;
        const float cosine = absdot(lw, it.n);
        const f3 wo = mul(w2l, lw);
        const f3 f = bxdf_f<F>(bx, wo);
        if (ldelta) {  // path.cpp:104-106: no MIS against a delta light
          nee = mk3(0.0f) + lle * mk3(1.0f) * cosine * f / ls_pdf;
        } else {
          const float mis = balance_heuristic(ls_pdf, bxdf_pdf<F>(bx, wo));
          nee = mk3(0.0f) + lle * mk3(1.0f) * cosine * f / ls_pdf * mis;
        }
      }
    }
  }
  return nee;
}

// min(beta * lo, 8) (path.cpp:121): beta is 1, or -- the vertex left a BSSRDF walk in channel beta_channel - 1
// (bxdf.cpp:335) -- 3 in that channel and 0 in the others.
__device__ __forceinline__ f3 clamp_radiance(int beta_channel, f3 lo) {
  f3 beta = mk3(1.0f);
  if (beta_channel) {
    beta = mk3(0.0f);
    set(beta, beta_channel - 1, 3.0f);
  }
  return mk3(0.0f) + vmin(mk3(1.0f) * beta * lo, mk3(8.0f));
}

// One level of the backward fold (path.cpp:114-121).  e = the level's pending entry: direct term (3),
// BSDF value (3), cosine / pdf, pdf.  Li: radiance from the level below in, this level's out.  The light pdf (lp_valid, lp)
// weighs the level directly above the terminal vertex only.  beta_flags: 2 bits per level, the BSSRDF beta channel.
// Returns the MIS weight it used.
template <unsigned F>
__device__ __forceinline__ float fold_level(const float (&e)[8], unsigned long long beta_flags, int level, f3& Li, bool& lp_valid, float lp) {
  const f3 e_nee{e[0], e[1], e[2]};
  const f3 e_f{e[3], e[4], e[5]};
  const float e_cp = e[6], e_pdf = e[7];
  const float mis = lp_valid ? balance_heuristic(e_pdf, lp) : 1.0f;
  const f3 lo = e_nee + Li * e_f * (e_cp * mis);
  int beta_channel = 0;
  if constexpr (F & F_SSS) beta_channel = int(unsigned(beta_flags >> (2 * level)) & 3u);
  Li = clamp_radiance(beta_channel, lo);
  lp_valid = false;
  return mis;
}

}  // namespace pine_gpu
