// pine_amd/csrc/pine_radiance.h -- the per-vertex steps of radiance() (path.cpp:42-124), written once.
//
// Every film has to match the reference bit for bit: each path vertex runs the same floating-point operations, the same
// sampler draws and the same RNG draws in the same order as the reference.  That sequence lives HERE; the two path kernels
// (path_trace_kernel in pine_kernels_device.h, path_queue_body in pine_queue_kernel.h) only decide when a step runs and
// where its state is kept.  The functions take what they need as arguments -- SceneView, scalar fields of DeviceScene,
// DTables, DSampler&, DRng& or load / store callables -- and know nothing about queues, contexts, LDS layouts or lane
// state.  All are force-inlined: a caller's constant arguments fold, and a callable costs nothing.
// Included by pine_kernels_device.h after SceneView, PackedState and material_le.
#pragma once

namespace pine_gpu {

// SceneView over a scene blob (DeviceScene::blob and its off_* offsets) staged at `base`.  The nodes and the reciprocal
// table are the caller's: not every kernel stages them with the rest.
__device__ __forceinline__ void view_of_blob(const char* base, const DeviceScene& S, SceneView& V) {
  V.shapes = reinterpret_cast<const DShape*>(base + S.off_shapes);
  V.materials = reinterpret_cast<const DMaterial*>(base + S.off_materials);
  V.bvhs = reinterpret_cast<const DBvh*>(base + S.off_bvhs);
  V.prims = nullptr;
  V.lights = reinterpret_cast<const DLight*>(base + S.off_lights);
  V.node_ops = reinterpret_cast<const DNodeOp*>(base + S.off_node_ops);
  V.leaf = reinterpret_cast<const DShape*>(base + S.off_leaf) - S.top_prim_begin;
  V.etree = reinterpret_cast<const EmbreeNode*>(base + S.off_etree);
  V.emesh = reinterpret_cast<const int*>(base + S.off_emesh);
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

// The surface at the hit of ray (ray_o, ray_d) at tmax with primitive `prim` of `shape`.
template <unsigned F>
__device__ __forceinline__ void hit_surface(const SceneView& V, const DShape* shape, int prim, f3 ray_o, f3 ray_d, float tmax, DSurface& it) {
  it.p = it.n = mk3(0.0f);
  it.uv = f2{0, 0};
  const f3 ph = ray_o + tmax * ray_d;
  bool on_mesh = false;
  if constexpr (F & F_MESH) on_mesh = shape->kind == SHAPE_MESH;
  if (on_mesh) {
    if constexpr (F & F_EMBREE) mesh_surface_info_embree(V.rcpps, V.tri_verts, V.tri_attrs, as_int(shape->f[4]), prim, ray_o, ray_d, it);
    else mesh_surface_info(V.tri_verts, V.tri_attrs, as_int(shape->f[4]), prim, ph, it);
  } else shape_surface_info<F>(shape, ph, it);
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
        Lo = mk3(1.0f) * sky_color_of(ld3(V.lights[env_light].color), ray_d);
        if (!is_delta) {
          has_light_pdf = true;
          light_pdf = 1 / (4 * kPi);  // Sky::pdf -- not divided by the light count
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
    } else {  // light.cpp:11-84: point, spot, directional, Sky
      if constexpr (F & F_LIGHTS) lvalid = light_sample_other(L, it.p, u2, lw, ldist, lpdf, lle);
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
