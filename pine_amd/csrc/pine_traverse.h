// pine_amd/csrc/pine_traverse.h -- what a ray does in the scene's BVHs (included by pine_kernels_device.h after SceneView /
// WorkParams, before pine_radiance.h).  It holds
//   * the steps every walk shares, each written once: fetch_node / fetch_triangle, load_leaf_record, bvh2_order_children,
//     the test hook's TravLog -- the flat state machine of pine_trav.h uses them too;
//   * the nested walks: bvh2_walk, and on it mesh_traverse (a mesh's own BVH) and scene_traverse (the top level);
//   * EmbreeAccel's order (F_EMBREE variants): Embree's reciprocal and triangle test, the BVH8 ray setup and child test,
//     scene_traverse_embree / scene_occluded_embree.
// The order in which boxes and primitives are tested is part of the result (tests/test_bvh_fixtures.py,
// tests/test_embree_order.py: every primitive test of every ray, in order, against the reference).
#pragma once

namespace pine_gpu {

// One BVH node into registers.  F_LDS_TOP: from the workgroup's LDS copy when the index is below the cached
// count (four ds_read_b128), else from global memory (four global_load_dwordx4).  The LDS arm goes through an
// address_space(3) pointer: with two generic pointers the compiler folds the branch into a pointer select and
// emits flat loads, which occupy both memory pipes.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const u32x4 lds_u32x4;
template <unsigned F>
__device__ __forceinline__ DNode fetch_node(const SceneView& S, int index) {
  union {
    DNode n;
    u32x4 q[4];
  } b;
  if constexpr (F & F_LDS_TOP) {
    if (index < S.lds_node_count) {
      lds_u32x4* p = (lds_u32x4*)(S.lds_nodes) + size_t(index) * 4;
      b.q[0] = p[0], b.q[1] = p[1], b.q[2] = p[2], b.q[3] = p[3];
      return b.n;
    }
  }
  const u32x4* g = reinterpret_cast<const u32x4*>(S.nodes + index);
  b.q[0] = g[0], b.q[1] = g[1], b.q[2] = g[2], b.q[3] = g[3];
  return b.n;
}

// One leaf-ordered triangle: from the workgroup's LDS packets when they are staged (an 8-byte entry, then three 16-byte
// vertices: ds_read_b64 + 3 ds_read_b128), else its 48-byte record in global memory.  The floats are the same.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const u32x2 lds_u32x2;
template <unsigned F>
__device__ __forceinline__ void fetch_triangle(const SceneView& S, int i, float (&v)[9], int& tri) {
  if constexpr ((F & F_LDS_TOP) != 0 && (F & F_MESH) != 0) {
    if (S.lds_tri_entries != nullptr) {
      const u32x2 e = *((lds_u32x2*)(S.lds_tri_entries) + i);
      lds_u32x4* vb = (lds_u32x4*)(S.lds_tri_verts);
      const u32x4 a = vb[e.x & 0xffffu], b = vb[e.x >> 16], c = vb[e.y & 0xffffu];
      v[0] = __uint_as_float(a.x), v[1] = __uint_as_float(a.y), v[2] = __uint_as_float(a.z);
      v[3] = __uint_as_float(b.x), v[4] = __uint_as_float(b.y), v[5] = __uint_as_float(b.z);
      v[6] = __uint_as_float(c.x), v[7] = __uint_as_float(c.y), v[8] = __uint_as_float(c.z);
      tri = int(e.y >> 16);
      return;
    }
  }
  const float4* rec = S.tri_leaf + size_t(i) * 3;
  const float4 a = rec[0], b = rec[1], c = rec[2];
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w, v[8] = c.x;
  tri = __float_as_int(c.y);
}

// ------------------------------------------------------------------------------------------------
// BVH traversal -- pine's ordered stack traversal (src/pine/impl/accel/bvh.cpp:321-451), with the
// node's two child boxes tested against the tmax captured when the node is visited, leaf children
// tested inline in stored primitive order, nearer-exit child first.  The stack lives in LDS,
// lane-interleaved ([slot][thread]) so pushes/pops are bank-conflict free.
// ------------------------------------------------------------------------------------------------
// Test hook (pine_gpu_test_traverse): the primitives a traversal tests, in order -- a top-level primitive's geometry
// index, or 0x40000000 | triangle index inside the mesh entered last.  Null in every kernel (the calls fold away).
struct TravLog {
  unsigned* words;
  int n, cap;
  __device__ __forceinline__ void put(unsigned w) {
    if (n < cap) words[n] = w;
    n++;
  }
};

// A top-level leaf primitive's whole 128-byte record (SceneView::leaf; the packed word rides in its kind field), fetched in
// ONE batch of eight quad loads before the kind is looked at: reading the kind word first and the kind's fields after the
// dispatch is two dependent round trips per primitive test -- to L2 where the records live in global memory (10 000 cones:
// C4 7.70 -> 7.11 ms), to LDS elsewhere (C5 134.5 -> 132.1 ms, C2's nested walk 13.20 -> 13.06 ms).  Quads that no kind
// of the variant reads are dead loads the compiler drops.
__device__ __forceinline__ DShape load_leaf_record(const DShape* sh) {
  DShape rec;
  const uint4* src = reinterpret_cast<const uint4*>(sh);
  uint4* dst = reinterpret_cast<uint4*>(&rec);
#pragma unroll
  for (int q = 0; q < 8; q++) dst[q] = src[q];
  return rec;
}

// The end of a BVH2 node visit (bvh.cpp:405-446): l / r are the inner children whose boxes the ray enters (-1: none, or a
// leaf), t0 / t1 their exit distances.  Of two, the one with the larger exit distance is pushed (equal: the right one) and
// the other is visited next.  -> next: the node to visit next, -1 for none (the caller pops).  (`next` is set on every
// path, and through the reference: as a returned value it cost two flat-walk variants 4 spilled VGPRs each -- and the nested
// walk asks for its pop first; profiles/traversal_once.txt.)
template <int STRIDE, class StackT>
__device__ __forceinline__ void bvh2_order_children(int l, int r, float t0, float t1, StackT* stack, int& sp, int& next) {
  next = r;
  if (l != -1) {
    if (r != -1) {
      if (t0 > t1) {
        stack[sp * STRIDE] = StackT(l);
        next = r;
      } else {
        stack[sp * STRIDE] = StackT(r);
        next = l;
      }
      sp++;
    } else next = l;
  }
}

// The nested walk over one BVH2 from inner node `root`, with the stack entries from sp0 on: visit a node, test both child
// boxes against the tmax of that moment, hand leaf children to `leaf(start, count)` in stored order (it tests the primitives,
// may shorten `ray`, and returns true to end the walk: an any-hit query's answer), order the inner children, pop.
// -> true when a leaf ended the walk.  TOP_REGION >= 0: the top-level walk -- its REGION id of -DPINE_PROFILE_REGIONS builds,
// and the -DPINE_DUP_NODES cost measurement (both box tests once more on an opaque tmin); a mesh's walk (-1) has neither.
template <int TOP_REGION, unsigned F, int STRIDE, class StackT, class Leaf>
__device__ __forceinline__ bool bvh2_walk(const SceneView& S, int root, int sp0, const DRay& ray, const DRayOct& oct, StackT* stack, Leaf&& leaf) {
  int sp = sp0;
  int next = root;
  while (true) {
    if constexpr (TOP_REGION >= 0) {
      REGION(TOP_REGION);  // top-level node visit
    }
    // (without F_LDS_TOP the node is read through the pointer, not copied)
    DNode nd;
    const DNode* node = &S.nodes[next];
    if constexpr (F & F_LDS_TOP) {
      nd = fetch_node<F>(S, next);
      node = &nd;
    }
    int l = -1, r = -1;
    float t0 = ray.tmax, t1 = ray.tmax;
#ifdef PINE_DUP_NODES
    if constexpr (TOP_REGION >= 0) {
      float q0 = ray.tmax, q1 = ray.tmax, tm = ray.tmin;
      asm volatile("" : "+v"(tm));
      const bool b0 = box_hit_oct(node->lo0, node->hi0, oct, tm, q0);
      const bool b1 = box_hit_oct(node->lo1, node->hi1, oct, tm, q1);
      float sink = (b0 ? q0 : 0.0f) + (b1 ? q1 : 0.0f);
      asm volatile("" : : "v"(sink));
    }
#endif
    if (box_hit_oct(node->lo0, node->hi0, oct, ray.tmin, t0)) {
      if (node->count[0] == 0) l = node->child[0];
      else if (leaf(node->child[0], node->count[0])) return true;
    }
    if (box_hit_oct(node->lo1, node->hi1, oct, ray.tmin, t1)) {
      if (node->count[1] == 0) r = node->child[1];
      else if (leaf(node->child[1], node->count[1])) return true;
    }
    if (l == -1 && r == -1) {
      if (sp == sp0) break;
      next = int(stack[(--sp) * STRIDE]);
    } else bvh2_order_children<STRIDE>(l, r, t0, t1, stack, sp, next);
  }
  return false;
}

// ---- PINE_GPU_FLAG_ORDER_EMBREE: arithmetic of the vendored Embree 4.3.1 as an AVX2 x86 host runs it (see scene_traverse_embree) ----
// rcp(a) (common/math/vec3fa.h:122-144, common/simd/vfloat4_sse2.h:304-318): one fused Newton step on the RCPPS estimate, which is
// the table's entry for the operand's top 11 mantissa bits scaled by its exponent (infinity for zero / denormal operands and
// results beyond the range, zero for results below the normal range)
__device__ __forceinline__ float embree_rcp(const unsigned* table, float a) {
  const unsigned u = __float_as_uint(a);
  const int e = int((u >> 23) & 0xffu);
  const unsigned t = table[(u >> 12) & 0x7ffu];  // the estimate for the mantissa in [1, 2): in (0.5, 1]
  const int re = int((t >> 23) & 0xffu) + 127 - e;
  const unsigned sign = u & 0x80000000u;
  const float r = __uint_as_float(e == 0 || re >= 255 ? (sign | 0x7f800000u) : re <= 0 ? sign : (sign | (unsigned(re) << 23) | (t & 0x7fffffu)));
  return __fmaf_rn(r, __fmaf_rn(-a, r, 1.0f), r);
}
__device__ __forceinline__ float embree_rcp_safe(const unsigned* table, float a) {
  return embree_rcp(table, fabsf(a) < 1e-18f ? 1e-18f : a);  // zero_fix: min_rcp_input (vec3fa.h:167-172)
}
// One lane of TriangleMIntersector1Moeller<4, true> (kernels/geometry/triangle_intersector_moeller.h:66-140, :29-37): meshes
// are Embree TRIANGLE geometry under EmbreeAccel (embree.cpp:76-87), Triangle4 blocks keeping v0, e1 = v0 - v1, e2 = v2 - v0
// (geometry/triangle.h); cross and dot products fused as common/math/vec3.h does.  -> t, the barycentrics and the geometric
// normal EmbreeAccel::intersect builds the surface point from (embree.cpp:233-247).  Which triangles Embree's own hierarchy
// hands to the test (spatial splits: not restated) cannot change the closest hit; only an exact tie in t is decided by it.
__device__ __forceinline__ bool embree_tri_test(const unsigned* table, const float* v, f3 o, f3 d, float tnear, float tfar, float& t, f2& uv, f3& ng) {
  const f3 v0 = ld3(v), e1 = v0 - ld3(v + 3), e2 = ld3(v + 6) - v0;
  auto crossf = [](f3 a, f3 b) { return f3{__fmaf_rn(a.y, b.z, -(a.z * b.y)), __fmaf_rn(a.z, b.x, -(a.x * b.z)), __fmaf_rn(a.x, b.y, -(a.y * b.x))}; };
  auto dotf = [](f3 a, f3 b) { return __fmaf_rn(a.x, b.x, __fmaf_rn(a.y, b.y, a.z * b.z)); };
  ng = crossf(e2, e1);
  const f3 C = v0 - o, R = crossf(C, d);
  const float den = dotf(ng, d), abs_den = fabsf(den);
  const unsigned sgn = __float_as_uint(den) & 0x80000000u;
  const float U = __uint_as_float(__float_as_uint(dotf(R, e2)) ^ sgn), V = __uint_as_float(__float_as_uint(dotf(R, e1)) ^ sgn);
  if (!(den != 0.0f && U >= 0.0f && V >= 0.0f && U + V <= abs_den)) return false;
  const float T = __uint_as_float(__float_as_uint(dotf(ng, C)) ^ sgn);
  if (!(abs_den * tnear < T && T <= abs_den * tfar)) return false;
  const float r = embree_rcp(table, abs_den);
  t = T * r;
  uv = f2{U * r, V * r};
  return true;
}
// EmbreeAccel::intersect's surface point on a mesh (embree.cpp:233-247): position, normal and texcoord from Embree's barycentrics
// and geometric normal of the winning triangle -- recomputed here from the ray (they do not depend on tfar)
__device__ __forceinline__ void mesh_surface_info_embree(const unsigned* table, const float* tri_verts, const float* tri_attrs, int flags, int prim, f3 o, f3 d, DSurface& it) {
  const float* v = tri_verts + size_t(prim) * 9;
  float t = 0.0f;
  f2 bary{0.0f, 0.0f};
  f3 ng = mk3(0.0f);
  (void)embree_tri_test(table, v, o, d, -1.0f, __uint_as_float(0x7f800000u), t, bary, ng);  // (the hit exists: every t passes)
  it.p = lerp3(bary.x, bary.y, ld3(v), ld3(v + 3), ld3(v + 6));
  it.n = normalize(ng);
  it.uv = bary;
  if (flags != 0) {
    const float* a = tri_attrs + size_t(prim) * 16;
    if (flags & 1) it.n = normalize(lerp3(bary.x, bary.y, ld3(a), ld3(a + 3), ld3(a + 6)));
    if (flags & 2) it.uv = (1.0f - bary.x - bary.y) * f2{a[9], a[10]} + bary.x * f2{a[11], a[12]} + bary.y * f2{a[13], a[14]};
  }
}

// (EMB: Embree's triangle test instead of pine's -- the scene queries of the F_EMBREE variants; the BSSRDF walk's queries against
//  the mesh's own ShapeBVH are pine's whatever the accel)
template <bool ANY, int STRIDE = kBlock, unsigned F = 0, class StackT = int, bool EMB = false>
__device__ __forceinline__ bool mesh_traverse(const SceneView& S, const DBvh bvh, DRay& ray,
                                              const DRayOct& oct, StackT* stack, int sp0, int& prim_out, TravLog* log = nullptr) {
  bool hit = false;
  auto leaf = [&](int start, int count) -> bool {
    for (int i = start; i < start + count; i++) {
      // leaf-ordered record: v0 v1 v2 | triangle index (FlatAccel::tri_leaf, or its LDS packets)
      float v[9];
      int tri;
      fetch_triangle<F>(S, i, v, tri);
      if (log) log->put(0x40000000u | unsigned(tri - bvh.prim_base));  // (the index within its mesh, as the reference counts)
      if constexpr (EMB) {
        float t;
        f2 uv;
        f3 ng;
        if (embree_tri_test(S.rcpps, v, ray.o, ray.d, fmaxf(ray.tmin, 0.0f), ray.tmax, t, uv, ng)) {
          if (ANY) return true;
          ray.tmax = t;
          hit = true;
          prim_out = tri;
        }
      } else if (ANY) {
        if (tri_hit(v, ray)) return true;
      } else if (tri_intersect(v, ray)) {
        hit = true;
        prim_out = tri;
      }
    }
    return false;
  };
  if (bvh.root_count > 0) {
    if (leaf(bvh.root_start, bvh.root_count)) return true;
    return hit;
  }
  if (bvh2_walk<-1, F, STRIDE>(S, bvh.root, sp0, ray, oct, stack, leaf)) return true;
  return hit;
}

// The BVH8 side of EmbreeAccel's order, shared by its closest-hit and any-hit queries (described at scene_traverse_embree).
// The ray as a node test reads it (kernels/bvh/node_intersector1.h:26-60): rdir, org * rdir, where in a node's record the near
// plane of each axis starts (the lower one where rdir >= 0; the far one is at `^ 24`), tnear / tfar as the integers compared.
struct EmbreeRay {
  float rdx, rdy, rdz, ordx, ordy, ordz;
  int nx, ny, nz;
  int tnear, tfar;
};
__device__ __forceinline__ EmbreeRay embree_ray(const SceneView& S, const DRay& ray) {
  EmbreeRay e;
  e.rdx = embree_rcp_safe(S.rcpps, ray.d.x), e.rdy = embree_rcp_safe(S.rcpps, ray.d.y), e.rdz = embree_rcp_safe(S.rcpps, ray.d.z);
  e.ordx = ray.o.x * e.rdx, e.ordy = ray.o.y * e.rdy, e.ordz = ray.o.z * e.rdz;
  e.nx = e.rdx >= 0.0f ? 0 : 24, e.ny = e.rdy >= 0.0f ? 0 : 24, e.nz = e.rdz >= 0.0f ? 0 : 24;
  e.tnear = __float_as_int(fmaxf(ray.tmin, 0.0f));
  e.tfar = __float_as_int(fmaxf(ray.tmax, 0.0f));
  return e;
}
// One node's child test (node_intersector1.h:484-530): `enter(child, tn)` for every child the ray enters, in slot order.
// Four children at a time: the six planes of each as quads (near / far side chosen by the quad's address), the child words
// as one more; unused slots are never entered -- their planes are infinite -- and a second half without children is skipped.
template <class Enter>
__device__ __forceinline__ void embree_node_children(const EmbreeNode* node, const EmbreeRay& e, Enter&& enter) {
  const float* nd = reinterpret_cast<const float*>(node);
  const int count = reinterpret_cast<const int*>(nd)[56];
  const float rdx = e.rdx, rdy = e.rdy, rdz = e.rdz, ordx = e.ordx, ordy = e.ordy, ordz = e.ordz;
  const int tnear = e.tnear, tfar = e.tfar;
  for (int half = 0; half < 8 && half < count; half += 4) {
    const float4 nxq = *reinterpret_cast<const float4*>(nd + e.nx + half), nyq = *reinterpret_cast<const float4*>(nd + 8 + e.ny + half),
                 nzq = *reinterpret_cast<const float4*>(nd + 16 + e.nz + half);
    const float4 fxq = *reinterpret_cast<const float4*>(nd + (e.nx ^ 24) + half), fyq = *reinterpret_cast<const float4*>(nd + 8 + (e.ny ^ 24) + half),
                 fzq = *reinterpret_cast<const float4*>(nd + 16 + (e.nz ^ 24) + half);
    const int4 ch = *reinterpret_cast<const int4*>(nd + 48 + half);
    auto one = [&](float px, float py, float pz, float qx, float qy, float qz, int child) {
      const int tn = max(max(__float_as_int(__fmaf_rn(px, rdx, -ordx)), __float_as_int(__fmaf_rn(py, rdy, -ordy))),
                         max(__float_as_int(__fmaf_rn(pz, rdz, -ordz)), tnear));
      const int tf = min(min(__float_as_int(__fmaf_rn(qx, rdx, -ordx)), __float_as_int(__fmaf_rn(qy, rdy, -ordy))),
                         min(__float_as_int(__fmaf_rn(qz, rdz, -ordz)), tfar));
      if (!(tn > tf)) enter(child, tn);
    };
    one(nxq.x, nyq.x, nzq.x, fxq.x, fyq.x, fzq.x, ch.x);
    one(nxq.y, nyq.y, nzq.y, fxq.y, fyq.y, fzq.y, ch.y);
    one(nxq.z, nyq.z, nzq.z, fxq.z, fyq.z, fzq.z, ch.z);
    one(nxq.w, nyq.w, nzq.w, fxq.w, fyq.w, fzq.w, ch.w);
  }
}

// PINE_GPU_FLAG_ORDER_EMBREE (F_EMBREE variants): closest-hit queries hand the non-mesh shapes to their tests in the order the
// reference's DEFAULT accel does -- BVHNIntersector1<8, BVH_AN1, false, ...>::intersect of the vendored Embree 4.3.1
// (src/contrib/embree/kernels/bvh/bvh_intersector1.cpp:30-107) over the BVH8 of pine_embree_order.h, as an AVX2 x86 host runs it:
//   * the ray: rdir = rcp_safe(dir) -- one fused Newton step on the RCPPS estimate (common/math/vec3fa.h:122-172; the estimates
//     are the table of pine_amd/data/rcpps_table.h) -- and org_rdir = org * rdir (kernels/bvh/node_intersector1.h:26-60);
//   * a node: per child fused plane * rdir - org_rdir, maximum / minimum over the float words compared as INTEGERS, entered when
//     not tNear > tFar (node_intersector1.h:484-530);
//   * its hit children, in slot order: one -> descend; two -> the nearer first (equal: the second); three / four -> the sorting
//     networks of common/stack_item.h:54-84; more -> the stable descending insertion sort (:88-104); the nearest is descended
//     into, the others wait on the stack with their distances (kernels/bvh/bvh_traverser1.h:310-385);
//   * a popped entry whose distance lies beyond the closest hit so far is dropped (bvh_intersector1.cpp:77-79).
// Meshes are Embree triangle geometry: they are asked FIRST (the triangle accel precedes the user-geometry accel,
// kernels/common/scene.cpp:741-755), through Embree's own triangle test (embree_tri_test above; pine's per-mesh BVH only decides
// which triangles are looked at).  tests/test_embree_order.py, tests/test_gpu_parity.py: the films of the real reference built
// with EmbreeAccel, bit for bit.
template <unsigned F, int STRIDE, class StackT>
__device__ __forceinline__ bool scene_traverse_embree(const SceneView& S, DRay& ray, StackT* stack, int& geom_out, int& prim_out, TravLog* log) {
  bool hit = false;
  auto test_leaf = [&](int place) {
    const DShape rec = load_leaf_record(&S.leaf[place]), *sh = &rec;
    const int word = sh->kind;  // (the packed word rides in the copy's kind field)
    const int kind = word >> kPrimKindShift;
    bool is_mesh = false;
    if constexpr (F & F_MESH) is_mesh = kind == SHAPE_MESH;
    if (log) log->put(unsigned(word & kPrimIndexMask));
    if (is_mesh) {
      if constexpr (F & F_MESH) {
        const DRayOct oct = make_oct(ray);
        int prim = 0;
        if (mesh_traverse<false, STRIDE, F, StackT, true>(S, S.bvhs[as_int(sh->f[2])], ray, oct, stack, S.stack_top, prim, log)) {
          hit = true;
          geom_out = word;
          prim_out = prim;
        }
      }
    } else if (shape_intersect<F>(kind, sh, ray)) {
      hit = true;
      geom_out = word;
    }
  };
  if constexpr (F & F_MESH)
    for (int k = 0; k < S.num_emesh; k++) test_leaf(S.emesh[k]);
  if (S.etree_root == kEmbreeNoChild) return hit;
  EmbreeRay er = embree_ray(S, ray);
  int2 items[kEmbreeStackEntries];  // (child word, distance word)
  int sp = 1;
  items[0] = int2{S.etree_root, int(0xff800000u)};  // (distance -inf)
  while (sp > 0) {
    sp--;
    int cur = items[sp].x;
    if (__int_as_float(items[sp].y) > ray.tmax) continue;
    bool dropped = false;
    while (cur >= 0) {
      const int first = sp;
      embree_node_children(&S.etree[cur], er, [&](int child, int tn) { items[sp++] = int2{child, tn}; });
      const int hits = sp - first;
      if (hits == 0) {
        dropped = true;
        break;
      }
      auto order = [&](int a, int b) {  // cmp_xchg: items[a] <= items[b] afterwards
        if (items[b].y < items[a].y) {
          const int2 t = items[a];
          items[a] = items[b], items[b] = t;
        }
      };
      int2* h = items + first;
      if (hits == 2) {
        if (unsigned(h[0].y) < unsigned(h[1].y)) {
          const int2 t = h[0];
          h[0] = h[1], h[1] = t;
        }
      } else if (hits == 3) {
        order(first + 1, first), order(first + 2, first + 1), order(first + 1, first);
      } else if (hits == 4) {
        order(first + 1, first), order(first + 3, first + 2), order(first + 2, first), order(first + 3, first + 1), order(first + 2, first + 1);
      } else if (hits > 4) {
        for (int i = 1; i < hits; i++) {
          const int2 item = h[i];
          int j = i;
          while (j > 0 && unsigned(h[j - 1].y) < unsigned(item.y)) h[j] = h[j - 1], j--;
          h[j] = item;
        }
      }
      cur = items[--sp].x;  // the nearest; the others wait
    }
    if (dropped) continue;
    test_leaf(~cur);  // an Object leaf: the user callback (embree.cpp:24-40)
    er.tfar = __float_as_int(ray.tmax);
  }
  return hit;
}

// ... and its any-hit query, EmbreeAccel::hit (embree.cpp:143-165) = BVHNIntersector1<8, ...>::occluded
// (bvh_intersector1.cpp:117-195).  The order cannot change an any-hit answer; WHICH shapes are asked can: a shape is asked
// exactly when the ray enters its own box (and its ancestors') within [tnear, tfar], where pine's BVH asks every shape of a
// leaf whose UNION box is entered -- a Plane beyond its +-100 bounds (geometry.cpp:52) is found by the one and not by the other.
// And a query that starts with a negative tfar is answered "occluded" (rtcOccluded1 leaves such a ray alone, and
// embree.cpp:164 returns `tfar < 0`), where pine's BVH finds nothing: light samples with a negative distance reach this.
template <unsigned F, int STRIDE, class StackT>
__device__ __forceinline__ bool scene_occluded_embree(const SceneView& S, const DRay& ray_in, StackT* stack, TravLog* log) {
  if (ray_in.tmax < 0.0f) return true;
  DRay ray = ray_in;
  if constexpr (F & F_MESH)
    for (int k = 0; k < S.num_emesh; k++) {
      const DShape* sh = &S.leaf[S.emesh[k]];
      if (log) log->put(unsigned(sh->kind & kPrimIndexMask));
      const DRayOct oct = make_oct(ray);
      int prim = 0;
      if (mesh_traverse<true, STRIDE, F, StackT, true>(S, S.bvhs[as_int(sh->f[2])], ray, oct, stack, S.stack_top, prim, log)) return true;
    }
  if (S.etree_root == kEmbreeNoChild) return false;
  const EmbreeRay er = embree_ray(S, ray);
  int items[kEmbreeStackEntries];
  int sp = 1;
  items[0] = S.etree_root;
  while (sp > 0) {
    const int cur = items[--sp];
    if (cur < 0) {
      const DShape rec = load_leaf_record(&S.leaf[~cur]), *sh = &rec;
      const int word = sh->kind;
      if (log) log->put(unsigned(word & kPrimIndexMask));
      if (shape_hit<F>(word >> kPrimKindShift, sh, ray)) return true;
      continue;
    }
    embree_node_children(&S.etree[cur], er, [&](int child, int) { items[sp++] = child; });
  }
  return false;
}

// ANY: BVH::hit (bvh.cpp:497-511).  !ANY: BVH::intersect (bvh.cpp:513-548) minus the final
// compute_surface_info, which the caller does once for the winning primitive.
// geom_out receives the winning primitive's PACKED word (index | emissive bit | kind).
template <bool ANY, unsigned F, int STRIDE = kBlock, class StackT = int>
__device__ __forceinline__ bool scene_traverse(const SceneView& S, DRay& ray, StackT* stack, int& geom_out,
                                               int& prim_out, TravLog* log = nullptr) {
  if (S.num_shapes == 0) return false;
  if constexpr ((F & F_EMBREE) != 0) {
    if constexpr (ANY) return scene_occluded_embree<F, STRIDE>(S, ray, stack, log);
    else return scene_traverse_embree<F, STRIDE>(S, ray, stack, geom_out, prim_out, log);
  }
  const DRayOct oct = make_oct(ray);
  const DBvh top = S.bvhs[0];
  bool hit = false;
  auto leaf = [&](int start, int count) -> bool {
    for (int i = start; i < start + count; i++) {
      REGION(ANY ? 5 : 2);  // leaf primitive test
      const DShape rec = load_leaf_record(&S.leaf[i]), *sh = &rec;
      const int word = sh->kind;  // (the packed word rides in the copy's kind field)
      const int kind = word >> kPrimKindShift;
      bool is_mesh = false;
      if constexpr (F & F_MESH) is_mesh = kind == SHAPE_MESH;
      if (log) log->put(unsigned(word & kPrimIndexMask));
      if (is_mesh) {
        if constexpr (F & F_MESH) {
          const DBvh mb = S.bvhs[as_int(sh->f[2])];
          int prim = 0;
          const bool h = mesh_traverse<ANY, STRIDE, F>(S, mb, ray, oct, stack, S.stack_top, prim, log);
          if (ANY) {
            if (h) return true;
          } else if (h) {
            hit = true;
            geom_out = word;
            prim_out = prim;
          }
        }
      } else if (ANY) {
        if (shape_hit<F>(kind, sh, ray)) return true;
      } else if (shape_intersect<F>(kind, sh, ray)) {
        hit = true;
        geom_out = word;
      }
#ifdef PINE_DUP_SHAPES  /* cost-measurement builds only: run the selected shape tests a second time on an opaque copy of the ray */
      {
        const bool sel = PINE_DUP_SHAPES == 0 ? kind == SHAPE_RECT : kind == SHAPE_OBB;
        if (sel) {
          DRay rr = ray;
          asm volatile("" : "+v"(rr.tmin));
          const bool h2 = ANY ? shape_hit<F>(kind, sh, rr) : shape_intersect<F>(kind, sh, rr);
          float sink = h2 ? rr.tmax : 0.0f;
          asm volatile("" : : "v"(sink));
        }
      }
#endif
    }
    return false;
  };
  if (top.root_count > 0) {
    if (leaf(top.root_start, top.root_count)) return true;
    return hit;
  }
  if (top.root < 0) return false;  // geometries exist but none has primitives (only empty meshes): nothing to visit
  if (bvh2_walk<(ANY ? 4 : 1), F, STRIDE>(S, top.root, 0, ray, oct, stack, leaf)) return true;
  return hit;
}

}  // namespace pine_gpu
