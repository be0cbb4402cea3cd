/* include/pine_gpu.h -- C ABI of the MI355X-native PathIntegrator hot path (libpine_gpu.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repository wicstas/pine).  The reference exposes the path to scripts through its Context
 * reflection table (src/pine/core/context.h:235-609, registered in
 * src/pine/core/program_context.cpp:23-125); INTEGRATION.md shows the thunks a pine maintainer
 * would register to route `PathIntegrator(...).render(scene)` through this library.
 *
 * Conventions: every function returning int returns 0 (or a non-negative id) on success and a
 * negative value on failure, with a message available from pine_gpu_last_error() (the reference
 * aborts through SEVERE, src/pine/core/log.h:45-51; nothing aborts across this ABI).  Vectors are
 * float[3]; matrices are float[16] in the reference's storage order (column vectors,
 * src/pine/core/vecmath.h:575-640), i.e. m[c*4 + r].  Thread-safety: a scene may be built from one
 * thread at a time; rendering distinct plans from distinct threads is safe; pine_gpu_progress() may
 * be polled from any thread (src/cli/pine.cpp:36-40 does exactly that).
 */
#ifndef PINE_GPU_H
#define PINE_GPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PINE_GPU_ABI_VERSION 4

typedef struct pine_gpu_scene pine_gpu_scene; /* replaces pine::Scene, src/pine/core/scene.h:14-43 */
typedef struct pine_gpu_plan pine_gpu_plan;   /* a PathIntegrator bound to a scene + device state */

/* ---- errors / progress ------------------------------------------------------------------ */
const char* pine_gpu_last_error(void);  /* thread-local message of the last failing call */
float pine_gpu_progress(void);          /* get_progress(), src/pine/core/integrator.cpp:17-19 */
int pine_gpu_abi_version(void);

/* ---- host math used by scene scripts (PRL builtins) ---------------------------------------
 * translate/scale/rotate_x|y|z/look_at: src/pine/core/vecmath.h:1102-1180; operator*(mat4,mat4)
 * :617-624; inverse(mat4): src/pine/core/vecmath.cpp:103-132.  Same operand order, same libm. */
void pine_gpu_mat4_identity(float out[16]);
void pine_gpu_mat4_translate(const float v[3], float out[16]);
void pine_gpu_mat4_scale(const float v[3], float out[16]);
void pine_gpu_mat4_rotate_x(float rad, float out[16]);
void pine_gpu_mat4_rotate_y(float rad, float out[16]);
void pine_gpu_mat4_rotate_z(float rad, float out[16]);
void pine_gpu_mat4_mul(const float a[16], const float b[16], float out[16]);
void pine_gpu_mat4_inverse(const float m[16], float out[16]);
void pine_gpu_mat4_look_at(const float from[3], const float at[3], float out[16]);
/* what the reference's glTF import composes node transforms from (src/pine/core/fileio.cpp:127-169): q2m(w, x, y, z), the
 * matrix's scalar constructor (row-major arguments) and transpose */
void pine_gpu_mat4_from_quaternion(float w, float x, float y, float z, float out[16]);
void pine_gpu_mat4_from_rows(const float rows[16], float out[16]);
void pine_gpu_mat4_transpose(const float m[16], float out[16]);

/* ---- Scene ---------------------------------------------------------------------------------
 * Scene(): src/pine/core/scene.cpp:64-79 (`Scene` ctor + `add`/`set` methods). */
pine_gpu_scene* pine_gpu_scene_create(void);
void pine_gpu_scene_destroy(pine_gpu_scene* scene);

/* scene.add(name, Material): Scene::add_material src/pine/core/scene.cpp:8-13.  Constant shading
 * nodes only (Node3f/Nodef literals).  Returns the material id.  A later add with the same name
 * shadows the earlier one, as the reference's map assignment does. */
int pine_gpu_scene_add_material_emissive(pine_gpu_scene*, const char* name, const float color[3]);
                                         /* Emissive(Node3f)   src/pine/core/material.h:18-28  */
int pine_gpu_scene_add_material_diffuse(pine_gpu_scene*, const char* name, const float albedo[3]);
                                         /* Diffuse(Node3f)    src/pine/core/material.h:30-37  */
int pine_gpu_scene_add_material_uber(pine_gpu_scene*, const char* name, const float albedo[3],
                                     float roughness, float metallic, float transmission, float ior);
                                         /* Uber(...)          src/pine/core/material.h:80-97  */
int pine_gpu_scene_add_material_subsurface(pine_gpu_scene*, const char* name, const float albedo[3],
                                           float roughness, const float sigma_s[3]);
                                         /* Subsurface(...)    src/pine/core/material.h:99-110 */
int pine_gpu_scene_find_material(pine_gpu_scene*, const char* name);
                                         /* Scene::find_material src/pine/core/scene.cpp:49-54 */

/* scene.add(Light) / scene.set(EnvironmentLight): Scene::add_light, set_env_light src/pine/core/scene.cpp:29-46.
 * PointLight / SpotLight / DirectionalLight (delta lights: sampled without MIS, path.cpp:104-106) and
 * the Sky environment light (added to radiance on a miss, path.cpp:75-81; sampled uniformly over the
 * sphere): src/pine/core/light.h:21-67, light.cpp:11-84.  Lights enter the light sampler's list in
 * add order together with the area lights of emissive geometry; the environment light comes last
 * (lightsampler.cpp:6-10).  ImageSky (light.cpp:127-171): an image over the sphere, sampled by the reference's
 * Distribution2D of its texels' lengths and looked up bilinearly on a miss.  Setting an environment light
 * replaces the previous one.  Atmosphere (light.cpp:94-125): the single-scattering Rayleigh / Mie sky of color.cpp:41-98 with a
 * sun disc, sampled by the Distribution2D of its own colours over an image_size grid and evaluated per ray on a miss. */
int pine_gpu_scene_add_light_point(pine_gpu_scene*, const float position[3], const float color[3]);
int pine_gpu_scene_add_light_spot(pine_gpu_scene*, const float position[3], const float direction[3],
                                  const float color[3], float falloff_radian, float cutoff_additional_radian);
int pine_gpu_scene_add_light_directional(pine_gpu_scene*, const float direction[3], const float color[3]);
int pine_gpu_scene_set_env_sky(pine_gpu_scene*, const float sun_color[3]);
/* ImageSky(image, tint, elevation, rotation): w x h texels of 3 floats, rows top first (a Radiance HDR image as the reference
 * loads it).  Refused with an error: a texel that is negative or not finite, w or h < 1, more than 2^26 texels. */
int pine_gpu_scene_set_env_image(pine_gpu_scene*, const float* rgb, int w, int h, const float tint[3], float elevation, float rotation);
/* ... of an 8-bit image (the reference's vec3u8 images): each texel becomes pow(value / 255, 2.2) here, once. */
int pine_gpu_scene_set_env_image_u8(pine_gpu_scene*, const uint8_t* rgb, int w, int h, const float tint[3], float elevation, float rotation);
/* Atmosphere(sun_direction, sun_color, image_size): the reference's image_size is 1024 x 1024 (scripts cannot change it).  The
 * light's tables -- its colour at every grid point, about 100 expf each -- are computed by a kernel on `device`, or, device = -1,
 * by the same function on host threads (at most min(16, $OMP_NUM_THREADS, hardware threads)): the same bytes either way.
 * Refused with an error: a sun direction that is zero or not finite, a sun colour that is not finite, image_w or image_h < 1,
 * more than 2^22 texels, device >= 0 where there is no such device. */
int pine_gpu_scene_set_env_atmosphere(pine_gpu_scene*, const float sun_direction[3], const float sun_color[3], int image_w, int image_h, int device);

/* Shading nodes (Nodef / Node3f: src/pine/core/node.h:13-297, registered node.cpp:29-116).  A node
 * lives in the scene's node table; each call returns its id (or < 0).  Supported: constants, the
 * surface inputs Position / Normal / UV, NodeBinary (+ - * / ^), NodeUnary (- abs sqr sqrt fract),
 * NodeComponent, NodeToVec3, NodeCheckerboard, NodeImage / NodeImagef (`Texture`); `lerp` etc. are
 * compositions of these exactly as node.cpp:88-102 composes them; NodeNoisef / NodeNoise3f.  Not supported: function
 * nodes.  Subtrees that do not read the surface are folded to literals on the host with the same float
 * operations (a `Texture` of a constant coordinate included); the rest run as small postfix programs in
 * the shading stage of the kernels. */
int pine_gpu_scene_node_constf(pine_gpu_scene*, float value);                 /* Nodef(float)   node.h:262 */
int pine_gpu_scene_node_const3(pine_gpu_scene*, const float value[3]);        /* Node3f(vec3)   node.h:281 */
int pine_gpu_scene_node_input(pine_gpu_scene*, int which);                    /* 0 Position, 1 Normal, 2 UV  node.h:113-127 */
int pine_gpu_scene_node_binary(pine_gpu_scene*, int op, int a, int b);        /* op: one of + - * / ^ (as a char); both Nodef or both Node3f  node.h:129-152 */
int pine_gpu_scene_node_unary(pine_gpu_scene*, int op, int a);                /* '-' neg, 'a' abs, 's' sqr, 'r' sqrt, 'f' fract  node.h:154-178 */
int pine_gpu_scene_node_component(pine_gpu_scene*, int a, int component);     /* NodeComponent(Node3f, 0..2) node.h:180-193 */
int pine_gpu_scene_node_to_vec3(pine_gpu_scene*, int x, int y, int z);        /* NodeToVec3(x) when y = z = -1  node.h:195-210 */
int pine_gpu_scene_node_checkerboard(pine_gpu_scene*, int p, float ratio);    /* NodeCheckerboard node.h:232-239, node.cpp:15-18 */
int pine_gpu_scene_node_splat(pine_gpu_scene*, int a);                        /* a Nodef where a Node3f is expected  node.h:78,291-293 */
int pine_gpu_scene_node_is_vec3(pine_gpu_scene*, int id);                     /* 1 Node3f, 0 Nodef */
/* Images for NodeImage / NodeImagef (image.h:11-25), rows as loaded (nothing is flipped); each call returns the image's id.
 * Float texels (Array2d<vec3>: 3 per texel, finite) are kept as they are.  8-bit texels (Array2d<vec3u8> / <vec4u8>:
 * `channels` 3 or 4) are kept as one word each and linearised on lookup, pow(value / 255, 2.2) (image.cpp:10-13); the alpha
 * of a 4-channel image never reaches a result, as in vec3(vec4).  Refused: w or h below 1, more than 2^26 texels, a float
 * texel that is not finite, `channels` other than 3 or 4. */
int pine_gpu_scene_add_image(pine_gpu_scene*, const float* rgb, int w, int h);
int pine_gpu_scene_add_image_u8(pine_gpu_scene*, const uint8_t* texels, int channels, int w, int h);
/* NodeImage(p, image) -> Node3f, NodeImagef(p, image) -> Nodef (its .x)  node.h:236-251, node.cpp:20-27: the texel at
 * min(vec2i(size * fract(vec2(p))), size - 1) -- nearest, repeating, unfiltered.  Where a coordinate is not finite the
 * reference's float-to-int conversion is undefined; here that axis reads texel 0.  Refused: an image id that does not exist,
 * a `p` that is not a Node3f. */
int pine_gpu_scene_node_image(pine_gpu_scene*, int p, int image);
int pine_gpu_scene_node_imagef(pine_gpu_scene*, int p, int image);
/* NodeNoisef(p, octaves) -> Nodef, NodeNoise3f(p, octaves) -> Node3f  node.h:209-225, node.cpp:7-13: fbm(p, int(octaves)) and
 * fbm3d(p, int(octaves)) of noise.cpp:29-41, 63-75 -- Perlin gradient noise, summed over `octaves` rounds of doubled frequency
 * and halved weight; Noisef equals the first component of Noise3f.  The octaves value truncates to int and may differ per
 * surface point; fewer than one round gives the reference's 0 / 0, a NaN.  The rounds are bounded by 32: a value above it
 * (+inf included) runs 32, a NaN none.  Pinned to the reference for |p| * 2^(octaves - 1) < 2^30.  Refused, each by the node's
 * name: a `p` that is not a Node3f, an `octaves` that is not a Nodef, an id out of range, a constant octaves above 32 or not
 * finite. */
int pine_gpu_scene_node_noisef(pine_gpu_scene*, int p, int octaves);
int pine_gpu_scene_node_noise3f(pine_gpu_scene*, int p, int octaves);
/* Materials whose parameters are nodes (albedo: Node3f; the others: Nodef). */
int pine_gpu_scene_add_material_diffuse_n(pine_gpu_scene*, const char* name, int albedo);
int pine_gpu_scene_add_material_uber_n(pine_gpu_scene*, const char* name, int albedo, int roughness, int metallic,
                                       int transmission, float ior);
int pine_gpu_scene_add_material_metal(pine_gpu_scene*, const char* name, int albedo, int roughness);
                                         /* Metal(Node3f, Nodef)         src/pine/core/material.h:39-50 */
int pine_gpu_scene_add_material_glossy(pine_gpu_scene*, const char* name, int albedo, int roughness, int ior);
                                         /* Glossy(Node3f, Nodef, Nodef) src/pine/core/material.h:52-64 */
int pine_gpu_scene_add_material_glass(pine_gpu_scene*, const char* name, int albedo, int roughness, int ior);
                                         /* Glass(Node3f, Nodef, Nodef)  src/pine/core/material.h:66-78 */

/* scene.add(Shape, material): Scene::add_geometry src/pine/core/scene.cpp:14-22 (emissive geometry
 * becomes an AreaLight automatically).  Returns the geometry index.  Shape constructors:
 * src/pine/core/geometry.cpp:901-946. */
int pine_gpu_scene_add_rect(pine_gpu_scene*, const float position[3], const float ex[3],
                            const float ey[3], int flip_normal, int material);
                                         /* Rect(vec3,vec3,vec3,bool) geometry.cpp:255-267 */
int pine_gpu_scene_add_aabb(pine_gpu_scene*, const float lower[3], const float upper[3], int material);
                                         /* Box(vec3,vec3) = AABB     bbox.h:29-33         */
int pine_gpu_scene_add_obb(pine_gpu_scene*, const float lower[3], const float upper[3],
                           const float m[16], int material);
                                         /* Box(AABB,mat4) = OBB      bbox.cpp:144         */
int pine_gpu_scene_add_sphere(pine_gpu_scene*, const float center[3], float radius, int material);
                                         /* Sphere(vec3,float)        geometry.cpp:72      */
int pine_gpu_scene_add_disk(pine_gpu_scene*, const float position[3], const float normal[3],
                            float radius, int material);
                                         /* Disk(vec3,vec3,float)     geometry.cpp:123-127 */
int pine_gpu_scene_add_cone(pine_gpu_scene*, const float position[3], const float normal[3],
                            float radius, float height, int material);
                                         /* Cone(vec3,vec3,float,float) geometry.cpp:409-414 */
int pine_gpu_scene_add_plane(pine_gpu_scene*, const float position[3], const float normal[3], int material);
                                         /* Plane(vec3,vec3)          geometry.cpp:31-34   */
int pine_gpu_scene_add_line(pine_gpu_scene*, const float p0[3], const float p1[3], float thickness,
                            int material);
                                         /* Line(vec3,vec3,float)     geometry.cpp:171-179 */
int pine_gpu_scene_add_cylinder(pine_gpu_scene*, const float p0[3], const float p1[3], float radius,
                                int material);
                                         /* Cylinder(vec3,vec3,float) geometry.h:140-141 (side surface only;
                                            not usable as a light, as in the reference)    */
int pine_gpu_scene_add_triangle(pine_gpu_scene*, const float v0[3], const float v1[3], const float v2[3],
                                int material);
                                         /* Triangle(vec3,vec3,vec3)  geometry.cpp:528-531 */
/* Mesh(vertices, indices, texcoords, normals) geometry.cpp:596-604: per-vertex normals (interpolated shading normal,
 * geometry.h:199-204) and / or texture coordinates (:205-210), as the reference's glTF import produces them; either may be
 * null.  pine_gpu_mesh_apply: Mesh::apply(mat4) geometry.cpp:647-653 in place on caller arrays (the import applies a node's
 * accumulated transform to its mesh before adding it). */
int pine_gpu_scene_add_mesh_full(pine_gpu_scene*, const float* vertices, int num_vertices, const uint32_t* indices, int num_triangles,
                                 const float* normals, const float* texcoords, int material);
int pine_gpu_mesh_apply(float* vertices, int num_vertices, float* normals, const float m[16]);

/* State-level forms, for a binding that walks an already constructed pine::Scene (examples/adapter):
 * the members the reference's shape object keeps, exactly as stored -- a constructed Rect / Disk / Plane / Cone holds
 * NORMALISED axes and derived lengths that do not invert to its constructor arguments bit for bit.  (Sphere, Box,
 * Line, Cylinder and Mesh store their constructor arguments: use the calls above.)  Member lists:
 * Rect geometry.h:92-96, Disk :56-60, Plane :23-25, Cone :134-140 (bottom_position = its Disk's centre), Triangle :115-117. */
int pine_gpu_scene_add_rect_state(pine_gpu_scene*, const float position[3], const float ex[3], const float ey[3], const float n[3],
                                  float lx, float ly, const float rx[3], const float ry[3], int material);
int pine_gpu_scene_add_disk_state(pine_gpu_scene*, const float position[3], const float n[3], const float u[3], const float v[3],
                                  float r, int material);
int pine_gpu_scene_add_plane_state(pine_gpu_scene*, const float position[3], const float n[3], const float u[3], const float v[3],
                                   int material);
int pine_gpu_scene_add_cone_state(pine_gpu_scene*, const float apex[3], const float n[3], float r, float h, float A, float A2, float S,
                                  const float bottom_position[3], int material);
int pine_gpu_scene_add_triangle_state(pine_gpu_scene*, const float v0[3], const float v1[3], const float v2[3], const float n[3],
                                      int material);
int pine_gpu_scene_add_mesh(pine_gpu_scene*, const float* vertices, int num_vertices,
                            const uint32_t* indices, int num_triangles, int material);
                                         /* Mesh(vertices, indices)   geometry.cpp:601-609 */

/* scene.set(ThinLenCamera(Film(size, tonemapper), from, to, fov[, len_radius, focus_distance])):
 * src/pine/core/camera.cpp:7-16,40-45; Film src/pine/core/film.h:24-27.
 * tonemapper: 0 = Uncharted2, 1 = ACES (used only by pine_gpu_film_finalize). */
int pine_gpu_scene_set_camera_thinlens(pine_gpu_scene*, int film_w, int film_h, int tonemapper,
                                       const float from[3], const float to[3], float fov,
                                       float len_radius, float focus_distance);

/* State-level form: the members of a constructed ThinLenCamera (src/pine/core/camera.h:21-26); c2w = its mat3, 9 floats,
 * columns x, y, z. */
int pine_gpu_scene_set_camera_thinlens_state(pine_gpu_scene*, int film_w, int film_h, int tonemapper, const float position[3],
                                             const float c2w[9], const float fov2d[2], float len_radius, float focus_distance);

/* Test hooks: the 128-byte device record of geometry `index` (30 floats of state, kind, material: pine_types.h DShape)
 * and the camera record -- what constructor-level and state-level calls must agree on. */
int pine_gpu_scene_shape_record(pine_gpu_scene*, int index, float out[32]);
int pine_gpu_scene_camera_record(pine_gpu_scene*, float out[20]);

/* Text dump of the scene as it was built (the .pscene exchange format, pine_amd/scene_io.py).
 * Returns the number of bytes needed (excluding NUL); writes at most `capacity` bytes. */
int64_t pine_gpu_scene_describe(pine_gpu_scene*, char* buf, int64_t capacity);

/* Host-side accel build only (no GPU): BVH::build src/pine/impl/accel/bvh.cpp:453-495.
 * Returns node count; optional dumps for tests: nodes as 16 x int32/float32 words each. */
int pine_gpu_scene_build_accel(pine_gpu_scene*);
int64_t pine_gpu_scene_accel_dump(pine_gpu_scene*, void* nodes_out, int64_t node_capacity_bytes,
                                  int32_t* prims_out, int64_t prim_capacity);

/* ---- PathIntegrator ------------------------------------------------------------------------
 * PathIntegrator(Accel, Sampler, LightSampler, int) + render(Scene&):
 * src/pine/impl/integrator/path.cpp:7-41, registered program_context.cpp:76-81.  The sampler is
 * BlueSampler(spp) (src/pine/core/sampler.cpp:115-121: spp rounded up to a power of two, clamped
 * to 256) or SobolSampler(spp), the light sampler UniformLightSampler, the accel pine's BVH order.
 */
typedef struct {
  int32_t spp;             /* requested samples per pixel (BlueSampler argument)            */
  int32_t max_path_length; /* PathIntegrator depth argument (> 0)                           */
  int32_t device;          /* HIP device ordinal                                            */
  int32_t shard_rank;      /* this process renders tiles t with t % shard_world == rank     */
  int32_t shard_world;     /* 1 = whole film                                                */
  int32_t samples_per_item;/* 0 = auto; work item = this many consecutive samples of a pixel */
  int32_t flags;           /* PINE_GPU_FLAG_*                                               */
  int32_t sampler;         /* PINE_GPU_SAMPLER_*: which Sampler the PathIntegrator is constructed with   */
} pine_gpu_render_params;

#define PINE_GPU_SAMPLER_BLUE  0 /* BlueSampler(spp)  src/pine/core/sampler.h:166-201 (the default)           */
#define PINE_GPU_SAMPLER_SOBOL 1 /* SobolSampler(spp) src/pine/core/sampler.h:83-164, sampler.cpp:81-113: spp
                                    as given (no clamp to 256, any count); on the device up to 4096 (a count that is
                                    not a power of two renders one work item per pixel)                      */
#define PINE_GPU_SAMPLER_HALTON 2 /* HaltonSampler(spp) src/pine/core/sampler.h:40-81, sampler.cpp:39-79,
                                    lowdiscrepancy.h:26-51: scrambled radical inverses over the first primes; on the
                                    device under SobolSampler's limit (4096 samples per pixel)               */

#define PINE_GPU_FLAG_TIMING 1 /* record per-kernel HIP-event timings for the roofline report */
#define PINE_GPU_FLAG_PROGRESS 2 /* the kernels post the claimed work-item count to host memory now and then, so that
                                    pine_gpu_progress() moves while a launch runs (pine_gpu_path_render sets it itself) */
#define PINE_GPU_FLAG_FAST 4 /* declared-tolerance arithmetic instead of bit-exact parity with the reference: contracted
                                    multiply-adds, 1-ulp hardware reciprocal / square root / division, the device's native
                                    sin / cos / pow / log.  Integer work -- sampler, RNG, hash -- stays exact.  Declared tolerance
                                    (tests/test_gpu_parity.py FAST_TOLERANCE): where the path depends continuously on the
                                    float bits (Rect-only cbox) >= 99.9 % of the pixels are within relative L2 1e-4 of the exact film (RMSE 4e-6); where the
                                    reference's algorithm decides on nearly equal numbers (scaled OBBs, grazing cones, near-delta
                                    lobes) 0.8 - 2 % of the samples take another path and the films agree as Monte-Carlo estimates:
                                    RMSE at 256 spp <= 4e-3 (cbox) / 2e-2 (10 000 cones), bias of the image mean <= 5e-3.  Only
                                    scenes one of the fast variants covers (the BASELINE scenes' feature sets); others fail with a
                                    message.  Never the default, never the parity gate. */
#define PINE_GPU_FLAG_DEVICE_BVH 8 /* build the BVH on the GPU (the same level-synchronous binned-SAH build as on the host, same tree, same
                                    primitive order: pine_amd/csrc/pine_bvh_build_device.h) when the plan is the first to need the scene's
                                    accel.  pine_gpu_plan_stats.accel_built_on_device says what happened. */
#define PINE_GPU_FLAG_DEBUG_FORCE_BAIL 0x100 /* test hook: the stage-queued path kernel raises its protocol-failure
                                    bail-out at once; every synchronising entry point must then FAIL (never return the film) */
/* Scene-specialised kernels.  The path kernel can be compiled FOR THE SCENE: (1) with exactly the scene's
 * feature set (shape kinds, material lobes, node programs, light kinds, sampler) instead of the nearest precompiled superset;
 * (2) small scenes without meshes (at most 10 primitives: cbox-class) get their BVH and every primitive record baked into the
 * kernel as immediates, the traversal fully unrolled; a small top level around ONE mesh becomes code run where a ray is
 * created, and only rays that reach the mesh enter the traversal stages.  Same tests in pine's order: bit-identical films;
 * cbox 24 % faster, the Subsurface icosphere 46 %.  A build is one `hipcc --genco` run in a child process (seconds), cached
 * on disk by content ($PINE_GPU_CACHE_DIR, else ~/.cache/pine_gpu); it needs hipcc and this library's device headers.
 *
 * DEFAULT (no flag) -- automatic, never in the caller's way: a code object already in the cache is loaded at plan creation
 * (about a millisecond); otherwise the compiler runs in the BACKGROUND while the precompiled kernel renders, and the first
 * launch after it has finished -- of this plan or of any later plan or pine_gpu_path_render call on the same geometry -- runs
 * the scene's own kernel.  Nothing fails because of it: no compiler, no headers, no cache directory or a full compile queue
 * leave the precompiled kernel in place.  What ran is in pine_gpu_plan_stats (`specialized`, `specialize_source`,
 * `specialize_pending`).  $PINE_GPU_SPECIALIZE=0 (or PINE_GPU_FLAG_NO_SPECIALIZE): precompiled kernels only. */
#define PINE_GPU_FLAG_SPECIALIZE 0x400 /* the caller WANTS the scene's kernel from the first launch: plan creation waits for the
                                    compiler, and a kernel that cannot be built fails the plan.  A scene with nothing to gain
                                    renders with the precompiled kernel.  Also $PINE_GPU_SPECIALIZE=1 (every plan). */
#define PINE_GPU_FLAG_SPECIALIZE_NO_BAKE 0x800 /* (either mode) the exact feature set only, never the baked scene --
                                    for geometry that changes from render to render (an animation): a baked kernel is keyed by
                                    the geometry and would be compiled per frame, a feature-set kernel once */
#define PINE_GPU_FLAG_SPECIALIZE_ASYNC 0x1000 /* with PINE_GPU_FLAG_SPECIALIZE: plan creation does not wait for the compiler -- the
                                    background build of the default mode, but a build that fails is reported (plan stats:
                                    specialized == -1) instead of passing silently */
#define PINE_GPU_FLAG_NO_SPECIALIZE 0x2000 /* the precompiled kernel table only: no cache lookup, no background compiler */
#define PINE_GPU_FLAG_ORDER_EMBREE 0x4000 /* closest-hit queries hand the scene's non-mesh shapes to their tests in the order of the reference's
                                    DEFAULT accel, EmbreeAccel (src/pine/impl/accel/embree.cpp:101-143,195-257; what a .pine script's
                                    PathIntegrator(sampler, n) gets on real pine, program_context.cpp:79-81), instead of pine-BVH order.  pine
                                    registers every such shape as one Embree user primitive with pine's own bounds and intersect callbacks, so
                                    Embree decides only the ORDER -- and pine has shapes whose answer depends on it: the scaled
                                    Box(AABB, mat4) (src/pine/core/bbox.cpp:149-171), Plane's finite bounds, Line, Cylinder.  The order is
                                    restated from the vendored Embree 4.3.1's BVH8 builder and single-ray traverser as an AVX2 x86 host runs
                                    them (pine_amd/csrc/pine_embree_order.h, scene_traverse_embree); the films of the real reference built
                                    with EmbreeAccel are reproduced bit for bit (tests/golden/film_embree_*, any number of shapes), without
                                    the flag (the default, and the parity gate) those of Accel(BVH()).  Meshes are Embree triangle
                                    geometry there: they are asked first, through Embree's own Moeller-Trumbore test and barycentrics
                                    (restated too); only an exact tie in t between coplanar triangles of different meshes is decided by
                                    Embree's own triangle hierarchy, which is not.  Not with _FAST. */
#define PINE_GPU_FLAG_ORDER_NEAREST PINE_GPU_FLAG_ORDER_EMBREE /* (the name of this flag before the order was Embree's own for any shape count) */
#define PINE_GPU_FLAG_VERTEX_LOG 0x200 /* test hook: choose the kernel variant compiled with the per-vertex log (pine_gpu_plan_vertex_log) */

/* Multi-GPU partition: rank that owns pixel (x, y) of a film_w-wide film when 8x8-pixel tiles are
 * dealt round-robin to `world` ranks (host-side helper; the kernels use the same mapping). */
int pine_gpu_shard_of_pixel(int film_w, int x, int y, int world);

/* Path to the packed BlueSobol tables (pine_amd/data/bluesobol_u8.bin).  Optional: without it the library looks at
 * $PINE_GPU_TABLES, then at ../data/bluesobol_u8.bin relative to the directory libpine_gpu.so was loaded from. */
int pine_gpu_set_table_path(const char* path);

/* One-shot, drop-in form: render into a HOST film of W*H float4 (row 0 first, exactly
 * Array2d<vec4>, src/pine/core/array.h:51-55); includes upload + download.  Fails if no GPU. */
int pine_gpu_path_render(pine_gpu_scene*, const pine_gpu_render_params*, float* film_out_host);

/* The same on several devices of one node from ONE process (`pine_gpu_path_render(..., device_mask, ...)`):
 * shard r of n -- 8x8-pixel tiles dealt round-robin, SURVEY.md 8(e) -- renders on the r-th selected device; the per-device
 * tile slabs travel to the first device with peer copies (xGMI), are scattered into the film there and downloaded.  The film
 * is bit-identical to the one-device film.  `prm->device / shard_rank / shard_world` are ignored.  The reference's
 * counterpart is its thread pool over one shared film (src/pine/core/parallel.h:19-67, path.cpp:31-39).
 * _multi: bit d of `device_mask` selects HIP device d.  _devices: an explicit list (a device may appear more than once). */
int pine_gpu_path_render_multi(pine_gpu_scene*, const pine_gpu_render_params*, uint64_t device_mask, float* film_out_host);
int pine_gpu_path_render_devices(pine_gpu_scene*, const pine_gpu_render_params*, const int* devices, int num_devices,
                                 float* film_out_host);

/* Resident form (bench / multi-GPU): build device state once, launch many times.
 * `film_dev` is a DEVICE pointer to W*H float4; `stream` is a hipStream_t (0 = default stream).
 * Pixels outside this rank's shard are written as zeros, so a sum-reduce over ranks is exact. */
pine_gpu_plan* pine_gpu_plan_create(pine_gpu_scene*, const pine_gpu_render_params*);
/* Device memory of destroyed plans (the per-sample radiance buffer of a 640 x 640 x 256 render is 1.7 GB) is kept for the next
 * plan instead of being returned to the driver: a one-shot pine_gpu_path_render spends most of its time outside the kernels in
 * hipMalloc / hipFree otherwise.  At most $PINE_GPU_POOL_MB (default 16 384; 0 = keep nothing) per process; this call
 * returns all of it, and drops the process's table of loaded scene kernels (the last 16 code objects stay loaded per device so
 * that the next plan of the same geometry does not load its kernel again).  The reference has no counterpart (its film and per-thread state live in host memory). */
void pine_gpu_release_cached_memory(void);
int pine_gpu_plan_launch(pine_gpu_plan*, void* film_dev, void* stream);
void pine_gpu_plan_destroy(pine_gpu_plan*);

/* Multi-GPU without moving the zeros: the rank writes only its own tiles, tile-major, into a slab
 * of pine_gpu_packed_slab_floats(...) floats ([local tile][pixel in 8x8 tile] float4; equal size on
 * every rank, the last tile may be padding); the slabs are gathered to one rank ([rank][slab]) and
 * pine_gpu_film_unpack scatters them into the row-major W*H float4 film there.  This replaces the
 * reference's shared-memory film (src/pine/impl/integrator/path.cpp:38 writes film[p] from any
 * thread) across devices.  pine_gpu_packed_offset is the host-side statement of the same mapping. */
int pine_gpu_plan_launch_packed(pine_gpu_plan*, void* slab_dev, void* stream);
int64_t pine_gpu_packed_slab_floats(int film_w, int film_h, int world);
int pine_gpu_packed_offset(int film_w, int film_h, int world, int x, int y, int* rank_out, int64_t* float4_index_out);
int pine_gpu_film_unpack(int film_w, int film_h, int world, int device, const void* slabs_dev, void* film_dev, void* stream);

typedef struct {
  uint64_t camera_samples;   /* samples this plan renders per launch (its shard)              */
  uint64_t vertices;         /* radiance() invocations of the last launch    */
  uint64_t shadow_rays;
  float trace_ms;            /* path kernel, HIP events on the launch stream: mean over the launches   */
  float resolve_ms;          /* ordered per-pixel sum kernel                since the previous stats_get */
  float prepass_ms;          /* RNG checkpoint kernel                       (at most the last 64)       */
  int32_t spp_effective;
  int32_t samples_per_item;
  int32_t grid_blocks;
  int32_t block_threads;
  int32_t lds_bytes;
  int32_t timed_launches;    /* number of launches the three timings are averaged over        */
  uint64_t walk_steps;       /* BSSRDF random-walk steps of the last launch (bxdf.cpp:340-351; stage-queued kernel) */
  float accel_build_ms;      /* host: BVH build + flattening for this plan (0 if the scene's accel was already built) */
  float upload_ms;           /* host: device allocation + upload of scene, tables and work buffers at plan creation  */
  int32_t accel_built_on_device; /* 1: that build ran on the GPU (PINE_GPU_FLAG_DEVICE_BVH)                            */
  int32_t serial_tiles;      /* tile classes (Subsurface scenes): 8x8 tiles of this shard whose pixels are one whole-pixel item each
                              * because a camera ray of theirs can reach a Subsurface shape; the others' samples are independent
                              * items of samples_per_item samples.  0: one class (samples_per_item describes every item) */
  int32_t specialized;       /* 0 a precompiled kernel runs (no gain possible, specialisation off, or a background build is still
                              * running); 1 a kernel compiled for this scene's exact feature set; 2 ... with the scene's BVH and
                              * primitive records baked in as well; -1 a background build failed, the precompiled kernel keeps running */
  float specialize_ms;       /* host: generating + compiling (or fetching from the cache) + loading that kernel at plan creation */
  uint32_t kernel_features;  /* feature bits (pine_device.h F_*) of the path kernel in use */
  int32_t specialize_source; /* where the scene's kernel came (or will come) from: 0 none; 1 the on-disk cache; 2 compiled at plan
                              * creation (PINE_GPU_FLAG_SPECIALIZE); 3 compiled in the background by this process           */
  int32_t specialize_pending;/* 1: a background build is still running (the precompiled kernel renders meanwhile)             */
  int32_t tiles_in_kernel;   /* 8x8 tiles of the last launch that the path kernel summed itself (its owned tiles); the resolve
                              * kernel summed the others */
} pine_gpu_plan_stats;
/* PINE_GPU_FLAG_SPECIALIZE, host half: the text plan creation would compile for this scene (its BVH as straight-line code,
 * boxes and primitive records as hexadecimal float literals), NUL-terminated into out[0..cap) when it fits; returns its
 * length, 0 when the scene does not qualify (meshes, a BVH too large to unroll, a non-finite record), < 0 on error.
 * Needs no GPU: a way to see what was compiled, and the CPU tests' handle on the generator. */
int64_t pine_gpu_scene_specialized_source(pine_gpu_scene*, char* out, int64_t cap);
/* ... and the compile step on its own (no GPU needed: hipcc cross-compiles): the scene's kernel for the stage-queued variant
 * <features, ctx> (pine_variants.h; the kernel's name carries features | F_BAKED) and `arch` ("gfx950"), through the same cache
 * plan creation uses; the code object's path into path_out.  A null scene compiles level 1: <features, ctx> as given, generic
 * traversal (tools/compile_sweep.py walks feature combinations with it).  Returns 1 on a cache hit, 0 after a compiler run, < 0 on failure.  Build check + tests. */
int pine_gpu_test_specialize_compile(pine_gpu_scene*, uint32_t features, int ctx, const char* arch, char* path_out, int64_t cap);
/* The scene's BVH built on HIP device `device` right now (the accel is then reused by every later plan); returns the node
 * count, < 0 on failure.  pine_gpu_scene_accel_dump shows the result: identical to the host build's. */
int pine_gpu_scene_build_accel_device(pine_gpu_scene*, int device);
/* Blocks until the last launch has finished (needed to read the device-side counters).  Fails (< 0) if the
 * path kernel of that launch bailed out of a bounded wait: its film is incomplete. */
int pine_gpu_plan_stats_get(pine_gpu_plan*, pine_gpu_plan_stats* out);
/* For callers that launch asynchronously and read the film themselves: blocks until the plan's last launch
 * has finished; 0 = it completed, < 0 = its path kernel bailed out (pine_gpu_last_error() names the wait that
 * ran out) and the film must be discarded.  The reference has no counterpart: its render() cannot fail part-way. */
int pine_gpu_plan_check(pine_gpu_plan*);

/* Diagnostic builds only (-DPINE_PROFILE_SECTIONS): per-section wave-cycle sums of the last launch
 * (all zeros in the product build). */
int pine_gpu_plan_debug_sections(pine_gpu_plan*, uint64_t out[16]);
/* Test hook (stage-queued kernel): the per-vertex terms of path.cpp:98-121 of every path of a small film.  Called with
 * out == NULL it switches the log on for the plan's next launches and returns the number of floats; called with a buffer
 * after a launch it copies the log: 16 floats per radiance() invocation at
 * [((y * W + x) * spp + sample) * max_path_length + level] = kind (0 miss, 1 emissive, 2 path-length limit, 3 shaded) |
 * length | direct term (3) | bs.f (3) | cosine | bs.pdf | is_delta | mis | returned light pdf (-1: none) | returned Lo (3)
 * -- the record `pine_ref vertices` writes from the reference's own objects (tests/golden/vertices_*.npz).  The plan must have
 * been created with PINE_GPU_FLAG_VERTEX_LOG: only two kernel variants (cbox's kinds; everything but Subsurface) carry the hook. */
int64_t pine_gpu_plan_vertex_log(pine_gpu_plan*, float* out, int64_t capacity_floats);

/* Per-sample radiance of the last launch: copies spp_eff*W*H float4 (r,g,b,vertices) to host,
 * layout [(y*W+x)*spp + s].  Test/debug aid. */
int pine_gpu_plan_read_samples(pine_gpu_plan*, float* out_host, int64_t capacity_floats);

/* ---- Rendering in sample passes: a running film, bounded device memory, the same bits ----
 * A plan created WITH PASSES renders its film in n launches.  Pass j traces its share of the work, folds it into a running
 * per-pixel sum the plan owns (the reference's `L += ...` continued with the same roundings) and writes a viewable film;
 * after the last pass the film is bit for bit what pine_gpu_plan_launch of an ordinary plan writes.  The per-sample buffer
 * and the RNG checkpoints are sized for one pass, not for spp.
 *   - pixels whose samples are independent work items render the samples [j * P, min(spp, (j + 1) * P)) in pass j, P =
 *     pass_samples rounded down to a multiple of the plan's samples per item; their film value after pass j is
 *     (L_0 + ... + L_{m-1}) / m, m the samples so far, w = 1;
 *   - pixels that are one whole-pixel item (Subsurface tiles a camera ray can reach, fractional Uber, a SobolSampler /
 *     HaltonSampler count that is not a power of two) cannot be split by sample: their 8x8 tiles are dealt out in n slices,
 *     one slice per pass, all samples at once -- final once their slice has run, (0, 0, 0, 0) before.
 * n = ceil(spp / P); pass_samples <= 0 or >= spp: one pass, an ordinary plan.  An intermediate film is a PREVIEW, nothing
 * more: it is not the film of a render with fewer samples (BlueSampler's tables depend on the total spp).
 * Passes run in the order 0 .. n-1 (pass 0 starts the film afresh); any other order fails and launches nothing.
 * pine_gpu_plan_launch / _launch_packed of such a plan run all passes in order on the stream.  Plan stats after any pass:
 * vertices / shadow_rays / walk_steps are summed over the passes since pass 0, the three timings are per whole sequence
 * (from the last passes launched, at most 64); a bail-out of any pass fails them.  pine_gpu_plan_read_samples and the vertex log are
 * refused when n > 1 (the rows are gone by design). */
pine_gpu_plan* pine_gpu_plan_create_passes(pine_gpu_scene*, const pine_gpu_render_params*, int32_t pass_samples);
int pine_gpu_plan_pass_count(pine_gpu_plan*); /* 1 for an ordinary plan */
/* out = first sample, samples (the independent class's window of the pass), first whole-pixel tile, tiles (the pass's slice:
 * positions in the plan's order of whole-pixel tiles -- the tile classes' order, else the shard's natural tile order) */
int pine_gpu_plan_pass_info(pine_gpu_plan*, int pass, int32_t out[4]);
int pine_gpu_plan_launch_pass(pine_gpu_plan*, int pass, void* film_dev, void* stream);
/* The plan's tile order: the film tile (row-major index of the 8x8 tile) of every local tile, whole-pixel tiles of a plan
 * with tile classes first -- the order pass_info's tile numbers refer to.  Returns the number of local tiles. */
int pine_gpu_plan_tile_order(pine_gpu_plan*, int32_t* out, int cap);
/* bytes asked of the device for: per-sample rows | RNG checkpoints | running sum + carried RNG states | all buffers of the plan */
int pine_gpu_plan_device_bytes(pine_gpu_plan*, int64_t out[4]);
/* The planner itself, on the host (no GPU): the passes of one shard of a film_w x film_h film whose independent items are
 * samples_per_item samples (== spp: every pixel is one whole-pixel item) and `serial_tiles` of whose tiles are whole-pixel
 * tiles of a plan with tile classes.  Writes four numbers per pass as pine_gpu_plan_pass_info does, as many passes as fit
 * `cap` int32; returns the number of passes, < 0 on a bad argument. */
int pine_gpu_pass_schedule(int film_w, int film_h, int shard_rank, int shard_world, int spp, int samples_per_item, int serial_tiles,
                           int pass_samples, int32_t* out, int cap);
/* One-shot form with a running film: after every pass the host film is downloaded into film_out_host and `cb` (may be
 * NULL) is called with it; a non-zero return stops the render: the function returns PINE_GPU_RENDER_STOPPED and
 * film_out_host holds the last film delivered.  pine_gpu_progress() counts over the whole sequence. */
#define PINE_GPU_RENDER_STOPPED 1
typedef int (*pine_gpu_pass_callback)(void* user, int pass, int pass_count, const float* film_host);
int pine_gpu_path_render_passes(pine_gpu_scene*, const pine_gpu_render_params*, int32_t pass_samples, float* film_out_host,
                                pine_gpu_pass_callback cb, void* user);

/* ---- AOIntegrator ---------------------------------------------------------------------------
 * AOIntegrator(Accel, Sampler) + render(Scene&): src/pine/impl/integrator/ao.h, ao.cpp, RayIntegrator::render
 * (src/pine/core/integrator.cpp:83-100), registered program_context.cpp:58-61.  Ambient occlusion: per camera sample one closest-hit
 * ray and, where it hits, eight any-hit rays of length radius = min_value(scene.get_aabb().diagonal()) / 2 around one random frame;
 * the sample is the fraction of them that met nothing.  Materials, lights and emissive shapes play no part.  The integrator renders
 * max(sampler.spp() / 8, 1) samples per pixel (the sampler keeps its own count: tables, index stride); the film is the reference's
 * bit for bit with Accel = BVH() -- AOIntegrator(BVH(), sampler).  EmbreeAccel answers the eight rays with Embree's PACKET traversal
 * (rtcOccluded8), which nothing here restates: PINE_GPU_FLAG_ORDER_EMBREE is refused.
 * prm: spp / sampler / device / shard_rank / shard_world / PINE_GPU_FLAG_TIMING as for PathIntegrator; max_path_length and
 * samples_per_item are ignored; PINE_GPU_FLAG_FAST, _ORDER_EMBREE, _VERTEX_LOG and _SPECIALIZE are refused.
 * An AO plan works with pine_gpu_plan_launch (pixels outside the shard are zeros), _stats_get (camera_samples; spp_effective = the
 * AO count; vertices = primary hits; shadow_rays = any-hit queries = 8 x vertices; trace_ms, grid_blocks, block_threads, lds_bytes),
 * _check and _destroy; the packed launch, the vertex log and read_samples fail with a message.  Two schedules of the same arithmetic
 * give the same film: $PINE_GPU_AO_KERNEL=serial (the default: lane = sample, a loop over its eight rays) and =regroup (the wave's
 * hit points compacted, eight records x eight rays per trip); DESIGN.md 4.11 has the measurements behind the default. */
int pine_gpu_ao_render(pine_gpu_scene*, const pine_gpu_render_params*, float* film_out_host);
pine_gpu_plan* pine_gpu_ao_plan_create(pine_gpu_scene*, const pine_gpu_render_params*);
/* radius, then directions[8] (ao.cpp:6-9) as xyz: host only, no GPU */
int pine_gpu_ao_constants(pine_gpu_scene*, float out[25]);

/* ---- DenoiseIntegrator: guide images and the filter ------------------------------------------
 * DenoiseIntegrator(Accel, Sampler, LightSampler) + render(Scene&): src/pine/impl/integrator/denoiser.cpp, which computes two guide
 * images and hands them with the film the camera holds to denoise() (src/pine/core/denoise.h) -- Open Image Denoise in the reference,
 * a library for x86 hosts; DESIGN.md 4.12 has what stands in its place here.
 *
 * The guide images (denoiser.cpp:13-23): per pixel the albedo and the normal of the closest hit through the pixel centre --
 * camera.gen_ray((p + 0.5) / film_size, (0.5, 0.5)), material.albedo (an Emissive's colour, every other material's albedo node at
 * the surface's p, n, uv) and the interaction's n, not turned towards the camera; zeros on a miss.  out: W*H*3 floats each, film row
 * order, bit for bit the reference's with Accel = BVH().  prm: device and PINE_GPU_FLAG_DEVICE_BVH are read; spp, max_path_length
 * and sampler are not (the pass draws nothing).  Refused with a message: PINE_GPU_FLAG_ORDER_EMBREE, _FAST, _SPECIALIZE and
 * _VERTEX_LOG, a sharded film (shard_world != 1).  $PINE_GPU_GUIDES_VARIANT=<index> considers that kernel variant only (tests).
 * _device: albedo_dev / normal_dev are DEVICE pointers to W*H*3 floats; the launch is on `stream`, which has been synchronised when
 * the call returns (the scene's records on the device live for the length of the call). */
int pine_gpu_guides_render(pine_gpu_scene*, const pine_gpu_render_params*, float* albedo_out_host, float* normal_out_host);
int pine_gpu_guides_render_device(pine_gpu_scene*, const pine_gpu_render_params*, void* albedo_dev, void* normal_dev, void* stream);
/* The precompiled guide kernels in the order of the host's first-fit search: up to `cap` feature words (F_* bits); returns their
 * number.  Needs no GPU. */
int pine_gpu_guides_variants(uint32_t* features, int cap);

/* ---- Accel: batched ray queries ----------------------------------------------------------------
 * Accel::build(scene), intersect(ray, it), hit(ray): src/pine/core/accel.h:10-25, as RTIntegrator::intersect / hit hand them on
 * (src/pine/core/integrator.h:31-38) and CustomRayIntegrator exposes them to a user's radiance() (integrator.h:61-74,
 * src/pine/core/interpreter.cpp:46-53).  Here a query is a batch: n rays in, n answers out, in device memory on the caller's stream
 * or in host memory.  The traversal and the surface point are the path kernels' own: the answers are the reference's bit for bit,
 * with Accel = BVH() (src/pine/impl/accel/bvh.cpp:497-548) or -- PINE_GPU_FLAG_ORDER_EMBREE -- EmbreeAccel()
 * (src/pine/impl/accel/embree.cpp:144-165, :195-256).
 *
 * One ray is 8 floats: o[3], d[3], tmin, tmax (Ray, src/pine/core/ray.h:8-23).  The direction is used as given: it is not
 * normalised and t is in units of d; tmin is honoured.  One hit record is 12 words (48 bytes):
 *   0      f32  ray.tmax after the query        (miss: the tmax that came in, as the reference leaves it)
 *   1      i32  geometry index, in add order    (miss: -1)
 *   2      i32  triangle index within its mesh, -1 for every other shape (miss: -1)
 *   3      i32  material index                  (miss: -1)
 *   4-6    f32  it.p                            (miss: 0)
 *   7-9    f32  it.n as the interaction carries it: not turned towards the ray, interpolated where the mesh has normals (miss: 0)
 *   10-11  f32  it.uv                           (miss: 0)
 * A ray with a non-finite word or a zero direction is answered without a fault; what the answer is, is unspecified.
 * Everything else is the reference's answer, odd or not (the _edge.npz files of tests/golden hold it for tmin > 0, scaled and axis-parallel
 * directions with signed zeros, origins on a surface and spans that end exactly at a hit).  In particular:
 *   - the ends of [tmin, tmax] belong to the span or not shape by shape, and differently in intersect and hit: Plane and Sphere
 *     accept t == tmin and t == tmax in intersect and refuse both in hit; a Disk's intersect accepts both, its hit t == tmin only;
 *     a Triangle's (and a mesh's under pine's BVH) intersect refuses both and its hit accepts both; Rect refuses both in both;
 *     Cylinder, Cone, Line, Box and the transformed Box decide alike in both;
 *   - the reported t can lie outside the span: a transformed Box reports the box's far t where the near one is not above tmin, in
 *     units of the NORMALISED direction while tmin / tmax stay in units of d; a Cylinder's second root is not compared with tmin;
 *     a Sphere's t ignores the length of d.  A scaled direction therefore hits such shapes where the reference does, not where
 *     geometry would;
 *   - a ray that lies in a Plane, or runs along a Cylinder's axis, divides 0 by 0: it "hits" with t = NaN, and no box of the
 *     hierarchy is entered after that.
 * Unspecified under PINE_GPU_FLAG_ORDER_EMBREE: a negative tmin.  Embree requires tnear >= 0, clamps it to 0 for its node boxes
 * and not in its triangle test, so a hit behind the origin depends on which leaves its own hierarchy reaches.
 *
 * pine_gpu_accel_create (Accel::build, bvh.cpp:453-495): builds the scene's BVH if nobody has yet, uploads the scene's records to
 * `device` and keeps them: a snapshot -- a geometry added to the scene later is not in an existing accel.  flags: 0 (pine's BVH
 * order) or PINE_GPU_FLAG_ORDER_EMBREE (a hierarchy deeper than the per-ray stack of 192 entries fails here, as for plans);
 * PINE_GPU_FLAG_FAST, _SPECIALIZE and _VERTEX_LOG are refused with a message, as is any other bit.  A scene no precompiled kernel
 * variant covers is refused by name.  The scene needs no camera (only pine_gpu_accel_camera_rays_device does).  Fails if there is
 * no GPU.  $PINE_GPU_ACCEL_VARIANT=<index> considers that kernel variant only (tests).
 * An accel holds no mutable device state: queries on different streams, and from different threads, may run at once.
 * pine_gpu_accel_destroy waits for the device when a query was ever launched, then gives the records back. */
typedef struct pine_gpu_accel pine_gpu_accel;
pine_gpu_accel* pine_gpu_accel_create(pine_gpu_scene*, int device, uint32_t flags);
void pine_gpu_accel_destroy(pine_gpu_accel*);
/* Accel::intersect (accel.h:22-24; bvh.cpp:513-548) for n rays: rays_dev -> n * 8 floats, hits_dev -> n * 12 words, DEVICE pointers,
 * both 16-byte aligned (else the call fails; a row slice of either buffer keeps the alignment).  The two buffers must not overlap
 * (not checked).  The launch is enqueued on `stream` (a hipStream_t, 0 = the default stream) and the call returns without
 * synchronising.  n == 0: returns 0, nothing is launched; n < 0 or n > 2^31 - 1 fails.  Words behind the n-th record are not written. */
int pine_gpu_accel_intersect_device(pine_gpu_accel*, const void* rays_dev, int64_t n, void* hits_dev, void* stream);
/* Accel::hit (accel.h:16-18; bvh.cpp:497-511, embree.cpp:144-165) for n rays: occluded_dev -> n bytes, 1 where a shape's hit() finds
 * something in the span, else 0 -- the ends count as each shape's hit() decides, which is not always as its intersect() does (above).  rays_dev must be 16-byte aligned; the bytes need no alignment.  Otherwise as above. */
int pine_gpu_accel_hit_device(pine_gpu_accel*, const void* rays_dev, int64_t n, void* occluded_dev, void* stream);
/* ... on HOST arrays: upload, launch, wait, download. */
int pine_gpu_accel_intersect(pine_gpu_accel*, const float* rays_host, int64_t n, void* hits_host);
int pine_gpu_accel_hit(pine_gpu_accel*, const float* rays_host, int64_t n, uint8_t* occluded_host);
/* The rays of DenoiseIntegrator's guide images (src/pine/impl/integrator/denoiser.cpp:13-23): camera.gen_ray((p + 0.5) / film_size,
 * (0.5, 0.5)) (src/pine/core/camera.cpp:17-33) for every pixel of the film the scene's camera had at creation, row-major, tmin = 0,
 * tmax = FLT_MAX: W * H * 8 floats to the 16-byte aligned DEVICE pointer rays_dev, enqueued on `stream`. */
int pine_gpu_accel_camera_rays_device(pine_gpu_accel*, void* rays_dev, void* stream);
/* out: the chosen kernel variant's feature word (F_* bits), its dynamic LDS bytes per workgroup, the film's W and H (0 0: the scene
 * had no camera).  Needs no GPU call. */
int pine_gpu_accel_info(pine_gpu_accel*, int32_t out[4]);

/* ---- Shader: batched path-vertex shading queries on device buffers ----
 * One vertex of PathIntegrator::radiance() (src/pine/impl/integrator/path.cpp:42-123, without the medium lines) for n paths that
 * live in the CALLER's device buffers -- what a CustomRayIntegrator's radiance() gets besides the ray queries: the scene's
 * materials, the light sampler and the sampler (core/integrator.h:27-74).  With an accel,
 *   begin -> intersect -> vertex -> hit(shadow rays) -> intersect(next rays) -> vertex -> ... -> fold -> resolve
 * is a complete path tracer whose every ray, hit and vertex record the caller sees; run over all paths at every level it gives
 * PathIntegrator's film bit for bit (an accel of either order: the shader shades whatever hits it is given).
 *
 * A ray is Accel's: 8 floats, o[3] d[3] tmin tmax.  The null ray -- where a vertex has no shadow or next ray -- is o = 0,
 * d = (0, 0, 1), tmin = 0, tmax = -1: finite, answered at once, its answer never read.
 * A path state is 8 words (32 bytes):
 *   0-3  the pixel's RNG (two u64)          4  sample index (bits 0-11) | Vertex::length (21-26) | diffuse_length > 0 (27) | is_delta (28)
 *   5    px | py << 16                      6  the sampler's dimension counter (i32)         7  0: live, 1: done
 * A vertex record is 16 words (64 bytes):
 *   0     i32  kind: -1 none (the path was done before), 0 the ray left the scene, 1 it met an emissive surface, 2 the path-length
 *              limit, 3 a shaded vertex
 *   1     i32  Vertex::length                2  u32  flags: 1 has_shadow_ray, 2 has_next_ray, 4 the light pdf is there
 *   3     f32  kinds 0, 1: the pdf of having picked the vertex by light sampling, -1: none
 *   4-6   f32  kinds 0, 1: the returned Lo   7  f32  cosine
 *   8-10  f32  kind 3: the direct term, UNSHADOWED             11  f32  bs.pdf
 *   12-14 f32  bs.f                          15 f32  bs.is_delta (0 or 1)
 * The log of pine_gpu_shader_fold_device is 16 floats per vertex, the words of pine_gpu_plan_vertex_log:
 *   kind | length | direct term after visibility (3) | bs.f (3) | cosine | bs.pdf | is_delta | mis | light pdf (-1: none) | Lo (3)
 *
 * pine_gpu_shader_create reads spp, sampler, max_path_length and device of the parameters; the effective spp follows the plan's
 * rules (BlueSampler: rounded up to a power of two, at most 256; SobolSampler / HaltonSampler: as given, at most 4096).  It
 * uploads the scene's records -- a snapshot -- and keeps them.  Refused with a message, nothing approximated: a scene with a
 * Subsurface material (by name: its BSSRDF walk traverses inside the vertex), any flag bit (PINE_GPU_FLAG_ORDER_EMBREE too: the
 * order is the Accel's business), shard_world != 1, a scene no kernel variant covers, a machine without a GPU.  The scene needs
 * no camera (only pine_gpu_shader_begin_device does).  $PINE_GPU_SHADER_VARIANT=<index> considers that kernel variant only (tests).
 * A shader holds no mutable device state: calls on different streams may run at once.  pine_gpu_shader_destroy waits for the
 * device when anything was ever launched.
 *
 * Every _device call enqueues on `stream` (a hipStream_t, 0 = the default stream) and returns without synchronising.  Every
 * buffer is a 16-byte aligned DEVICE pointer (the occlusion bytes need no alignment).  n == 0 returns 0 and launches nothing;
 * n < 0 or n > 2^31 - 1 fails.  Every word of every output of the n paths is written; nothing behind them is. */
typedef struct pine_gpu_shader pine_gpu_shader;
pine_gpu_shader* pine_gpu_shader_create(pine_gpu_scene*, const pine_gpu_render_params*);
void pine_gpu_shader_destroy(pine_gpu_shader*);
/* out: bytes of a path state, bytes of a vertex record, floats of a ray, floats of a log entry.  Needs no GPU. */
int pine_gpu_shader_layout(int32_t out[4]);
/* out: the film's W and H (0 0: no camera), the effective spp, max_path_length, the chosen kernel variant's index, its feature
 * word (F_* bits), its dynamic LDS bytes per workgroup, the sampler kind.  Needs no GPU call. */
int pine_gpu_shader_info(pine_gpu_shader*, int32_t out[8]);
/* Sample `sample` (in [0, spp)) of every pixel of the film starts: W * H paths in row order.  Sample 0 seeds the pixel's RNG as
 * Sampler::start_pixel does; a later sample goes on from the RNG the state holds, as left by sample - 1 -- the RNG is serial over a
 * pixel's samples, so a caller renders them in order.  Writes every state (live, Vertex::first_vertex()) and the camera rays. */
int pine_gpu_shader_begin_device(pine_gpu_shader*, int sample, void* states_dev, void* rays_dev, void* stream);
/* One radiance() invocation per path: rays_dev[i] is the ray that led to the vertex, hits_dev[i] Accel's 12-word answer for it.
 * Writes the record, the shadow ray and the next ray of every path and advances its state.  A path whose state says done gets a
 * "none" record and null rays and keeps its state byte for byte: all n paths may be launched at every level. */
int pine_gpu_shader_vertex_device(pine_gpu_shader*, const void* rays_dev, const void* hits_dev, int64_t n, void* states_dev, void* records_dev,
                                  void* shadow_rays_dev, void* next_rays_dev, void* stream);
/* The backward fold of one sample (path.cpp:114-121): records_dev is levels x n records, occluded_dev levels x n bytes (what
 * Accel's hit answered for the shadow rays; read only where a record has one), level-major, 1 <= levels <= max_path_length.
 * sum_dev: n float4 -- path i adds its radiance to xyz (the running sum in sample order; sample 0 overwrites), w is the sample
 * count.  log_dev_or_null: levels x n x 16 floats, zeros past a path's end. */
int pine_gpu_shader_fold_device(pine_gpu_shader*, const void* records_dev, const void* occluded_dev, int levels, int64_t n, int sample, void* sum_dev,
                                void* log_dev_or_null, void* stream);
/* film_dev[i] = (sum_dev[i].xyz / spp, 1), the division of PathIntegrator's film. */
int pine_gpu_shader_resolve_device(pine_gpu_shader*, const void* sum_dev, int64_t n, void* film_dev, void* stream);

/* The filter: an a-trous edge-avoiding wavelet filter (Dammertz et al. 2010) on albedo-demodulated colour; the definition is in
 * pine_amd/csrc/pine_denoise.h and DESIGN.md 4.12.  film / out: W*H float4 (rgb filtered, a kept); albedo / normal: W*H*3 floats,
 * the guide images above.  A pixel whose normal is (0, 0, 0) -- a miss -- is copied through and contributes to no other pixel.
 * iterations 0 ... 8 (0: the identity), step 2^i in iteration i; normal_power_log2 k: the normal weight is max(0, n.n')^(2^k).
 * device >= 0: the gfx950 kernels on that device; device = -1 (pine_gpu_denoise only): the host-thread build of the same
 * functions (at most min(16, $OMP_NUM_THREADS, hardware threads)) -- the same bytes either way. */
typedef struct {
  int32_t iterations;         /* 5 */
  int32_t normal_power_log2;  /* 7: the power 128 */
  float sigma_color;          /* of the demodulated colour in iteration 0; halved with every iteration */
  float sigma_albedo;
  float eps_albedo;           /* demodulation divides by max(albedo, eps_albedo) per component */
  int32_t device;
} pine_gpu_denoise_params;
/* The defaults: of a sweep on four scenes the cell with the best mean error ratio among those where the filtered 16 spp film of
 * EVERY scene is closer to its 4096 spp film than the unfiltered one (profiles/denoise_quality.txt).  That criterion is ruled by
 * the few pixels that hold a sliver of a lamp, which only a small sigma_color leaves alone: the default is cautious, and
 * sigma_color = 0.25 smooths the rest of a picture far more (same file). */
#define PINE_GPU_DENOISE_SIGMA_COLOR 0.05f
#define PINE_GPU_DENOISE_SIGMA_ALBEDO 0.3f
#define PINE_GPU_DENOISE_EPS_ALBEDO 0.001f
void pine_gpu_denoise_params_default(pine_gpu_denoise_params*);
int pine_gpu_denoise(const pine_gpu_denoise_params*, int w, int h, const float* film_rgba_host, const float* albedo_host, const float* normal_host,
                     float* out_rgba_host);
/* ... on device memory, launched on `stream` (a hipStream_t, 0 = the default stream); out_dev may equal film_dev.  The stream has
 * been synchronised when the call returns: the work buffers come from the memory pool and go back to it. */
int pine_gpu_denoise_device(const pine_gpu_denoise_params*, int w, int h, const void* film_dev, const void* albedo_dev, const void* normal_dev,
                            void* out_dev, void* stream);

/* Host test hook: the reference's partition (src/psl/algorithm.h:394-402) as its sequential swap loop and as the data-parallel
 * formulation of the device BVH build; both permutations out, < 0 if they disagree. */
int pine_gpu_test_lomuto(const unsigned char* pred, int n, int* perm_sequential, int* perm_parallel);

/* Device-side unit-test hooks: run the device implementations on arrays (parity vs oracle). */
int pine_gpu_test_sampler(int device, int spp, float* out_host, int64_t capacity);  /* layout of oracle_sampler_stream */
int pine_gpu_test_rng(int device, uint64_t* out_host, int64_t capacity);            /* layout of oracle_rng_stream */
/* The sampler front of the kernels, sampler_get1d / sampler_get2d, call by call: BlueSampler (kind 0), SobolSampler (1) or
 * HaltonSampler (2) of `spp` samples on a w x h film, its tables built and uploaded by the code that builds a plan's.  n cases of 9
 * int32 -- kind, spp, w, h (the call's own), px, py, sample index, pattern, calls -- one thread each: the sampler of that pixel
 * and sample as the path kernels start it (dimension 0, HaltonSampler's 2), then `calls` calls of the pattern (0: get2d  1: get1d,
 * get2d alternating  2: get1d).  out_host: every float, case after case (oracle_sampler_draws has the layout); returns their
 * number.  mode 0: the tables read from memory; mode 1: the workgroup's LDS cache of a 256-thread kernel (stage_sobol_rows,
 * load_lane_slice, lane_tables), as the megakernel and the AO kernel read them.  device = -1: the host build of the same functions
 * (mode 0 only).  Refused without a launch: spp <= 0 or above 4096, a film side above 65535, a pixel outside the film, a sample
 * index outside the pixel's, more than 65536 cases or calls, too small a capacity. */
int64_t pine_gpu_test_sampler_draws(int device, int kind, int spp, int w, int h, int mode, const int32_t* cases_host, int64_t n,
                                    float* out_host, int64_t capacity);
/* Host test hook: CRC-32 and element counts of HaltonSampler's tables as the library derives them -- the primes, their prefix sums
 * (int32 each), the digit permutations (uint16). */
int pine_gpu_test_halton_tables(uint32_t crc32[3], int64_t counts[3]);
int pine_gpu_test_sincos(int device, const float* x_host, int64_t n, float* sin_out, float* cos_out);
int pine_gpu_test_powlog(int device, const float* x_host, const float* y_host, int64_t n, float* pow_out,
                         float* log_out);                                           /* powf(x, y), logf(x) */
int pine_gpu_test_atan(int device, const float* y_host, const float* x_host, int64_t n, float* atan2_out,
                       float* acos_out);                                            /* atan2f(y, x), acosf(x) */
/* Scalar math of pine_math.h / pine_libm.h over bit patterns, for the sweeps of tests/test_device_math.py.  fn names the
 * function f(a[, b[, c]]) and the reference it must equal bit for bit:
 *   SQRT psqrt(a) / RCP prcp(a) / DIV a / b      host IEEE sqrtf, 1.0f / a, a / b (correctly rounded)
 *   SIN COS LOG ACOS EXP psin pcos plog pacos pexp (a)   glibc sinf cosf logf acosf expf
 *   SINCOS psincos(a): two results (sin, cos)     glibc sinf, cosf
 *   ATAN2 patan2(a, b) / POW ppow(a, b)           glibc atan2f, powf
 *   MIN pmin(a, b) / MAX pmax(a, b) / CLAMP pclamp(a, b, c)   the same comparison expressions on the host
 * Comparison: bits equal, +0 != -0; two NaNs are equal (a payload or sign difference is counted in nan_payload_only);
 * NaN against a number is a mismatch.  stats[4] = checked results, mismatches, nan_payload_only, largest ulp distance of a
 * mismatch between two non-NaN results (-0 and +0 are 1 apart).  examples[cap][5] = a, b, c, got, want of the first cap
 * mismatches in input order (SINCOS: b = 0 for the sine result, 1 for the cosine one).  Host threads: at most
 * min(16, $OMP_NUM_THREADS, hardware threads).  All return 0, < 0 on error. */
enum {
  PINE_GPU_MATH_SQRT = 0,
  PINE_GPU_MATH_RCP = 1,
  PINE_GPU_MATH_SIN = 2,
  PINE_GPU_MATH_COS = 3,
  PINE_GPU_MATH_SINCOS = 4,
  PINE_GPU_MATH_LOG = 5,
  PINE_GPU_MATH_ACOS = 6,
  PINE_GPU_MATH_ATAN2 = 7,
  PINE_GPU_MATH_POW = 8,
  PINE_GPU_MATH_DIV = 9,
  PINE_GPU_MATH_MIN = 10,
  PINE_GPU_MATH_MAX = 11,
  PINE_GPU_MATH_CLAMP = 12,
  PINE_GPU_MATH_EXP = 13,
  PINE_GPU_MATH_COUNT = 14
};
/* got[i] = fn(a[i], b[i], c[i]) (SINCOS: got[2i], got[2i+1]) by the device build on HIP device `device`, or by the host
 * build of the same functions for device = -1.  b and c may be NULL when fn does not read them. */
int pine_gpu_test_math_eval(int device, int fn, const uint32_t* a, const uint32_t* b, const uint32_t* c, int64_t n,
                            uint32_t* got);
/* Host only: compares got (layout of pine_gpu_test_math_eval) with the reference. */
int pine_gpu_test_math_compare(int fn, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* got,
                               int64_t n, int64_t* stats, uint32_t* examples, int cap);
/* Evaluates and compares in chunks of 2^26: argument `swept_arg` (0 = a, 1 = b, 2 = c) runs over first + k * stride
 * (mod 2^32) for k < count, every other argument is fixed_bits; the inputs are generated where fn is evaluated. */
int pine_gpu_test_math_sweep(int device, int fn, uint32_t fixed_bits, int swept_arg, uint32_t first, uint64_t count,
                             uint32_t stride, int64_t* stats, uint32_t* examples, int cap);
/* BVH traversal (bvh.cpp:321-451, 497-548) of the scene's accel for each ray (8 floats: o, d, tmin, tmax), by the nested
 * loops of the scene-in-LDS kernel variants (flat = 0) or the flat state machine of the others (flat = 1).  Per ray
 * 2 * cap + 5 words: [count, count test words ...] (cap words), hit, geometry, triangle, tmax bits of the closest-hit query,
 * then [count, words ...] (cap words) and hit of the any-hit query.  A test word is a top-level primitive's geometry index
 * or 0x40000000 | triangle index within the mesh entered last: the layout of `pine_ref bvh` (tests/golden/bvh_*.npz). */
int pine_gpu_test_traverse(pine_gpu_scene*, int device, const float* rays_host, int64_t nrays, int flat, int cap, uint32_t* out_host);
/* (flat = 2: the closest-hit query in EmbreeAccel's order, PINE_GPU_FLAG_ORDER_EMBREE: the geometry indices handed to their tests)
 * ... and the hierarchy of that order over n boxes (6 floats each), HOST code only: the root's child word, then 8 child words per
 * node in creation order (>= 0 a node, < 0 the complement of a box index, INT32_MIN unused).  -> words written, < 0 on failure. */
int pine_gpu_test_embree_tree(const float* boxes, int n, int* words, int cap);
/* ... and the BAKED traversal of a plan created with PINE_GPU_FLAG_SPECIALIZE (plan stats: specialized == 2) on the same kind of
 * rays: per ray 4 words -- hit, geometry, tmax bits of the closest-hit query, result of the any-hit query.  Must equal the
 * corresponding words of pine_gpu_test_traverse for every finite ray (tests/test_specialize.py: axis-parallel and grazing rays,
 * origins on the walls, zero direction components). */
int pine_gpu_plan_test_traverse_baked(pine_gpu_plan*, const float* rays_host, int64_t nrays, uint32_t* out_host);
/* The scene's BVHs after pine_gpu_scene_build_accel: per BVH (top level first, then one per mesh in geometry order) 5 words:
 * root, root_start, root_count, prim_base (DBvh) and the geometry index of its mesh (-1 for the top level).  Returns their
 * number, or < 0.  With pine_gpu_scene_accel_dump this is the whole tree (tests compare it with the reference's own). */
int pine_gpu_scene_accel_bvhs(pine_gpu_scene*, int32_t* out, int64_t capacity_words);
int pine_gpu_test_shapes(pine_gpu_scene*, int device, const float* rays_host, int64_t nrays,
                         float* out_host, int64_t capacity);                        /* layout of oracle_shapes */
/* The BSDF lobes one call at a time (pine_device.h bxdf_f / bxdf_pdf / bxdf_is_delta / bxdf_sample), for tests/test_sampling_fixtures.py.
 * One case = 16 floats (integers as exactly representable floats): 0 lobe (BxdfKind order: Diffuse, Conductor, Refractive,
 * RefractiveDielectric, DiffusiveDielectric, BSSRDF)  1-3 albedo  4 roughness  5 ior  6-8 wi  9-11 wo (local frame)  12 13 sampler
 * pixel (< 1024)  14 sample index (< 64)  15 calls: bit 0 = f and pdf, bit 1 = sample.  One record = 14 floats: 0-2 f  3 pdf
 * 4 is_delta  5 sample returned a value  6-8 its wo  9-11 its f  12 its pdf  13 its is_delta; what was not computed is 0.
 * sample draws from SobolSampler(64) on a 1024 x 1024 image, at that pixel and sample index.  out_host: 2 * n records -- n by the
 * code built with every feature (F_ALL), then n by the code built with the narrowest feature mask that contains the case's lobe
 * (none, F_UBER or F_SSS), as the shipped kernel variants are.  device = -1: the host build of the same functions. */
int pine_gpu_test_bxdf(int device, const float* cases_host, int64_t n, float* out_host);
/* shape_sample + shape_pdf of every geometry and light_sample_other of every light that is no area light (scene order, the
 * environment light last) for n queries of 6 floats (o, u2, u1).  out_host: per (geometry, query) 13 floats -- 0 sampled (-1: a
 * Cylinder, which the reference cannot sample)  1-3 p  4-6 n  7-9 w  10 distance  11 pdf  12 shape_pdf of the ray o -> w with
 * tmax = distance and that n -- then per (light, query) 9 floats: 0 sampled  1-3 w  4 distance  5 pdf  6-8 le.  Zeros after
 * a 0 or -1.  device = -1: the host build of the same functions. */
int pine_gpu_test_light_samples(pine_gpu_scene*, int device, const float* queries_host, int64_t n, float* out_host);
/* The scene's ImageSky or Atmosphere one call at a time (pine_device.h image_sky_sample / _color / _pdf, atmosphere_sample /
 * atmosphere_sky_color), for tests/test_envsky.py and tests/test_atmosphere.py.  A query is
 * 5 floats: u2, then a direction wo.  A record is 13 floats: 0 1 the texel sample(u2) chose (ds.p, as exactly representable
 * floats)  2 its pdf  3-5 its wo  6-8 its le  9-11 color(wo of the query)  12 pdf(wo of the query).  device = -1: the host build
 * of the same functions.  An ImageSky is not part of pine_gpu_test_light_samples' records (it reports "not sampled"). */
int pine_gpu_test_env_light(pine_gpu_scene*, int device, const float* queries_host, int64_t n, float* out_host);
/* The ImageSky's or Atmosphere's density tree (the reference's Distribution2D) in pre-order, rebuilt from the flat device layout: per node 7
 * words -- weight (float bits), split_x, lower.x, lower.y, upper.x, upper.y, leaf.  Returns the number of words (they are
 * written when out is not NULL and capacity_words suffices), < 0 on error.  Needs no GPU. */
int64_t pine_gpu_test_env_tree(pine_gpu_scene*, int32_t* out, int64_t capacity_words);
/* The environment light as the light sampler calls it: light_sample_other (pine_device.h) with the light's buffer.  A query is 5
 * floats, p then u2; a record the 9 floats of pine_gpu_test_light_samples: 0 sampled  1-3 w  4 distance  5 pdf  6-8 le.  For an
 * ImageSky or an Atmosphere; device = -1: the host build. */
int pine_gpu_test_env_light_sample(pine_gpu_scene*, int device, const float* queries_host, int64_t n, float* out_host);
/* atmosphere_color(direction, sun_dir, 8, flag) (pine_atmosphere.h) one call at a time: a query is 7 floats -- direction, sun
 * direction (taken as given), flag (non-zero: with the sun disc) -- and gives 3.  device = -1: the host build. */
int pine_gpu_test_atmosphere_color(int device, const float* queries_host, int64_t n, float* out_host);
/* The tables of the scene's Atmosphere: w * h densities, then (w + 1) * (h + 1) colours of 3 floats (row by row; row h and column
 * w are the grid points a sample can reach when a rescaled u rounds to 1).  The colours are the light's own; the densities,
 * which the scene does not keep, are computed again where the light's were.  Returns the number of floats (they are written when
 * out is not NULL and capacity suffices), < 0 on error. */
int64_t pine_gpu_test_env_table(pine_gpu_scene*, float* out, int64_t capacity);
/* The shading-node programs of the scene's materials, as plan creation compiles them (needs no GPU): num_materials, num_ops,
 * then per material prog[4] (index of the first op of the program of albedo, roughness, metallic, transmission / ior; -1: the
 * parameter is a literal of the record), then per op 4 words: opcode, x, y, z (float bits).  Returns the number of words (they
 * are written when out is not NULL and capacity_words suffices), or < 0: a node tree needs more than the evaluator's stack. */
int64_t pine_gpu_test_node_programs(pine_gpu_scene*, int32_t* out, int64_t capacity_words);
/* ... and the size in 4-byte words of the image buffer a plan of the scene would upload for them: 0 where no program reads
 * an image, else the 256-word 8-bit table and every image a program names, once (tests/test_texture.py). */
int64_t pine_gpu_test_tex_words(pine_gpu_scene*);
/* The material-to-parameters step, for tests/test_node_fixtures.py: compiles the node programs, then material_params of every
 * material (scene order) at n queries of 8 floats (p, n, uv).  out_host: per (material, query) 10 floats -- 0-2 albedo
 * 3-5 albedo / Pi  6 roughness  7 metallic  8 transmission  9 ior.  device = -1: the host build of the same functions. */
int pine_gpu_test_material_params(pine_gpu_scene*, int device, const float* queries_host, int64_t n, float* out_host);
/* ... and the parameters-to-lobe step, choose_lobe (device code only: device >= 0).  One case = 16 floats (integers as exactly
 * representable floats): 0 material index (no Emissive)  1-3 p  4-6 n  7 8 uv  9-11 wi (world)  12 diffused  13 14 sampler
 * pixel (< 1024)  15 sample index (< 64).  The sampler is SobolSampler(64) on a 1024 x 1024 image at that pixel and sample,
 * the pixel's RNG is seeded as a render seeds it for that pixel.  out_host: 2 * n records of 8 floats -- n with after_walk = 0
 * (Material::sample_bxdf of the reference), then n with after_walk = 1 (the vertex resumes after its BSSRDF walk): 0 lobe
 * (BxdfKind order)  1-3 albedo  4 roughness  5 ior (0 where the lobe has no such member)  6 the sampler's dimension afterwards
 * 7 the next float of the pixel's RNG afterwards. */
int pine_gpu_test_choose_lobe(pine_gpu_scene*, int device, const float* cases_host, int64_t n, float* out_host);
/* The frame table: per face of every Rect (1), AABB and OBB (6: 2 * axis + 1 where the local normal points down
 * the axis), in geometry order, one entry of 12 floats -- n, t, b, each padded to four -- and per geometry base[g], its first
 * entry (-1: a kind without faces).  device = -1 (plan NULL): the scene's table as plan creation builds it, on the host.
 * device >= 0: the table of `plan`, a plan of this scene, copied back from the device; no entries where the plan has none.
 * generic (or NULL): per entry, in the same layout, what the per-hit code computes at a point of that face (host build of
 * shape_surface_info and coordinate_system).  faces (or NULL): for nrays rays of 8 floats (pine_gpu_test_shapes) and every
 * geometry that is no mesh, in that hook's record order, the face the host build reports at the hit; -1 without a hit or a face.
 * Returns the number of entries, < 0 on error. */
int64_t pine_gpu_test_frame_table(pine_gpu_scene*, pine_gpu_plan* plan, int device, float* entries, float* generic, int64_t cap_entries,
                                  int32_t* base, int64_t cap_shapes, const float* rays_host, int64_t nrays, int32_t* faces);
/* The slab test of the baked scenes' transformed boxes (box_slabs_lean, pine_device.h) beside the one every other caller runs
 * (box_slabs), both as the host compiles them.  n cases: boxes_host 6 floats each (lo, hi), rays_host 8 floats each (o, d, tmin,
 * tmax; the ray in the box's frame).  out_host: 6 words per case -- flag, tmin bits, tmax bits of box_slabs, then of the lean
 * routine (the bounds mean something on a hit only).  Needs no GPU. */
int pine_gpu_test_box_slabs(const float* boxes_host, const float* rays_host, int64_t n, uint32_t* out_host);
/* The baked traversal's short division and short normalisation (pine_math.h "division") beside the compiler's
 * own, bit by bit, on the device.  kind 0: per case a numerator and a denominator -- n / d against what a site of the traversal
 * computes (window test, quotient from the refined reciprocal, plain division outside the window).  kind 1: per case a vector of
 * three -- normalize() and prcp() of its components against local_direction_lean.  The cases: gen 0, n cases of 2 (3) words at
 * in_host; gen 1 (kind 0), the numerator p1 over the n denominators p0, p0 + 1, ...; gen 2, n pseudo-random cases from the seed
 * p0, every sign and mantissa, biased exponents p1 ... p2.  stats[4]: cases, mismatches, cases that took the short form, and of
 * those the ones with an operand outside the window (asked of the operand's bits).  examples: the first `cap` mismatches, 8
 * words each -- the operands (3), the index of the differing output, wanted, got, whether the short form was taken, 0. */
int pine_gpu_test_short_div(int device, int kind, int gen, const uint32_t* in_host, uint32_t p0, uint32_t p1, uint32_t p2, int64_t n,
                            int64_t stats[4], uint32_t* examples, int cap);
/* The precompiled path-kernel variants (pine_variants.h) in the order of the host's first-fit search: kind 0 the stage-queued
 * kernel, 1 the megakernel.  Up to `cap` entries of features (F_* bits), ctx (path contexts per workgroup; 0 for the
 * megakernel) and order; any of the arrays may be NULL.  Returns the number of variants, < 0 on error.  Needs no GPU.
 * With $PINE_GPU_TEST_VARIANT=queue:<order> / mega:<order> plan creation considers that variant only (tests/test_kernel_matrix.py). */
int pine_gpu_test_kernel_variants(int kind, uint32_t* features, int32_t* ctx, int32_t* order, int cap);
/* Who holds device resources right now.  out[0]: the handles the library's owners hold -- device blocks, pinned host memory,
 * events and streams of live plans and of calls in flight, all kinds counted together; a call that has returned, a plan that
 * has been destroyed or was never created holds none.  out[1]: the blocks the device memory pool keeps for the next plan
 * (pine_gpu_release_cached_memory frees them).  Reads two counters and launches nothing; returns 0. */
int pine_gpu_test_live_device_blocks(int64_t out[2]);
/* The poison mode of device memory, a test mode: with $PINE_GPU_TEST_POISON=<32-bit hex word> set -- read at every allocation --
 * every device block the library allocates (fresh or recycled by the pool, the pool's slack behind the requested bytes included)
 * and every pinned host block is filled with that word before anything else touches it, and the fill is complete on the device
 * before the allocation returns.  A value that is no 32-bit hex word (hex digits, an optional 0x) fails every allocation.  Unset,
 * nothing changes.  out[0]: the blocks poisoned by this process so far, out[1]: their
 * bytes.  Reads two counters and launches nothing; returns 0. */
int pine_gpu_test_poison_stats(int64_t out[2]);
/* One block of `bytes` bytes (> 0) on `device`, taken from the plans' memory pool (from_pool != 0) or from plain hipMalloc the way
 * every block of the library is, with nothing written to it: its first `bytes` bytes are copied to out_words ((bytes + 3) / 4
 * words).  Under $PINE_GPU_TEST_POISON they hold the word.  Launches nothing; 0, or -1 with the last error set. */
int pine_gpu_test_poison_probe(int device, int from_pool, int64_t bytes, uint32_t* out_words);

/* ---- Film (host side, after the hot path) ----------------------------------------------------
 * Film::finalize + tone mapping + to_uint8_array: src/pine/core/film.cpp:12-27,66-68,
 * src/pine/core/color.cpp:6-23, src/pine/core/fileio.cpp:42-54.  rgba_out: W*H*4 bytes, y-flipped. */
int pine_gpu_film_finalize_u8(const float* film_host, int w, int h, int tonemapper, uint8_t* rgba_out);

#ifdef __cplusplus
}
#endif
#endif /* PINE_GPU_H */
