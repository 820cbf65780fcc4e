/*
 * rt_abi.h — C-ABI drop-in boundary for the per-pixel Monte Carlo render loop.
 *
 * The reference (firelion9/raytracing-course-hw-public) has no plugin/FFI layer;
 * the one seam where the hot path is entered is the call
 *
 *     run_raytracer(const Scene &scene, Image &image)      src/main.cpp:37 -> src/raytracer.h:629
 *
 * Everything below replaces exactly that call (and what it owns: the two BVH
 * builds of raytracer.h:440-447 and the per-pixel sample loop of raytracer.h:618-627).
 * Plain pointers + sizes only; no C++ or torch types cross this boundary.
 *
 * Reference inputs consumed at the seam and their POD restatement here:
 *   scene.objects[i].shape      (geometry.h:458-503, 3 x vec3)      -> rt_scene_desc.positions  (9 floats / triangle)
 *   scene.objects[i].attrs      (geometry.h:633-637)                -> normals (9), texcoords (6), tangents (9)
 *   scene.objects[i].material   (geometry.h:604-613, one per Object)-> material_ids[i] into rt_material_desc[]
 *   material.*_tex pointers     (geometry.h:610-613)                -> texture indices, RT_TEX_NONE = built-in
 *                                                                      WHITE_TEXTURE / NORMAL_UP (geometry.h:601-602)
 *   Texture::data (color4 float = stb u8 / 255.0f, geometry.h:590-595) -> RGBA8 texels (the /255.0f and the per-lookup
 *                                                                      pow(c, 2.2f) of geometry.h:525-527 are done
 *                                                                      by bit-exact 256-entry tables)
 *   scene.camera                (scene.h:60-72)                     -> rt_camera
 *   scene.bg_color, scene.bg    (scene.h:75,81; main.cpp:28-31)     -> bg_color, bg_texture (RT_TEX_NONE = the 1x1 white default of
 *                                                                      USE_ENV_MAP=false, config.h:37; else the environment map)
 *   scene.ray_depth, samples    (scene.h:76-77)                     -> rt_scene_desc.ray_depth, rt_params.samples
 * Reference output at the seam:
 *   image.set_pixel(p_idx, render_pixel(...)) (raytracer.h:658) which tone-maps at once (image.h:40-42,79-82)
 *                                                                   -> linear float3 framebuffer; tone-map/quantise is a
 *                                                                      pure per-pixel host function applied afterwards
 *                                                                      (rt_tonemap_rgb8, restating image.h:49-82).
 * Errors: the reference throws std::runtime_error (caught in main.cpp:46-49). Nothing is thrown across this
 * ABI: every entry point returns RT_OK or an error code and rt_last_error() holds the message.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 4u /* 2: rt_scene_desc carries analytic primitives (scene-txt front end); 3: bg_texture (environment map);
                             4: every tuning knob is a field (rt_build_options, rt_params.sort_mode / packet_mode / max_paths ...): the library
                                reads no environment variable; progress callback; packet census in rt_stats. Still 4 after the development
                                options were retired (two rt_build_options fields became reserved, unused RT_SORT_* / RT_BUILD_* values are
                                refused): the binary layout and the meaning of every value that remains are unchanged. Still 4 after
                                rt_view / rt_render_views / rt_render_views_rgb8 were added, and after the rt_accum_* accumulators and
                                rt_adaptive were, and after rt_accum_create_ex, the feature reads and rt_accum_denoise / rt_denoise were, and
                                after rt_update_geometry and rt_ray / rt_render_rays / rt_render_rays_rgb8 were, and after
                                rt_update_geometry_device and rt_refit_times were, and after rt_set_environment / rt_env_pdf / rt_env_sample were,
                                and after rt_bake / rt_bake_rays / rt_lightmap_points were, and after rt_accum_attach_ids and the id reads were,
                                and after rt_accum_attach_light_groups and the light-group reads were: new entry points only, no existing layout changes */
#define RT_TEX_NONE (-1)
#define RT_ALL_DEVICES (-1) /* rt_create: one scene replica on every visible GPU + an RCCL communicator over them */

/* error codes */
enum {
    RT_OK = 0,
    RT_ERR_INVALID_ARG = 1,
    RT_ERR_NO_DEVICE = 2,   /* HIP runtime / GPU missing: the product never falls back to a CPU path */
    RT_ERR_HIP = 3,
    RT_ERR_OOM = 4,
    RT_ERR_IO = 5,
    RT_ERR_FORMAT = 6,
    RT_ERR_COMM = 7,
    RT_ERR_UNSUPPORTED = 8 /* a precondition of an optional fast path does not hold on this host; use the plain path */
};

/* RNG / transcendental policy of the sample loop.
 *   RT_RNG_DEVICE : counter-seeded xoshiro128++ stream per (pixel, sample) (include/rt_devspec.h). Scheduling
 *                   independent: any tiling / GPU count gives the same framebuffer. This is the production mode.
 *   RT_RNG_REFERENCE : the reference's stream: std::minstd_rand seeded with the 256-pixel span index
 *                   (raytracer.h:458,648; config.h:13) and the libstdc++-11 distribution algorithms,
 *                   one sequential stream per span. On the GPU one lane walks one span (parity mode,
 *                   not a performance mode): the image is the reference binary's, byte for byte.
 * Everything else is the reference's arithmetic in both modes, transcendentals included: sin / cos of the sampled
 * azimuths are glibc's sinf / cosf restated bit for bit (rt_devspec.h rt_sincos_libm, compared with libm on every
 * float of [0, 2 pi]); the modes differ in the random stream only.
 */
enum { RT_RNG_DEVICE = 0, RT_RNG_REFERENCE = 1 };

typedef struct rt_camera {
    float position[3];
    float right[3];
    float up[3];
    float forward[3];
    float fov_x; /* radians, as Camera::fov_x (scene.h:67) */
} rt_camera;

typedef struct rt_texture_desc {
    uint32_t width;
    uint32_t height;
    const uint8_t *rgba8; /* width*height*4, row-major, as stbi_load(..., 4) returns (geometry.h:586) */
} rt_texture_desc;

typedef struct rt_material_desc {
    float color[4];    /* material::color (geometry.h:605) */
    float emission[3]; /* material::emission */
    float roughness;
    float metallic;
    float ior;
    int32_t color_tex;    /* index into textures or RT_TEX_NONE */
    int32_t emissive_tex;
    int32_t metallic_roughness_tex;
    int32_t normal_tex;
} rt_material_desc;

/* Analytic primitives of the scene-txt front end (BASELINE configs 1-2; sample_data scene files: "ELLIPSOID rx ry rz", "PLANE nx ny nz"
 * with POSITION / ROTATION x y z w). The reference at HEAD renders triangles only (geometry.h:505) and keeps just an unused
 * intersect_ray_sphere (raytracer.h:61-77), so their semantics are DEFINED here (include/rt_primspec.h) and shared by the
 * HIP kernels and the CPU oracle: "parity unpinned" against the reference, bit-exact between the two. BOX and TRIANGLE
 * primitives are turned into triangles by the loader and take the (pinned) triangle path. */
enum { RT_PRIM_ELLIPSOID = 1, RT_PRIM_PLANE = 2 };
typedef struct rt_primitive_desc {
    uint32_t kind;        /* RT_PRIM_* */
    uint32_t material_id; /* into rt_scene_desc.materials; its textures are not sampled (scene-txt materials have none) */
    float param[3];       /* ELLIPSOID: semi-axes; PLANE: normal (need not be unit length) */
    float position[3];
    float rotation[4];    /* quaternion x y z w (order of sample_data and of geometry.h:154-156) */
} rt_primitive_desc;

/* Build-time tuning of rt_create. The reference's knobs are constexpr (config.h:7-47); these are per scene, and all-zero means
 * "the measured default" for every field, so a zero-initialised descriptor behaves as before. (Up to ABI 3 these were environment
 * variables read inside the library; now only the CLI, host/main.cpp, and bench.py translate environment into fields.) */
enum { RT_BUILDER_PLOC = 0, RT_BUILDER_LBVH = 1 };
typedef struct rt_build_options {
    uint32_t device_builder;  /* RT_BUILD_DEVICE_LBVH only: RT_BUILDER_PLOC (default; falls back to the radix tree when deeper than the
                                 traversal stacks) or RT_BUILDER_LBVH (Karras radix tree + refit) */
    uint32_t ploc_radius;     /* PLOC nearest-neighbour search radius, 1..32; 0 = 8 (profiles/r03_wide.txt) */
    uint32_t lbvh_leaf_tris;  /* triangles per leaf of the device-built binary tree, 1..8; 0 = 1 */
    uint32_t reserved0;       /* 0 (was node_order, a development placement option) */
    float wide_cost_node;     /* surface-area cost of a wide-node visit in the collapse; 0 = 1.0 */
    float wide_cost_tri;      /* ... of a triangle test; 0 = 0.3 */
    uint32_t reserved1;       /* 0 (was wide_order, read by nothing) */
    uint32_t reserved;        /* 0 */
} rt_build_options; /* rt_create refuses a non-zero reserved field */

typedef struct rt_scene_desc {
    uint32_t abi_version; /* RT_ABI_VERSION */
    uint32_t n_triangles;
    const float *positions;       /* 9*n : a.xyz b.xyz c.xyz */
    const float *normals;         /* 9*n */
    const float *texcoords;       /* 6*n */
    const float *tangents;        /* 9*n */
    const uint32_t *material_ids; /* n */
    uint32_t n_materials;
    const rt_material_desc *materials;
    uint32_t n_textures;
    const rt_texture_desc *textures;
    rt_camera camera;
    float bg_color[3];
    uint32_t ray_depth; /* Scene::ray_depth; 8 for glTF (scene.h:186, config.h:17) */
    uint32_t n_primitives; /* analytic primitives, tested by brute force next to the BVH (at most RT_MAX_PRIMITIVES) */
    const rt_primitive_desc *primitives;
    uint32_t build_flags; /* RT_BUILD_* */
    int32_t bg_texture;   /* Scene::bg (scene.h:81; main.cpp:29-31, config.h:36-38 USE_ENV_MAP / ENV_MAP_PATH): index into `textures` of the
                             environment map that Scene::bg_at (scene.h:83-89) samples by direction, RT_TEX_NONE = the reference's default, the
                             1x1 WHITE_TEXTURE (a constant bg_color background). Loaders: rt_loaded_set_env_map (rt_host.h) */
    rt_build_options build; /* all-zero = defaults */
} rt_scene_desc;
/* How rt_create builds the scene BVH (BVH::build, bvh.h:262-393):
 *   RT_BUILD_REFERENCE (default): on the host, in the reference's exact topology (same SAH sweep, same std::sort
 *       permutation) -> event counters and tie-breaking equal the reference's: the parity mode.
 *   RT_BUILD_DEVICE_LBVH: on the GPU (Morton sort + Karras radix tree + refit, csrc/rt_bvh_device.hip), tens of milliseconds
 *       for 10^7 triangles instead of seconds. Same closest hits (identical t), but a different topology: ties between
 *       equal-t triangles may resolve differently and the counters differ. One exception ("Two kinds of modes"): where
 *       coplanar triangles OVERLAP, two candidate hits lie within an ulp of each other and the reference's pruning rule lets the
 *       tree shape pick one, so such a ray may get the other triangle's hit, <= 4 ulp closer or farther, still a true hit of the
 *       triangle it names. Production mode for big scenes; also selected by
 *       the CLI's RT_BVH_DEVICE=1. The light BVH (emissive triangles only) is always built on the host.
 *   RT_BUILD_WIDE (may be combined with either binary builder): the binary tree is collapsed into an 8-wide tree whose nodes
 *       hold eight child boxes quantised conservatively to 8 bits per plane (80 B per node), chosen by a surface-area
 *       dynamic program; the wavefront pipeline then walks THAT tree with global-best culling and octant-ordered slots
 *       (csrc/wide_build.cpp, csrc/rt_wide.hip). Production mode: the closest hit over all triangles (t bit for bit the brute-force
 *       minimum: the reference's, or closer where the reference's own pruning skips a triangle; another index only on exact ties)
 *       with far fewer memory accesses per ray; event counters count wide nodes. The megakernel /
 *       reference-RNG parity renders are refused on such a scene (RT_ERR_UNSUPPORTED). The CLI sets it for RT_BVH_WIDE=1.
 *   RT_BUILD_WIDE_HOST_COLLAPSE (development; with RT_BUILD_DEVICE_LBVH | RT_BUILD_WIDE): read the device-built binary tree back and
 *       collapse it on the host (wide_build.cpp) instead of on the device — the cross-check of the device collapse.
 *   RT_BUILD_GROUP_COPY (tests; multi-GPU scenes): replace the RCCL exchange by peer copies, which lets a one-GPU box rehearse G > 1
 *       with repeated ordinals (RCCL refuses those). RT_BUILD_GROUP_SELF_EXCHANGE (tests): the first GPU's own blocks also travel
 *       through ncclSend / ncclRecv, which exercises the RCCL path with G = 1.
 *   RT_BUILD_TEX_TILED (tests, A/B runs): the textures one material samples together are stored as interleaved 16-byte records in
 *       4 x 2 tiles only. By default such a set stores one 64-byte footprint record per base texel (the four records of a bilinear
 *       lookup in one line, 4 x the memory) while the scene's footprint records stay below 2 GiB, and falls back to the tiled
 *       records beyond. Every sampled value is the same in both layouts, bit for bit.
 * rt_create refuses any other bit (8 was a development flag). */
enum { RT_BUILD_REFERENCE = 0, RT_BUILD_DEVICE_LBVH = 1, RT_BUILD_WIDE = 2, RT_BUILD_WIDE_HOST_COLLAPSE = 4, RT_BUILD_GROUP_COPY = 16,
       RT_BUILD_GROUP_SELF_EXCHANGE = 32, RT_BUILD_TEX_TILED = 128 };
#define RT_MAX_PRIMITIVES 4096u

/* Progress report of a render: called on the calling thread after every finished pass (pixel tile x sample range) of a single-GPU
 * scene, `done` of `total` passes; a multi-GPU scene reports once per GPU that finished, from that GPU's host thread (calls are
 * serialised). The reference prints "%d/%d     \r" per finished span (raytracer.h:647); the CLI does the same per pass under RT_VERBOSE. */
typedef void (*rt_progress_fn)(uint32_t done, uint32_t total, void *user);
/* Coherence sort of the rays of bounces >= 1 (wavefront pipeline; ordering never changes a result). rt_render refuses any other value
 * (2 - 5 and 7 were development keys). */
enum {
    RT_SORT_AUTO = 0,            /* octant + cell + sub-cone where the tree does not fit the caches, none for a cache-resident wide tree */
    RT_SORT_OFF = 1,
    RT_SORT_OCTANT_CELL_CONE = 6 /* direction octant, 64^3 origin cell, direction sub-cone (24 bits): what AUTO picks */
};
/* Primary rays as 64-ray packets (wf_extend_packet / wf_extend_wide_packet) */
enum {
    RT_PACKET_AUTO = 0, /* from 16 (binary tree) / 4 (wide tree) samples per pixel and pass, until the kernel's own census of a pass
                           shows fewer than packet_min_lanes lanes served per trip for this image size / samples per pass */
    RT_PACKET_OFF = 1,
    RT_PACKET_ON = 2
};

typedef struct rt_params {
    uint32_t width;
    uint32_t height;
    uint32_t samples;  /* SPP */
    uint32_t rng_mode; /* RT_RNG_* */
    uint64_t seed;     /* RT_RNG_DEVICE only */
    /* Image sharding: this call renders pixel blocks  b  with  b % shard_count == shard_index,
     * where block b = row-major pixels [b*shard_block, (b+1)*shard_block). Pixels of other shards are left
     * untouched in fb_rgb. shard_count = 0 or 1 renders everything. shard_block must be a multiple of 256
     * (the reference span, config.h:13) in RT_RNG_REFERENCE mode. */
    uint32_t shard_index;
    uint32_t shard_count;
    uint32_t shard_block;
    uint32_t flags; /* RT_FLAG_* */
    /* ---- ABI 4: tuning (all-zero = the measured defaults) and progress */
    uint32_t sort_mode;       /* RT_SORT_* */
    uint32_t packet_mode;     /* RT_PACKET_* */
    float packet_min_lanes;   /* RT_PACKET_AUTO: lanes served per packet trip below which later passes use the per-lane kernel;
                                 0 = 33 (binary tree, profiles/r02_packet.txt) / 20 (wide tree, profiles/r03_wide.txt) */
    uint32_t reserved0;       /* 0 */
    uint64_t max_paths;       /* paths (pixel, sample) per pass of the wavefront pipeline; 0 = 128 M, capped by free device memory */
    rt_progress_fn progress;  /* may be NULL */
    void *progress_user;
} rt_params;

enum {
    RT_FLAG_NONE = 0,
    RT_FLAG_DEVICE_FB = 1, /* fb_rgb is a device pointer (HBM resident); no D2H copy. The library writes it on the scene's
                              own non-blocking stream and synchronises that stream before returning, so results are
                              complete on return; PRECONDITION: the buffer must be idle on entry (the caller has
                              synchronised whatever stream last touched it, e.g. its allocation's zero-fill) — the
                              library's stream is not ordered with any caller stream. */
    RT_FLAG_COUNTERS = 2,  /* run the instrumented kernel variant and fill the event counters of rt_stats
                              (slower; timing fields are filled whenever `stats` is non-NULL) */
    RT_FLAG_MEGAKERNEL = 4, /* RT_RNG_DEVICE only: use the persistent one-lane-per-pixel megakernel instead of the
                              wavefront pipeline (same image bit for bit; kept as a cross-check. RT_RNG_REFERENCE
                              always uses the megakernel: its RNG stream is sequential per 256-pixel span) */
    RT_FLAG_GLOBAL_BEST = 8 /* production traversal (wavefront pipeline only): BVH::intersect_ray prunes a far child only
                              against the NEAR subtree's local best (bvh.h:216-223); with this flag every box is culled
                              against the GLOBAL best hit so far, which visits a subset of the reference's nodes. The
                              closest hit is the same (t bit for bit) except where a triangle's t rounds below its own
                              box's entry distance, or on exact ties; the event counters differ. Off by default: the
                              parity mode reproduces the reference's order and counters. The CLI sets it for RT_TRAVERSAL=global. */
};

/* Per-render statistics (optional out-parameter). Counters are layout independent event counts in the
 * reference's terms: what the reference algorithm touches, not what caches absorb. */
typedef struct rt_stats {
    uint64_t samples;
    uint64_t casts;          /* closest-hit traversals (raytracer.h:540-553) */
    uint64_t nodes_visited;  /* BVH::intersect_ray invocations (bvh.h:195) */
    uint64_t box_tests;      /* intersect(ray, aabb) calls (bvh.h:137) */
    uint64_t tri_tests;      /* intersect(ray, triangle) calls (bvh.h:52) */
    uint64_t shaded_hits;    /* to_intersection_info on closest hits (bvh.h:176) */
    uint64_t light_queries;  /* bvh_mix_dist::pdf calls (raytracer.h:363) */
    uint64_t light_nodes;
    uint64_t light_box_tests;
    uint64_t light_tri_tests;
    uint64_t light_hits;
    uint64_t texel_fetches;  /* texels read by Texture::sample (geometry.h:559-568), 4 per non-1x1 lookup */
    double kernel_ms;        /* device time of the render kernel(s), HIP events on the launch stream */
    double total_ms;         /* wall time of rt_render */
    double dominant_ms;      /* summed device time of the dominant kernel's launches (wf_extend; the megakernel when
                                that path is used), one HIP event pair per launch */
    uint32_t dominant_launches;
    uint32_t packet_lanes_x100; /* last packet census read back: lanes served per packet trip x 100 (0: no packet pass ran, or none
                                   has been read back yet) */
    uint32_t passes;            /* passes (pixel tile x sample range) of this render */
    uint32_t packet_passes;     /* ... whose primary rays went through the packet kernel */
} rt_stats;

typedef struct rt_scene rt_scene; /* opaque: device-resident scene + both BVHs */

/* Replaces RaytracerStaticContext(scene) (raytracer.h:440-454): builds scene_bvh and light_bvh with the
 * reference's SAH sweep (bvh.h:268-393) on the host, flattens them into the HBM layouts of DESIGN.md and
 * uploads everything to `device` (HIP ordinal). Caller keeps ownership of every pointer in `desc`. */
int rt_create(const rt_scene_desc *desc, int device, rt_scene **out);
void rt_destroy(rt_scene *scene);

/* Multi-GPU scenes (replaces the reference's thread pool over spans, raytracer.h:636-665, at node scale).
 * rt_create(desc, RT_ALL_DEVICES, &s) — or rt_create_on(desc, devices, n, &s) for an explicit list of HIP ordinals —
 * builds one replica of the scene per GPU (one host thread each) and ONE RCCL communicator over them (ncclCommInitAll),
 * inside this call. rt_render / rt_render_rgb8 on such a scene split the image into interleaved pixel blocks
 * (block b -> GPU b % G; 8 image rows per block unless rt_params.shard_block says otherwise; rt_params.shard_count must
 * be 0 or 1), render them concurrently and gather every GPU's blocks on the first GPU with grouped ncclSend/ncclRecv
 * (rgb8 with the device film: 3 B/pixel), then deliver the whole image to the caller's buffer (host memory, or memory of
 * the first GPU with RT_FLAG_DEVICE_FB). The image is bit-identical to a single-GPU render (per-(pixel, sample) seeding).
 * The probe entry points (rt_cast_rays, rt_light_pdf, rt_bvh_info, rt_film_rgb8) run on the first GPU's replica.
 * Errors: RT_ERR_COMM when RCCL cannot be loaded, refuses the device set, or an exchange fails.
 * Tests: build_flags RT_BUILD_GROUP_COPY / RT_BUILD_GROUP_SELF_EXCHANGE (above). */
int rt_create_on(const rt_scene_desc *desc, const int *devices, int n_devices, rt_scene **out);
int rt_scene_device_count(const rt_scene *scene); /* GPUs rendering for this scene (1 for rt_create on one device) */

/* Replaces run_raytracer(scene, image) (raytracer.h:629-674). Blocking. fb_rgb: width*height*3 floats,
 * row-major, y down, linear radiance = render_pixel(ctx,x,y) (raytracer.h:618-627). ray_depth == 0 is a
 * silent no-op like raytracer.h:630-631. `stats` may be NULL. */
int rt_render(rt_scene *scene, const rt_params *params, float *fb_rgb, rt_stats *stats);

/* Closest-hit probe: cast `n` rays through the scene BVH exactly as cast_ray (raytracer.h:540-553) with
 * min_dst = EPS. rays: 6*n floats (origin, dir). Outputs per ray: prim (original triangle index; n_triangles + i for
 * analytic primitive i; 0xFFFFFFFF for a miss), and bct[3] = (b, c, t) of bvh.h:83-85 ((0, 0, t) for an analytic
 * primitive). Used by the parity tests for bit-exact hit indices. */
int rt_cast_rays(rt_scene *scene, const float *rays, uint32_t n, uint32_t *prim_out, float *bct_out);

/* The same probe through the RENDERER's closest-hit kernels (the wavefront pipeline's wf_extend / wf_extend_packet over a
 * queue made of `rays`), so that tests exercise the production kernels on arbitrary rays. mode: RT_CAST_*. `stats` (optional)
 * receives the event counters of the launch (casts, nodes_visited, box_tests, tri_tests) and its device time. */
enum {
    RT_CAST_PROBE = 0,         /* = rt_cast_rays: one lane per ray, the reference's recursion as an explicit stack */
    RT_CAST_EXTEND = 1,        /* wf_extend, reference traversal order (parity mode) */
    RT_CAST_EXTEND_GLOBAL = 2, /* wf_extend, global-best pruning (RT_FLAG_GLOBAL_BEST) */
    RT_CAST_PACKET = 3,        /* wf_extend_packet (64 consecutive rays = one packet), reference order */
    RT_CAST_PACKET_GLOBAL = 4  /* wf_extend_packet, global-best pruning */
};
int rt_cast_rays_ex(rt_scene *scene, const float *rays, uint32_t n, uint32_t mode, uint32_t *prim_out, float *bct_out, rt_stats *stats);

/* Intersection-info probe: the closest hit of each ray as rt_cast_rays reports it, plus the two normals to_intersection_info
 * (bvh.h:80-121) hands to shade(): `normal` (the geometric normal, flipped to face the ray: bvh.h:86-87, 118) and `shading_normal`
 * (smooth normal through the normal map, flipped likewise: bvh.h:94-108, 119). For an analytic primitive both are its unit normal
 * facing the ray (rt_primspec.h). 3 floats each per ray, zeros for a miss; either output may be NULL. Lets the tests pin normals
 * against an independent evaluation (tests/test_gpu_txt.py: float64 closed forms for ELLIPSOID / PLANE). */
int rt_surface_normals(rt_scene *scene, const float *rays, uint32_t n, uint32_t *prim_out, float *t_out, float *normal_out, float *shading_normal_out);

/* Light-pdf probe: bvh_mix_dist::pdf (raytracer.h:363-375) for n (origin, dir) pairs. */
int rt_light_pdf(rt_scene *scene, const float *rays, uint32_t n, float *pdf_out);

/* Background probe: Scene::bg_at (scene.h:83-89) for n directions (3 floats each, as the render loop passes ray.dir: unit length is
 * the caller's business) -> n x rgb. With bg_texture = RT_TEX_NONE every answer is bg_color. */
int rt_bg_at(rt_scene *scene, const float *dirs, uint32_t n, float *rgb_out);

/* BVH introspection for parity tests: which = 0 scene_bvh, 1 light_bvh. Nodes are reported in the
 * reference's own pre-order numbering (bvh.h:157-163, 351-363): 10 x u32-sized words per node
 * {min.xyz, max.xyz (float bits), left, right, obj_begin, obj_end}; order = the BVH's object permutation
 * (BVH::objects, bvh.h:166) as original triangle indices. Pass NULL buffers to query counts. */
int rt_bvh_info(rt_scene *scene, int which, uint32_t *n_nodes, uint32_t *n_objects, uint32_t *root,
                uint32_t *nodes_out /* 10*n_nodes */, uint32_t *order_out /* n_objects */);

/* The BVH exactly as the traversal kernels see it, copied back from HBM (tests: validates what rt_create uploaded or built
 * on the device, not a host copy). nodes64: n_inner records of 16 words {lmin.xyz, lmax.xyz, rmin.xyz, rmax.xyz, left,
 * right, sel, pad}; a child ref is an inner index, or 0x80000000 | count << 27 | first triangle for a leaf. tris48: n_tris
 * records of 12 words {a.xyz, (b-a).xyz, (c-a).xyz, original triangle index, flags, pad}. Pass NULL buffers for the counts. */
int rt_bvh_device_dump(rt_scene *scene, int which, uint32_t *n_inner, uint32_t *n_tris, uint32_t *root, uint32_t *nodes64, uint32_t *tris48);
/* The compact node records of the binary scene tree (additive, RT_ABI_VERSION stays 4), copied back from HBM: n_inner records of 8 words
 * {six planes, left, right}, one per record of rt_bvh_device_dump(scene, 0) and in its order. Word 14 (`sel`) of THAT dump's records says how a
 * node's two children expand: per child (left: bits 0..6, right: bits 8..14) six selector bits and a valid bit. With C a child that has
 * `valid`, box(C) = its box in the parent's record (faces f = 0..5: min x, y, z, max x, y, z) and p = C's compact planes, C's own record is
 *   selector bit f clear: left child's face f = box(C)'s, right child's = p[f];      set: left child's = p[f], right child's = box(C)'s
 * and its child references are the compact record's, bit for bit. valid = 0: a leaf child, or a child some face of which does not follow
 * the rule; its compact record is zero. A NULL buffer: the count. RT_ERR_UNSUPPORTED for RT_BUILD_WIDE and multi-GPU scenes. */
int rt_bvh_compact_dump(rt_scene *scene, uint32_t *n_inner, uint32_t *compact32);
/* The same derivation on host arrays, by the code the device runs (no GPU needed): nodes64 = n_inner records of 16 words as
 * rt_bvh_device_dump returns them, whose `sel` words (word 14) are overwritten; compact32 = n_inner records of 8 words, written. */
int rt_compact_derive_host(uint32_t *nodes64, uint32_t n_inner, uint32_t *compact32);
/* PROBE, for tests only, like the dumps above (nothing a renderer calls; it may change without an ABI bump): overwrite plane `word` (0..11)
 * of record `node` of the binary scene tree in HBM, then derive the compact records and selector words again, as every build does. A plane
 * moved outwards leaves a correct, looser tree whose affected child loses `valid`: the one way to show the kernels a record that does not
 * follow the inheritance rule, which no builder makes. Blocking. */
int rt_bvh_patch_plane(rt_scene *scene, uint32_t node, uint32_t word, float value);
/* Of rt_stats::nodes_visited of the last call with counters on this scene: the inner-node visits the per-lane closest-hit kernel made from a
 * compact record (the second visit of a trip). 0 for multi-GPU scenes. */
int rt_second_visits(const rt_scene *scene, uint64_t *count);
/* The 8-wide scene BVH of a scene built with RT_BUILD_WIDE, copied back from HBM: nodes80 = n_nodes records of 20 words
 * (layout: WideNode, csrc/rt_device_types.h — origin xyz, exponents + inner mask, first inner child, first triangle, triangle
 * mask, pad, then qlo[3][8] and qhi[3][8] bytes); tris48 as in rt_bvh_device_dump, in the wide tree's order. NULL buffers: counts. */
int rt_bvh_wide_dump(rt_scene *scene, uint32_t *n_nodes, uint32_t *n_tris, uint32_t *depth, uint32_t *nodes80, uint32_t *tris48);
/* Wall time of the last rt_create's scene-BVH build in ms: {host build + flatten, 0} or {device build, upload of the raw arrays}. */
int rt_build_times(const rt_scene *scene, double *build_ms, double *upload_ms);
/* ... and of the wide collapse on top of it (RT_BUILD_WIDE; 0 otherwise): on the host (wide_build.cpp) after a host build, on the device after a device build. */
int rt_build_times_ex(const rt_scene *scene, double *build_ms, double *upload_ms, double *wide_ms);

/* Film (image.h:49-82): ACES -> gamma 1/2.2 -> x255 -> clamp -> round -> u8. Host function; n pixels. */
void rt_tonemap_rgb8(const float *rgb, size_t n_pixels, uint8_t *out_rgb8);

/* The same film on the device. rt_render_rgb8 = run_raytracer(scene, image) with the reference's own
 * output type: Image::set_pixel tone-maps each finished pixel at once (image.h:40-42), so the image the reference
 * holds after raytracer.h:629-674 is rgb8. Same parameters, sharding and flags as rt_render; `rgb8` receives
 * width*height*3 bytes (a device pointer with RT_FLAG_DEVICE_FB; only this shard's pixels are written), byte-identical
 * to rt_tonemap_rgb8 of the rt_render framebuffer. The gamma stage uses a threshold table derived from, and verified
 * against, the host libm's powf when the first call is made; if that verification fails the call returns an error
 * (no approximation is ever substituted). rt_film_rgb8 applies the device film to a caller-supplied host array. */
int rt_render_rgb8(rt_scene *scene, const rt_params *params, uint8_t *rgb8, rt_stats *stats);

/* Several camera views of one built scene in one call (turntables, stereo pairs, cube maps, multi-view datasets): no rebuild and
 * no re-upload of the BVH, the triangles or the texel pool per viewpoint. A view changes the camera and the RNG seed only.
 *   Output: view-major, fb[v][y][x][3] (rgb8: 3 bytes per pixel), n_views * width * height pixels. width, height, samples, rng_mode,
 *   flags, the tuning fields and progress are shared by all views and mean what they mean for rt_render; rt_params.seed is not read.
 *   Contract, bit for bit: view v equals rt_render / rt_render_rgb8 on a scene created from the same descriptor with
 *   camera = views[v].camera, rendered with seed = views[v].seed, in every mode (wavefront or megakernel, binary or wide tree, reference
 *   RNG). The scene's own camera is not changed: a later rt_render uses the creation camera. What the loaders placed relative to the
 *   creation camera stays where it is: the light triangle of rt_loaded_add_light_triangle does not follow the views.
 *   Sharding: shard_index / shard_count / shard_block select blocks of the view-major virtual image (n_views * height rows). In
 *   RT_RNG_REFERENCE mode, where one 256-pixel span is one sequential RNG stream of ONE view, n_views > 1 refuses shard_count > 1.
 *   Errors: RT_ERR_INVALID_ARG for n_views == 0, views == NULL, a non-zero reserved field or n_views * width * height >= 2^31;
 *   RT_ERR_UNSUPPORTED where rt_render would refuse the mode (a RT_BUILD_WIDE scene with the megakernel or the reference RNG).
 *   ray_depth == 0 leaves the buffer untouched, as in rt_render. */
typedef struct rt_view {
    rt_camera camera;  /* as rt_scene_desc.camera */
    uint32_t reserved; /* 0 */
    uint64_t seed;     /* RT_RNG_DEVICE stream seed of this view (rt_params.seed is not read) */
} rt_view;             /* 64 bytes */
int rt_render_views(rt_scene *scene, const rt_params *params, const rt_view *views, uint32_t n_views, float *fb_rgb, rt_stats *stats);
int rt_render_views_rgb8(rt_scene *scene, const rt_params *params, const rt_view *views, uint32_t n_views, uint8_t *rgb8, rt_stats *stats);

/* Radiance along caller-supplied rays (additive; RT_ABI_VERSION stays 4): the integrator behind any sensor model — panoramic, fisheye,
 * orthographic or thin-lens cameras, rolling shutters, irradiance probes, light-map texels. The rays and their RNG streams come from a
 * buffer instead of from rt_camera; everything after a path's first ray is rt_render's pipeline.
 * The rule, operation by operation. Let K = params->samples and G = rays_per_output (0 means 1).
 *   Sample s (0 <= s < K) of ray r:
 *     - the RNG is seeded with rt_xoshiro_seed(params->seed, r.stream, r.first_sample + s) (the sample index wraps mod 2^32);
 *     - two uniform_real(rng, 0.0f, 1.0f) draws are made and discarded: gen_ray's jitter draws (raytracer.h:527-538);
 *     - the value is sanitize_nans(trace_ray(Ray{r.origin, r.dir}, ray_depth)) (raytracer.h:593-616) with that RNG state,
 *     - through the scene's own traversal: parity, RT_FLAG_GLOBAL_BEST, or the wide tree of RT_BUILD_WIDE.
 *   Output j, for j < n_rays / G:
 *     - starts from +0.0;
 *     - adds the values of rays j*G .. j*G + G - 1 in that order, each ray's K samples in sample order;
 *     - is divided by (float)(G * K): render_pixel's loop (raytracer.h:618-627).
 *   out_rgb holds 3 floats per output. rt_render_rays_rgb8 is the device film on top: 3 bytes per output, byte-identical to rt_tonemap_rgb8
 *   of the float outputs.
 * Consequence, which is the contract: when the rays are a camera's own primary rays (origin and direction as gen_ray makes them for sample
 *   s of pixel p) with stream = p, first_sample = s, K = 1 and G = SPP, output p is pixel p of rt_render, bit for bit, and with
 *   RT_FLAG_COUNTERS every event counter equals rt_render's.
 * Scheduling independence: the order of the outputs, max_paths, the sort mode, the packet mode and the neighbours of a ray in the buffer
 *   change no bit of any output.
 * params: samples, seed, flags, the tuning fields and progress are read (flags may hold RT_FLAG_COUNTERS, RT_FLAG_GLOBAL_BEST and
 *   RT_FLAG_DEVICE_FB); width and height are not read; rng_mode must be RT_RNG_DEVICE; shard_count must be 0 or 1.
 * RT_FLAG_DEVICE_FB: `rays` AND the output are device pointers on the scene's GPU, idle on entry (as rt_render's framebuffer); `rays` must
 *   be 16-byte aligned.
 * A degenerate ray (a zero or non-finite component) is traversed as rt_cast_rays_ex traverses it; there is no host validation pass.
 * RT_OK and nothing written: n_rays == 0; a scene with ray_depth == 0 (as rt_render).
 * RT_ERR_INVALID_ARG: a NULL pointer with n_rays > 0; samples == 0; n_rays not a multiple of G; G * K or n_rays / G >= 2^31; a misaligned
 *   device ray buffer; shard_count > 1; an unknown flag; a pass option rt_render would refuse.
 * RT_ERR_UNSUPPORTED: RT_RNG_REFERENCE; RT_FLAG_MEGAKERNEL; a multi-GPU scene. */
typedef struct rt_ray {
    float origin[3];
    float dir[3];          /* used as given (no normalisation): unit length is the caller's business, as for rt_bg_at */
    uint32_t stream;       /* takes the pixel index's place in rt_xoshiro_seed(seed, stream, sample) */
    uint32_t first_sample; /* sample index of this ray's first sample */
} rt_ray;                  /* 32 bytes */
int rt_render_rays(rt_scene *scene, const rt_params *params, const rt_ray *rays, uint32_t n_rays, uint32_t rays_per_output, float *out_rgb, rt_stats *stats);
int rt_render_rays_rgb8(rt_scene *scene, const rt_params *params, const rt_ray *rays, uint32_t n_rays, uint32_t rays_per_output, uint8_t *rgb8, rt_stats *stats);

/* Sensor models evaluated on the device (additive; RT_ABI_VERSION stays 4): panoramic (equirectangular), equidistant fisheye,
 * orthographic and thin-lens cameras next to the reference's pinhole, for every entry point that makes an image. The sensor is evaluated in
 * the first stage of the wavefront pipeline, so sample s of pixel p is a pure function of (sensor, p, s) whichever call draws it.
 * The rule, operation by operation: IEEE binary32, evaluated as written, no contraction; vector expressions per component, left to right.
 * P, R, U, F are camera.position / right / up / forward, used as given. For sample s of pixel pix of a W x H image, x = pix % W, y = pix / W:
 *     rt_xoshiro_seed(&rng, seed, pix, s)
 *     ox = uniform_real(rng, 0, 1);  oy = uniform_real(rng, 0, 1)                  gen_ray's two draws, in gen_ray's order
 *     nx = 2 * ((float)x + ox) / (float)W - 1;   ny = 2 * ((float)y + oy) / (float)H - 1         gen_ray's own terms, in [-1, 1]
 *     tan_x = tanf(fov_x / 2), tan_y = tanf(fov_y / 2) with fov_y = atanf(tanf(fov_x / 2) * H / W) * 2   (host, as rt_render's)
 *     half_fov = fov_x / 2  (host, float)
 *   PINHOLE       o = P;  d = gen_ray's: norm((nx*tan_x)*R - (ny*tan_y)*U + 1.0f*F)
 *   EQUIRECT      a = PI_F * (nx + 1);  p = (PI_F * 0.5f) * (ny + 1)       azimuth + pi in [0, 2 pi]; polar angle from +U in [0, pi]
 *                 (sa, ca) = rt_sincos_libm(a);  (sp, cp) = rt_sincos_libm(p)
 *                 o = P;  d = norm((-(sp*sa))*R + cp*U + (-(sp*ca))*F)     the image centre looks along F, columns grow towards R, the top row towards U
 *   FISHEYE       px = nx;  py = ny * ((float)H / (float)W);  r = sqrtf(px*px + py*py);  th = r * half_fov     equidistant, fov_x across the width
 *                 (st, ct) = rt_sincos_libm(th)
 *                 o = P;  d = r == 0 ? norm(F) : norm((st*(px/r))*R - (st*(py/r))*U + ct*F)
 *   ORTHOGRAPHIC  half_h = half_width * (float)H / (float)W  (host, float)
 *                 o = P + (nx*half_width)*R - (ny*half_h)*U;  d = norm(F)
 *   THIN_LENS     q = (nx*tan_x)*R - (ny*tan_y)*U + 1.0f*F                 gen_ray's screen point, not normalised
 *                 rt_xoshiro_seed(&lens, seed ^ 0x9E3779B97F4A7C15, pix, s)  a second generator: the path's own stream is not advanced
 *                 l0 = uniform_real(lens, 0, 1);  l1 = uniform_real(lens, 0, 1)
 *                 rad = lens_radius * sqrtf(l0);  (sl, cl) = rt_sincos_libm((2 * PI_F) * l1)
 *                 e = (rad*cl)*R + (rad*sl)*U;  o = P + e;  d = norm(focus_distance * q - e)
 *   In every kind the path continues with `rng` as it stands after the two jitter draws and nothing else: where gen_ray leaves it.
 *   (rt_sincos_libm, uniform_real, rt_xoshiro_seed: rt_devspec.h. Every rt_sincos_libm argument lies in [0, 2 pi], the range on which
 *   that restatement equals libm's sinf / cosf on every float.)
 * Contracts, bit for bit:
 *   Sensor equals rays: view v of rt_render_sensors with samples = SPP equals rt_render_rays (K = 1, G = SPP, params->seed = sensor.seed) over
 *     the records rt_sensor_rays writes for that sensor; with RT_FLAG_COUNTERS every event counter agrees.
 *   Pinhole equals views: a RT_SENSOR_PINHOLE sensor gives view {camera, seed} of rt_render_views, counters included.
 *   Scheduling independence: max_paths, the sort mode, the packet mode and which other sensors share the call change no bit.
 * rt_render_sensors*: output view-major, fb[v][y][x][3] (rgb8: 3 bytes per pixel), like rt_render_views; the sensors of one call may be of
 *   different kinds. width, height, samples, the flags RT_FLAG_COUNTERS | RT_FLAG_GLOBAL_BEST | RT_FLAG_DEVICE_FB, the tuning fields and
 *   progress mean what they mean for rt_render; rt_params.seed is not read. Every single-GPU tree kind. ray_depth == 0: RT_OK, nothing written.
 *   RT_ERR_INVALID_ARG: a NULL argument or n_sensors == 0; an unknown kind; a non-zero reserved word; half_width, lens_radius or
 *     focus_distance outside the range stated at the field (for the kind that reads it); FISHEYE with fov_x not finite and > 0 or with
 *     (double)half_fov * sqrt(1 + (H/W)^2) > pi (a corner would look more than 180 degrees off axis: the library renders no dead pixels);
 *     n_sensors * width * height >= 2^31; shard_count > 1; samples == 0; an unknown flag; a pass option rt_render refuses.
 *   RT_ERR_UNSUPPORTED: RT_RNG_REFERENCE; RT_FLAG_MEGAKERNEL; a multi-GPU scene.
 * rt_sensor_rays: the same device function writes the n_pixels * samples rt_ray records of pixels [first_pixel, first_pixel + n_pixels) and
 *   samples [first_sample, first_sample + samples) of a width x height image: pixel-major, each pixel's samples adjacent, stream = pix,
 *   first_sample = s. flags: 0 (rays_out is a host buffer) or RT_FLAG_DEVICE_FB (a device buffer on the scene's GPU, 16-byte aligned, idle
 *   on entry). RT_ERR_INVALID_ARG: a NULL argument, what rt_render_sensors refuses of a sensor, an empty image, a pixel range past
 *   width * height, n_pixels * samples >= 2^31, a misaligned device buffer, any other flag. n_pixels == 0 or samples == 0 writes nothing.
 * rt_accum_create_sensor: rt_accum_create_ex with a sensor in place of {camera, seed}; everything else about the accumulator is unchanged.
 *   Its exactness contract reads: pixel p equals pixel p of rt_render_sensors with samples = n_p; the feature sums are those of each sample's
 *   primary ray as defined above. */
enum { RT_SENSOR_PINHOLE = 0, RT_SENSOR_EQUIRECT = 1, RT_SENSOR_FISHEYE = 2, RT_SENSOR_ORTHOGRAPHIC = 3, RT_SENSOR_THIN_LENS = 4 };
typedef struct rt_sensor {
    rt_camera camera;     /* position P and frame R = right, U = up, F = forward, used as given; fov_x read by PINHOLE, FISHEYE, THIN_LENS */
    uint32_t kind;        /* RT_SENSOR_* */
    float half_width;     /* ORTHOGRAPHIC: half the film width in world units, finite, > 0 */
    float lens_radius;    /* THIN_LENS: finite, >= 0 */
    float focus_distance; /* THIN_LENS: distance of the focal plane along F, finite, > 0 */
    uint32_t reserved[5]; /* 0 */
    uint64_t seed;        /* RT_RNG_DEVICE stream seed of this view */
} rt_sensor;              /* 96 bytes; fields a kind does not read are ignored */
int rt_render_sensors(rt_scene *scene, const rt_params *params, const rt_sensor *sensors, uint32_t n_sensors, float *fb_rgb, rt_stats *stats);
int rt_render_sensors_rgb8(rt_scene *scene, const rt_params *params, const rt_sensor *sensors, uint32_t n_sensors, uint8_t *rgb8, rt_stats *stats);
int rt_sensor_rays(rt_scene *scene, const rt_sensor *sensor, uint32_t width, uint32_t height, uint32_t first_pixel, uint32_t n_pixels, uint32_t first_sample, uint32_t samples, uint32_t flags, rt_ray *rays_out);

/* Baking on the device (additive; RT_ABI_VERSION stays 4): irradiance at surface points, spherical-harmonic light probes and light-map
 * texels. The first ray of every sample is made in the first stage of the wavefront pipeline from (seed, point.stream, sample), so a bake is
 * reproducible the way an image is, and the samples are folded on the device; everything in between is rt_render's pipeline.
 * The rule, operation by operation: IEEE binary32, evaluated as written, no contraction; vector expressions per component, left to right.
 * Let K = params->samples. Sample s (0 <= s < K) of point j, with S = bake->first_sample + s (wraps mod 2^32), p = position, n = normal, both
 * used as given:
 *     rt_xoshiro_seed(&rng, params->seed, stream, S)
 *     uniform_real(rng, 0, 1);  uniform_real(rng, 0, 1)                           made and discarded: the stream stands where a camera ray's stands
 *     rt_xoshiro_seed(&dg, params->seed ^ 0xD6E8FEB86659FD93, stream, S)          a second generator: the path's own stream is not advanced
 *     z = uniform_real(dg, -1, 1);  co_z = sqrtf(max(0, 1 - z*z))                 sphere_uniform (raytracer.h:94-105)
 *     phi = uniform_real(dg, 0, 2 * PI_F);  (sn, cs) = rt_sincos_libm(phi)
 *     v = (co_z*cs, co_z*sn, z)
 *   IRRADIANCE    d = norm(n + v);  o = p + offset * n                            the reference's cosine lobe, as shade() samples it
 *   SH9           d = v;  o = p                                                   normal and offset are not read
 *     L = sanitize_nans(trace_ray(Ray{o, d}, ray_depth)) with `rng`, through the scene's own traversal (parity, RT_FLAG_GLOBAL_BEST, wide).
 *   A degenerate ray (n + v = 0, a non-finite component) is traversed as rt_cast_rays_ex traverses it; no host pass validates positions or
 *   normals.
 * The fold: one owner per output float, samples in order s = 0, 1, ..., starting from +0.0, no float atomics.
 *   IRRADIANCE    out[j][c], 3 floats per point:    E   = (sum_s L_s.c / (float)K) * PI_F
 *   SH9           out[j][k][c], 27 floats per point: C_k = (sum_s (L_s.c * Y_k(d_s)) / (float)K) * (4.0f * PI_F), with d = (x, y, z):
 *     Y0 = 0.282094792f            Y1 = 0.488602512f*y          Y2 = 0.488602512f*z
 *     Y3 = 0.488602512f*x          Y4 = 1.092548431f*(x*y)      Y5 = 1.092548431f*(y*z)
 *     Y6 = 0.315391565f*(3.0f*(z*z) - 1.0f)                     Y7 = 1.092548431f*(x*z)      Y8 = 0.546274215f*(x*x - y*y)
 *   When the samples of a point are split over several passes (max_paths) the sums continue in pass order; between passes they stand in `out`.
 * rt_bake_rays: the same device function writes the n_points * samples records rt_ray{o, d, stream, first_sample = S} of samples
 *   [bake->first_sample, + samples): point-major, each point's samples adjacent. flags: 0 (points and rays_out are host buffers) or
 *   RT_FLAG_DEVICE_FB (both are device buffers on the scene's GPU, 16-byte aligned, idle on entry).
 * Contracts, bit for bit:
 *   Bake equals rays: IRRADIANCE equals PI_F * the outputs of rt_render_rays (K = 1, G = samples, the same seed) over rt_bake_rays' records;
 *     SH9 equals the fold above applied to the per-ray outputs (G = 1) of those records. With RT_FLAG_COUNTERS every event counter equals
 *     rt_render_rays'.
 *   Scheduling independence: max_paths, the sort mode, the packet mode and the neighbours of a point in the buffer change no bit.
 * params: samples, seed, flags (RT_FLAG_COUNTERS | RT_FLAG_GLOBAL_BEST | RT_FLAG_DEVICE_FB), the tuning fields and progress are read; width
 *   and height are not; rng_mode must be RT_RNG_DEVICE. RT_FLAG_DEVICE_FB: `points` and `out` are device pointers on the scene's GPU, idle on
 *   entry; `points` must be 16-byte aligned, `out` 4-byte.
 * RT_OK and nothing written: n_points == 0; a scene with ray_depth == 0.
 * RT_ERR_INVALID_ARG: a NULL pointer with n_points > 0; an unknown kind; a non-zero reserved word of rt_bake_desc (and, for host points, of a
 *   point: device points are not read back); a non-finite offset; samples == 0; samples or n_points >= 2^31 (rt_bake_rays: n_points * samples
 *   >= 2^31); a misaligned device buffer; shard_count > 1; an unknown flag; a pass option rt_render refuses.
 * RT_ERR_UNSUPPORTED: RT_RNG_REFERENCE; RT_FLAG_MEGAKERNEL; a multi-GPU scene. */
typedef struct rt_bake_point {
    float position[3];
    float normal[3];   /* used as given (no normalisation) */
    uint32_t stream;   /* takes the pixel index's place in rt_xoshiro_seed(seed, stream, sample) */
    uint32_t reserved; /* 0 */
} rt_bake_point;       /* 32 bytes */
enum { RT_BAKE_IRRADIANCE = 0, RT_BAKE_SH9 = 1 };
typedef struct rt_bake_desc {
    uint32_t kind;         /* RT_BAKE_* */
    uint32_t first_sample; /* sample index of every point's first sample */
    float offset;          /* IRRADIANCE: the origin is lifted by offset * normal; finite */
    uint32_t reserved[5];  /* 0 */
} rt_bake_desc;            /* 32 bytes (a C identifier names the entry point or the record, not both) */
int rt_bake(rt_scene *scene, const rt_params *params, const rt_bake_desc *bake, const rt_bake_point *points, uint32_t n_points, float *out, rt_stats *stats);
int rt_bake_rays(rt_scene *scene, const rt_bake_desc *bake, uint64_t seed, const rt_bake_point *points, uint32_t n_points, uint32_t samples, uint32_t flags, rt_ray *rays_out);

/* The texel centres of a light-map atlas as bake points (additive). The scene supplies the device and the stream only; the arrays are the
 * caller's: per triangle 9 position floats, 9 normal floats (one normal per corner) and 6 atlas coordinates (u, v per corner, the atlas
 * spans [0, 1]^2, v grows with the row).
 * The rule, in IEEE binary32 as written. Texel q = y*W + x has the centre cx = ((float)x + 0.5f) / (float)W, cy = ((float)y + 0.5f) / (float)H.
 * For triangle t with atlas corners a, b, c, corner positions A, B, C and corner normals Na, Nb, Nc:
 *     area = (b.x-a.x)*(c.y-a.y) - (b.y-a.y)*(c.x-a.x)                            0 or not finite: the triangle covers nothing
 *     w1 = ((cx-a.x)*(c.y-a.y) - (cy-a.y)*(c.x-a.x)) / area
 *     w2 = ((b.x-a.x)*(cy-a.y) - (b.y-a.y)*(cx-a.x)) / area
 *     w0 = 1.0f - w1 - w2
 *     covered iff w0 >= 0 && w1 >= 0 && w2 >= 0                                   either winding; edges are inclusive
 *   The owner of q is the lowest covering t (as if every (t, q) pair were tested). The point of an owned texel:
 *     position = w0*A + w1*B + w2*C;  normal = norm(w0*Na + w1*Nb + w2*Nc);  stream = q;  reserved = 0
 *   Points are written in increasing q, texels_out[i] = q of point i. *n_points (a host word in either form) receives the number of owned
 *   texels even when it exceeds `capacity`; then the first `capacity` points are written and the call returns RT_OK.
 * flags: 0 (host arrays) or RT_FLAG_DEVICE_FB: the three inputs are device pointers as rt_update_geometry_device takes them (4-byte aligned,
 *   idle, read in place) and points_out / texels_out are device pointers, points_out 16-byte aligned.
 * RT_ERR_INVALID_ARG: a NULL argument (the inputs only with n_tris > 0, the outputs only with capacity > 0); width or height 0;
 *   width * height >= 2^31; a misaligned device pointer; any other flag. RT_ERR_UNSUPPORTED: a multi-GPU scene. n_tris == 0 writes no point
 *   and *n_points = 0.
 * Not covered: conservative coverage of texels a triangle only touches, seam dilation, packing and unwrapping. */
int rt_lightmap_points(rt_scene *scene, const float *positions, const float *normals, const float *lm_uv, uint32_t n_tris, uint32_t width, uint32_t height,
                       uint32_t flags, rt_bake_point *points_out, uint32_t *texels_out, uint32_t capacity, uint32_t *n_points);

/* Resumable sample accumulators: progressive and adaptive rendering (additive; RT_ABI_VERSION stays 4).
 * An accumulator belongs to one scene, one image size (width x height) and one view (a camera and an RT_RNG_DEVICE seed). It keeps, in
 * device memory, for every pixel p:
 *   S_p  the sum of its samples 0 .. n_p - 1, added in sample order (float3; starts at +0.0),
 *   E_p  the sum of its even-index samples 0, 2, 4, ..., added in the same order (float3; starts at +0.0),
 *   n_p  its sample count (u32).
 * Exactness: after any sequence of accumulator calls, pixel p of the resolved image equals, bit for bit, pixel p of rt_render with
 *   samples = n_p on the same scene, with the same flags, camera and seed (rt_render_views with {camera, seed} for a camera other than the
 *   scene's own): for the parity traversal and RT_FLAG_GLOBAL_BEST, binary or wide device-built trees, any max_paths, sort mode and packet
 *   mode, and any split of the samples over calls. Sample s of pixel p is seeded from (seed, p, s) whichever call draws it, and one lane
 *   adds a pixel's new samples onto S_p / E_p in sample order (no float atomics), so no result depends on scheduling. A pixel with
 *   n_p = 0 resolves to 0.
 * Scope: the RT_RNG_DEVICE wavefront pipeline on one GPU.
 *   RT_RNG_REFERENCE -> RT_ERR_UNSUPPORTED: one minstd_rand stream runs sequentially through a whole 256-pixel span, so a pixel's later
 *     samples cannot be drawn without replaying the span.
 *   RT_FLAG_MEGAKERNEL -> RT_ERR_UNSUPPORTED (the megakernel renders whole pixels, not sample lists).
 *   A multi-GPU scene (rt_create_on, RT_ALL_DEVICES) -> RT_ERR_UNSUPPORTED at rt_accum_create.
 *   shard_count > 1 or RT_FLAG_DEVICE_FB in the render params -> RT_ERR_INVALID_ARG.
 * An rt_render on the same scene between accumulator calls does not disturb the accumulator (it shares the scene's stream and
 * wavefront workspace, never the accumulator's own buffers).
 *
 * The adaptive rule (rt_accum_render_adaptive), exactly:
 *   error of pixel p: +inf if n_p < 2; otherwise, with h = (n_p + 1) / 2 (integer), I = S_p / n_p, A = E_p / h per component in float,
 *     err_p = (|I.r - A.r| + |I.g - A.g| + |I.b - A.b|) / (1e-4f + sqrtf(I.r + I.g + I.b))
 *   (the half-buffer estimate; a NaN or infinite err_p counts as not converged).
 *   Pixel p is ACTIVE when n_p < max_samples and (n_p < min_samples or some q of the 3x3 window around p, clipped at the image border,
 *     has !(err_q <= threshold)).
 *   Round 0 brings every pixel below min_samples up to it (min_samples - n_p samples: these differ per pixel when the accumulator is not
 *     fresh). Each later round judges every pixel again and adds min(step, max_samples - n_p) samples to each active pixel. The call
 *     returns when a judge finds no active pixel (it always terminates: an active pixel gains at least one sample per round). *rounds
 *     receives the number of rounds that added samples.
 *   After return, for every pixel: n_p >= max_samples (a progressive call may have gone past the cap; such pixels are never active), or
 *     every err_q of its window is <= threshold. rt_accum_read's `error` is the err of the current state: what the last judge saw.
 *   rt_params.progress is called once per finished round with (round, total): total is 1 + ceil((max - min) / step), the rounds one pixel
 *   can take part in; a pixel whose neighbours gained samples may become active again, and then total grows with round.
 * RT_ERR_INVALID_ARG: a NULL argument; params->samples == 0 for rt_accum_render; params width / height other than the accumulator's;
 *   min_samples == 1; max_samples < min_samples; a threshold that is NaN, negative or infinite; a non-zero reserved field.
 * A scene with ray_depth == 0 makes rt_accum_render* a no-op, as it does rt_render. */
typedef struct rt_accum rt_accum; /* opaque */
/* camera NULL: the scene's creation camera. */
int rt_accum_create(rt_scene *scene, uint32_t width, uint32_t height, const rt_camera *camera, uint64_t seed, rt_accum **out);
void rt_accum_destroy(rt_accum *acc); /* precondition: before rt_destroy of its scene */
/* Adds params->samples samples to EVERY pixel (a progressive step). params: width / height must equal the accumulator's, seed is not read,
 * rng_mode must be RT_RNG_DEVICE; the flags RT_FLAG_COUNTERS / RT_FLAG_GLOBAL_BEST, the tuning fields and progress mean what they mean for
 * rt_render. stats (may be NULL) sums over every pass of the call; stats->samples is the number of samples added. */
int rt_accum_render(rt_accum *acc, const rt_params *params, rt_stats *stats);

typedef struct rt_adaptive {
    float threshold;       /* >= 0 and finite; 0 sends every pixel to max_samples except where a whole window has err exactly 0 */
    uint32_t min_samples;  /* 0 = 16; otherwise >= 2 */
    uint32_t max_samples;  /* >= min_samples */
    uint32_t step;         /* samples added to each active pixel per round; 0 = 32 (profiles/adaptive_sponza.txt: half the rounds of 16 at
                              the same error; every round pays ~ray_depth closest-hit launch tails) */
    uint32_t reserved[4];  /* 0 */
} rt_adaptive;             /* 32 bytes */
/* params->samples is not read; everything else as rt_accum_render. `rounds` may be NULL. */
int rt_accum_render_adaptive(rt_accum *acc, const rt_params *params, const rt_adaptive *ad, uint32_t *rounds, rt_stats *stats);

/* The image: S_p / (float)n_p per pixel (0 where n_p = 0), exactly as rt_render's last pass divides. flags: 0 (host buffer) or
 * RT_FLAG_DEVICE_FB (a device buffer). rt_accum_resolve_rgb8 applies the device film on top: == rt_tonemap_rgb8 of the float image. */
int rt_accum_resolve(rt_accum *acc, uint32_t flags, float *fb_rgb);
int rt_accum_resolve_rgb8(rt_accum *acc, uint32_t flags, uint8_t *rgb8);
/* Copies the state to host buffers (any may be NULL): S (3 floats per pixel), E (3 floats), n, and err (as the last judge computed it;
 * +inf everywhere before the first adaptive call). */
int rt_accum_read(rt_accum *acc, float *sum_rgb, float *even_sum_rgb, uint32_t *samples, float *error);

/* First-hit feature sums (the auxiliary images a denoiser is guided by; additive, RT_ABI_VERSION stays 4).
 * rt_accum_create_ex is rt_accum_create with flags: accum_flags = 0 IS rt_accum_create; RT_ACCUM_FEATURES makes the accumulator keep, for
 * every pixel p, four more fields, each added to by the lane that adds to S_p, in the same sample order, in the same rounds (no float atomics):
 *   AS_p  float3: sum over the samples of the albedo of the closest hit of the sample's primary ray: material.color.rgb x colour texture, the
 *         colour to_intersection_info (bvh.h:80-121) hands to shade(). A miss adds (0, 0, 0).
 *   NS_p  float3: sum of that hit's shading normal, facing the ray, as rt_surface_normals reports it (an analytic primitive: its normal).
 *         A miss adds (0, 0, 0).
 *   ZS_p  float: sum of the hit distance t. A miss adds 0.
 *   h_p   u32: number of samples whose primary ray hit.
 * The primary ray of sample s of pixel p is the one seeded from (seed, p, s), the first ray of that sample's path; its first hit is the closest
 * hit the scene's own traversal returns. The alpha coin of shade() (raytracer.h:559) is not consulted: a hit that shading passes through still
 * counts. Every call that adds samples adds their features (rt_accum_render, rt_accum_render_adaptive, any split over passes and lists), so
 * after any sequence of calls the four sums are functions of n_p alone, like S_p. S_p, E_p, n_p, the image and the event counters of rt_stats
 * are those of an accumulator without the flag, bit for bit. An accumulator without the flag allocates and launches nothing new.
 * Any other bit of accum_flags -> RT_ERR_INVALID_ARG; every other refusal is rt_accum_create's. RT_ERR_OOM when the per-path feature records
 * (32 B per path of a pass) do not fit beside the wavefront workspace. */
enum { RT_ACCUM_FEATURES = 1 };
int rt_accum_create_ex(rt_scene *scene, uint32_t width, uint32_t height, const rt_camera *camera, uint64_t seed, uint32_t accum_flags, rt_accum **out);
/* rt_accum_create_ex for a sensor (rt_sensor above: the rule, the refusals): the view is {sensor, sensor->seed}. */
int rt_accum_create_sensor(rt_scene *scene, uint32_t width, uint32_t height, const rt_sensor *sensor, uint32_t accum_flags, rt_accum **out);
/* The raw sums (any pointer may be NULL): AS, NS (3 floats per pixel), ZS (1 float), h (u32). RT_ERR_INVALID_ARG without RT_ACCUM_FEATURES. */
int rt_accum_read_features(rt_accum *acc, float *albedo_sum, float *normal_sum, float *depth_sum, uint32_t *hits);
/* The means (any pointer may be NULL): albedo = AS / (float)n, normal = NS / (float)n (NOT renormalised), depth = ZS / (float)h (0 where
 * h = 0); all 0 where n = 0. flags: 0 or RT_FLAG_DEVICE_FB (all three are device buffers). RT_ERR_INVALID_ARG without RT_ACCUM_FEATURES. */
int rt_accum_resolve_features(rt_accum *acc, uint32_t flags, float *albedo, float *normal, float *depth);

/* rt_accum_denoise: an edge-avoiding a-trous filter over the accumulator's image, guided by its feature means and by the noise estimate its
 * half buffer E gives, on the device. Needs RT_ACCUM_FEATURES (else RT_ERR_INVALID_ARG). The accumulator is not modified: denoise, add
 * samples, denoise again. fb_rgb: width * height * 3 floats (a device buffer with RT_FLAG_DEVICE_FB; `flags` is 0 or that).
 * The rule, exactly. Only + - * / fabsf min max and comparisons, IEEE binary32, no contraction, in the order written (sums left to right):
 *   A pixel is VALID when n_p > 0. An invalid pixel outputs (0, 0, 0) and is never a tap. For a valid pixel, with fn = (float)n, h = h_p:
 *     C = S / fn, alb = AS / fn, N = NS / fn (per component), Z = ZS / (float)h (0 when h = 0), m = (float)(n - h) / fn,
 *     den_c = (alb_c + m) + 1e-3f   (1.0f for every channel with RT_DENOISE_NO_DEMODULATE),
 *     L0 = C / den                  (the working signal: the image with the first hit's albedo divided out),
 *     d_p = (|C.r - A.r| / den.r + |C.g - A.g| / den.g) + |C.b - A.b| / den.b with A = E / (float)((n + 1) / 2);  d_p = +inf when n < 2,
 *     s_p = (sum of d_q over the valid pixels q of the 3x3 window around p clipped at the image border, row-major) / (float)(their number).
 *   Iteration i = 0 .. K-1 (K = iterations) has stride t = 2^i and reads L^i, writes L^(i+1). Taps q = p + t * (dx, dy), dy = -2..2 outer,
 *   dx = -2..2 inner, the centre included; a tap outside the image or invalid is skipped. k = (1/16, 1/4, 3/8, 1/4, 1/16).
 *     w = (((k[dy+2] * k[dx+2]) * wn) * wz) * wc, and the centre tap has wn = wz = wc = 1. For the other taps:
 *     wn: a = (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z, pp and qq likewise from (N_p, N_p) and (N_q, N_q). pp == 0 and qq == 0 -> 1;
 *         else a <= 0 or pp * qq == 0 -> 0; else c = (a * a) / (pp * qq), then c = c * c `normal_sharpness` times; wn = c.
 *     wz: h_p == 0 and h_q == 0 -> 1; exactly one of them 0 -> 0; else
 *         r = (Z_p - Z_q) / ((sigma_depth * (float)(t * max(|dx|, |dy|))) * max(Z_p, Z_q)), wz = 1 / (1 + r * r).
 *     wc: e = ((|L_p.r - L_q.r| + |L_p.g - L_q.g|) + |L_p.b - L_q.b|) / ((sigma_color * s_p) * (1 / (float)t) + 1e-6f), wc = 1 / (1 + e * e)
 *         (L of iteration i; s_p = +inf makes wc = 1: a pixel with a neighbourhood of n < 2 is filtered by geometry alone).
 *     L^(i+1)_p = (sum of w * L^i_q) / (sum of w), both sums in tap order starting from 0; the centre makes the divisor >= 9/64.
 *   Output: L^K * den per channel.
 * Which lane or block computes a pixel, and whether its taps come through LDS, changes no result.
 * rt_accum_denoise_rgb8 applies the device film on top: == rt_tonemap_rgb8 of rt_accum_denoise's image.
 * RT_ERR_INVALID_ARG: a NULL accumulator or buffer, flags other than RT_FLAG_DEVICE_FB, iterations > 8, normal_sharpness > 8, a sigma that is
 *   negative, NaN or infinite, an unknown bit of rt_denoise.flags, a non-zero reserved field. opt NULL = all defaults. */
enum { RT_DENOISE_NO_DEMODULATE = 1 };
typedef struct rt_denoise {
    uint32_t iterations;       /* K; 0 = 5, at most 8 */
    float sigma_color;         /* 0 = 8.0 */
    float sigma_depth;         /* 0 = 0.5 */
    uint32_t normal_sharpness; /* squarings of the squared cosine: 0 = 3 (cos^16); at most 8 */
    uint32_t flags;            /* RT_DENOISE_* */
    uint32_t reserved[3];      /* 0 */
} rt_denoise;                  /* 32 bytes; all-zero = the defaults (measured: profiles/denoise_quality.txt) */
int rt_accum_denoise(rt_accum *acc, const rt_denoise *opt, uint32_t flags, float *fb_rgb);
int rt_accum_denoise_rgb8(rt_accum *acc, const rt_denoise *opt, uint32_t flags, uint8_t *rgb8);

/* Id mattes: which object, material or triangle a pixel shows, and with what coverage (additive; RT_ABI_VERSION stays 4).
 * rt_accum_attach_ids makes an accumulator keep, for every pixel, a table of the ids its samples saw. Ids are attached by this call, not by a
 * bit of accum_flags; they may be combined with RT_ACCUM_FEATURES.
 * The id of a sample. The id of sample s of pixel p belongs to the closest hit of that sample's primary ray: the ray seeded from (seed, p, s),
 *   or the sensor's ray, as the scene's own traversal returns it (parity, RT_FLAG_GLOBAL_BEST, wide): the hit the feature sums use. The alpha
 *   coin of shade() (raytracer.h:559) is not consulted. A miss gives RT_ID_MISS.
 *   RT_ID_PRIMITIVE: what rt_cast_rays reports as `prim`: the original triangle index, or n_triangles + i for analytic primitive i.
 *   RT_ID_MATERIAL:  that triangle's material_ids entry, or primitives[i].material_id.
 *   RT_ID_USER:      table[prim]. The table is copied at attach and the caller keeps theirs. An entry equal to RT_ID_MISS is legal and counts
 *                    with the misses.
 * The table of a pixel. Each pixel has K slots (id_j, c_j), j = 0 .. K-1, and a counter `other`; all start at (0, 0) and 0. The pixel's samples
 *   are taken in sample order s = 0, 1, ...; for the id of each:
 *     if some slot j with c_j > 0 has id_j == id:  c_j += 1;
 *     else if some slot has c_j == 0:              the lowest such j takes (id, 1);
 *     else:                                        other += 1.
 *   Slots fill in first-seen order and nothing is ever evicted, so (sum of c_j) + other = n_p, a slot with c_j == 0 reads id_j == 0, and the
 *   table is exact for the ids it holds: only the samples counted in `other` are unaccounted for. After any sequence of rt_accum_render /
 *   rt_accum_render_adaptive calls the table is a function of n_p alone, like S_p: for any split over calls, passes and lists, any max_paths,
 *   sort mode and packet mode. One lane owns a pixel's table for a list entry and walks its new samples in order; there are no atomics.
 * What stays the same. S_p, E_p, n_p, the feature sums, the image, err and every event counter of an accumulator with ids are, bit for bit,
 *   those of one without. An accumulator without ids allocates and launches nothing new.
 * rt_accum_attach_ids: once per accumulator, before any call has added samples to it.
 *   RT_ERR_INVALID_ARG: a NULL accumulator or desc; an unknown kind; slots > RT_ID_MAX_SLOTS; a non-zero reserved word; a flag other than
 *   RT_FLAG_DEVICE_FB; RT_ID_USER with a NULL table or n_table != n_triangles + n_primitives of the scene; another kind with a table or a
 *   non-zero n_table; a device table that is not 4-byte aligned; a second attach; an attach after samples were added.
 *   RT_ERR_OOM (from a later render call): the per-path id records (4 B per path of a pass) do not fit beside the wavefront workspace.
 *   After any refusal the accumulator is unchanged.
 * rt_accum_read_ids: the tables on the host, any pointer may be NULL: ids [p][K], counts [p][K] (u32 each), other [p].
 * rt_accum_resolve_labels: label_p = the id_j of the slot with the largest c_j, ties to the lowest j; coverage_p = (float)c_j / (float)n_p.
 *   With n_p = 0: RT_ID_MISS and 0. `other` is not consulted: a pixel whose table overflowed may have a more frequent id that never got a
 *   slot; a caller who cares checks `other` from rt_accum_read_ids (or attaches more slots). Either output may be NULL. flags: 0 (host
 *   buffers) or RT_FLAG_DEVICE_FB (both are device buffers on the scene's GPU, 4-byte aligned, idle on entry).
 * rt_accum_resolve_matte: matte_p = (float)(sum of c_j over the slots with c_j > 0 whose id_j is one of ids[0 .. n_ids-1]) / (float)n_p: an
 *   integer sum, then one division; 0 with n_p = 0. Duplicates in `ids` count once; RT_ID_MISS is an id like any other. `ids` is always a
 *   host array, 1 <= n_ids <= 4096; `matte` is a host buffer, or a device buffer with RT_FLAG_DEVICE_FB.
 * The three reads: RT_ERR_INVALID_ARG for a NULL accumulator, an accumulator without ids, a flag other than RT_FLAG_DEVICE_FB, a NULL `ids`
 *   or `matte`, n_ids outside 1..4096. */
enum { RT_ID_PRIMITIVE = 0, RT_ID_MATERIAL = 1, RT_ID_USER = 2 };
#define RT_ID_MISS 0xFFFFFFFFu
#define RT_ID_MAX_SLOTS 16u
typedef struct rt_id_desc {
    uint32_t kind;         /* RT_ID_* */
    uint32_t slots;        /* K: 1..16; 0 = 4 */
    const uint32_t *table; /* RT_ID_USER: n_table words, the id of original triangle i, then of analytic primitive i; else NULL */
    uint32_t n_table;      /* RT_ID_USER: must equal n_triangles + n_primitives of the scene; else 0 */
    uint32_t flags;        /* 0, or RT_FLAG_DEVICE_FB: table is a device pointer on the scene's GPU, 4-byte aligned, idle on entry */
    uint32_t reserved[2];  /* 0 */
} rt_id_desc;              /* 32 bytes */
int rt_accum_attach_ids(rt_accum *acc, const rt_id_desc *desc);
int rt_accum_read_ids(rt_accum *acc, uint32_t *ids, uint32_t *counts, uint32_t *other);
int rt_accum_resolve_labels(rt_accum *acc, uint32_t flags, uint32_t *label, float *coverage);
int rt_accum_resolve_matte(rt_accum *acc, uint32_t flags, const uint32_t *ids, uint32_t n_ids, float *matte);

/* Light groups: a pixel's radiance split by the emitter it came from, so that lights can be dimmed, tinted or switched off after the render
 * (additive; RT_ABI_VERSION stays 4). rt_accum_attach_light_groups makes an accumulator keep G more sums per pixel, GS_g,p. Groups are attached
 * by this call, not by a bit of accum_flags; they combine with RT_ACCUM_FEATURES, with ids and with sensor accumulators, on every tree kind and
 * under RT_FLAG_GLOBAL_BEST. rt_accum_denoise is untouched (denoising a mix is not offered).
 * The value of a sample, V. The value sample s of pixel p adds to S_p is the fold of its path's frames (raytracer.h:588-590). It starts from the
 *   path's terminal value T: the background of a miss; the hit's emission at one of shade()'s three early exits (the sampled direction is NaN,
 *   :569-571; p < EPS, :576-578; the scale is 0, :584-586); or (0,0,0) when the depth budget is used up (:596-598). Then, for every pending frame
 *   b from the innermost outwards: res = e_b + res * scl_b, with e_b the emission of frame b's hit. Then sanitize_nans (:607-616).
 * Whose a value is. e_b belongs to the material of frame b's hit: material_ids[prim] of a triangle, primitives[i].material_id of an analytic
 *   primitive; its group is material_group[that material]. An emission T belongs to its hit's material in the same way; a background T belongs
 *   to background_group; a depth-exhausted T is (+0,+0,+0) in every group. RT_LIGHT_GROUP_NONE (for a material or for the background) means
 *   no group: that emitter is in S_p and in no GS_g,p.
 * The value of a group, V_g. The same sequence of binary32 operations with every e_b and T whose group is not g replaced by (+0,+0,+0), then
 *   sanitize_nans of V_g itself. No decision of a path reads an emission value, so the paths, the scales and every event counter are those of
 *   the ungrouped sample.
 * The group sums. GS_g,p = the sum of V_g over pixel p's samples, in sample order s = 0, 1, ..., in binary32 from +0: the lane that adds a
 *   list entry's samples to S_p adds their V_g to GS_g,p, in the same rounds; there are no float atomics. After any sequence of
 *   rt_accum_render / rt_accum_render_adaptive calls GS_g,p is a function of n_p alone, like S_p: for any split over calls, passes and lists,
 *   any max_paths, sort mode and packet mode.
 * Exactness. The fold never mixes colour channels, so a channel that only one group's emitters feed is, in that group, bit for bit the
 *   channel of S_p. In general the groups need NOT add up to S_p bit for bit: float addition is not associative, and V = sum of V_g holds in
 *   real numbers only (a NaN that sanitize_nans removes from V may also survive in no V_g, or be removed from several).
 * What stays the same. S_p, E_p, n_p, err, the feature sums, the id tables, every image, every event counter and every adaptive decision of
 *   an accumulator with groups are, bit for bit, those of one without. An accumulator without groups allocates and launches nothing new.
 * rt_accum_attach_light_groups: once per accumulator, before any call has added samples to it. material_group is copied; the caller keeps
 *   theirs.
 *   RT_ERR_INVALID_ARG: a NULL accumulator or desc; n_groups outside 1..RT_LIGHT_GROUP_MAX; a NULL material_group; n_materials other than the
 *   scene's material count; a material_group entry or a background_group that is neither < n_groups nor RT_LIGHT_GROUP_NONE; a non-zero
 *   reserved word; a flag other than RT_FLAG_DEVICE_FB; a device table that is not 4-byte aligned; a second attach; an attach after samples
 *   were added.
 *   RT_ERR_OOM (from a later render call): the per-path records (n_groups x 16 B and ray_depth + 1 tag bytes per path of a pass) do not fit
 *   beside the wavefront workspace.
 *   After any refusal the accumulator is unchanged.
 * rt_accum_read_light_groups: GS on the host, [G][pixels][3] floats.
 * rt_accum_resolve_light_group: fb_p = GS_group,p / (float)n_p per channel, 0 where n_p = 0. fb_rgb: width * height * 3 floats (a device
 *   buffer with RT_FLAG_DEVICE_FB; `flags` is 0 or that, here and below).
 * rt_accum_resolve_light_mix: relighting. weights is always a host array of G x 3 floats, w[g][c]. Per pixel and channel c, in binary32 with
 *   no contraction: acc = +0; for g = 0 .. G-1 ascending: acc = acc + (GS_g,p[c] / (float)n_p) * w[g][c]; fb_p[c] = acc. A quotient is 0
 *   where n_p = 0. All-ones weights give the image up to the rounding named under "Exactness"; a weight may be negative, inf or NaN and is used
 *   as given.
 * rt_accum_resolve_light_mix_rgb8 applies the device film on top: == rt_tonemap_rgb8 of rt_accum_resolve_light_mix's image.
 * The four reads: RT_ERR_INVALID_ARG for a NULL accumulator, an accumulator without groups, group >= G, a flag other than RT_FLAG_DEVICE_FB, a
 *   NULL buffer or NULL weights. */
#define RT_LIGHT_GROUP_MAX  8u
#define RT_LIGHT_GROUP_NONE 0xFFFFFFFFu
typedef struct rt_light_group_desc {
    uint32_t n_groups;              /* G: 1..RT_LIGHT_GROUP_MAX */
    uint32_t background_group;      /* < G, or RT_LIGHT_GROUP_NONE */
    const uint32_t *material_group; /* n_materials words: each < G, or RT_LIGHT_GROUP_NONE */
    uint32_t n_materials;           /* must equal the scene's material count */
    uint32_t flags;                 /* 0, or RT_FLAG_DEVICE_FB: material_group is a device pointer on the scene's GPU, 4-byte aligned, idle on entry */
    uint32_t reserved[2];           /* 0 */
} rt_light_group_desc;              /* 32 bytes */
int rt_accum_attach_light_groups(rt_accum *acc, const rt_light_group_desc *desc);
int rt_accum_read_light_groups(rt_accum *acc, float *group_sums /* [G][pixels][3] */);
int rt_accum_resolve_light_group(rt_accum *acc, uint32_t group, uint32_t flags, float *fb_rgb);
int rt_accum_resolve_light_mix(rt_accum *acc, const float *weights /* G x 3 */, uint32_t flags, float *fb_rgb);
int rt_accum_resolve_light_mix_rgb8(rt_accum *acc, const float *weights, uint32_t flags, uint8_t *rgb8);

/* New per-triangle arrays for a built scene (animation frames, deforming meshes, simulation steps) without rt_destroy + rt_create
 * (additive; RT_ABI_VERSION stays 4). Blocking; runs on the scene's own stream. The call replaces the five per-triangle arrays of the
 * creation descriptor; all five must be non-NULL when n_triangles > 0, and the caller keeps ownership of them. Everything else is the
 * scene's as created and is neither read again nor uploaded again: materials, textures, the texel pool and the tables; the analytic
 * primitives; the camera; bg_color, bg_texture, ray_depth, build_flags and build.
 *   RT_UPDATE_REBUILD (every single-GPU build kind): afterwards the scene is, for every entry point, the scene rt_create would build from
 *     the creation descriptor with those five arrays swapped in: both BVHs, the triangle, shading and light records, the ray-ordering
 *     bounds and rt_build_times* are those of that fresh scene. A parity scene stays a parity scene (the reference's topology of the new
 *     geometry, its image and its counters). The new buffers are built beside the live ones, then swapped in and the old ones freed.
 *   RT_UPDATE_REFIT (scenes built with RT_BUILD_WIDE, collapsed on the host or on the device): the 8-wide tree keeps its topology: slot
 *     states, group bases and the order of the triangle records (DevTri::prim per record) stay. Every triangle record, shading record, node
 *     origin, cell exponent and quantised plane is recomputed for the new arrays, each by the rule the builders use for a node with those
 *     contents (the scene grids of the new bounds, the origin snap, the cell exponent, floor / ceil planes): a pure function of the topology
 *     and the arrays, whichever lane computes it. The light BVH and the light records are rebuilt as in REBUILD, so the set of lights
 *     follows the new material_ids. The hit contract is the wide tree's (the closest hit over all triangles, another index only on exact
 *     ties): a topology chosen for other positions can cost node visits, never a hit. Rebuild when the visits grow. After a
 *     REFIT rt_bvh_info(0) returns RT_ERR_UNSUPPORTED: the binary tree the wide one was collapsed from no longer describes the scene.
 *   Either mode resets the packet policy of rt_render* (it was measured on the old tree).
 * RT_ERR_INVALID_ARG (checked before any device work): a NULL scene, struct or array; n_triangles other than the scene's; an unknown mode;
 *   a non-zero reserved word; a material id >= the scene's material count; a non-finite position; a scene with a live accumulator
 *   (rt_accum_create* without its rt_accum_destroy): its sums are of the old geometry.
 * RT_ERR_UNSUPPORTED: a multi-GPU scene; RT_UPDATE_REFIT on a scene built without RT_BUILD_WIDE (a refitted binary tree would not be the
 *   reference's topology); either mode on a RT_BUILD_WIDE scene whose new extent leaves the wide tree's exponent range (rt_create's test).
 * After RT_ERR_INVALID_ARG, RT_ERR_UNSUPPORTED or RT_ERR_OOM the scene is unchanged, bit for bit. */
enum { RT_UPDATE_REBUILD = 0, RT_UPDATE_REFIT = 1 };
typedef struct rt_geometry_update {
    uint32_t n_triangles;         /* must equal the scene's */
    uint32_t mode;                /* RT_UPDATE_* */
    const float *positions;       /* 9*n, as rt_scene_desc */
    const float *normals;         /* 9*n */
    const float *texcoords;       /* 6*n */
    const float *tangents;        /* 9*n */
    const uint32_t *material_ids; /* n */
    uint32_t reserved[4];         /* 0 */
} rt_geometry_update;             /* 64 bytes */
int rt_update_geometry(rt_scene *scene, const rt_geometry_update *upd);

/* rt_update_geometry for arrays that are in HBM already (a cloth solver, skinning or a physics step in torch; additive, RT_ABI_VERSION stays
 * 4): the same struct and the same modes, but the five pointers are DEVICE pointers on the scene's GPU. Blocking.
 *   Equivalence: after RT_OK the scene is, bit for bit and for every entry point and dump, the scene rt_update_geometry leaves when given
 *     host copies of the same bytes in the same mode: both trees (the light tree included: rt_bvh_info(1), rt_bvh_device_dump(1)), every
 *     record, the packet-policy reset, the rt_bvh_info(0) refusal after a REFIT. rt_build_times* report the same builds; upload_ms is 0
 *     where nothing was uploaded (build_ms starts once the build's sort and bounds buffers are allocated, for both entry points).
 *   Buffers: the arrays are read, never written, and not retained: the caller may overwrite or free them as soon as the call returns. They
 *     must be idle on entry (no pending work of the caller's writes them): the library reads them on the scene's own stream and
 *     synchronises it before returning, the rule of RT_FLAG_DEVICE_FB. Each pointer must be 4-byte aligned and nothing more: a view that
 *     starts one element into a larger allocation is legal.
 *   What crosses the bus: the bounds of the vertices and the verdict of the checks (8 words), then the emissive triangles alone (their
 *     indices and positions, 40 bytes each) for the light BVH, which is still built on the host, and that tree back. RT_UPDATE_REFIT reads
 *     the caller's arrays in place: nothing is allocated or copied for them. RT_UPDATE_REBUILD of a scene built with RT_BUILD_DEVICE_LBVH
 *     builds from them in place. Legal, but not the fast path: RT_UPDATE_REBUILD of a scene whose build reads the arrays on the host (the
 *     reference-topology builds, i.e. no RT_BUILD_DEVICE_LBVH; the host collapse of a wide tree, i.e. RT_BUILD_WIDE_HOST_COLLAPSE or a
 *     RT_BUILD_WIDE scene of 8 triangles or fewer) stages one device-to-host copy of the five arrays and runs rt_update_geometry's path.
 * Refusals: rt_update_geometry's, with the same codes. The material id and the non-finite position are found by a kernel (the message names
 *   the lowest offending triangle, as the host loop does; no message depends on scheduling). Added, RT_ERR_INVALID_ARG both: a pointer that
 *   is not 4-byte aligned ("misaligned"; checked with the struct, before the scene is looked at), and a pointer for which
 *   hipPointerGetAttributes does not report device memory of the scene's GPU, pinned host memory included ("not device memory"; checked
 *   before any launch, at the first and the last byte of each array: what lies between them is the caller's word). After any refusal the scene is unchanged, bit for bit: every check, every allocation and the exponent-range test
 *   come before the first write to anything a render kernel reads. */
int rt_update_geometry_device(rt_scene *scene, const rt_geometry_update *upd);
/* Wall time of the last successful RT_UPDATE_REFIT of `scene` through either entry point (0, 0 before the first): *refit_ms the refit of records
 * and nodes on the device, *levels_ms the part of it spent in the top-down level pass, which reads the topology alone (one launch and one
 * host read per level). A measurement aid, like rt_build_times. RT_ERR_INVALID_ARG: a NULL argument; RT_ERR_UNSUPPORTED: a multi-GPU scene. */
int rt_refit_times(const rt_scene *scene, double *refit_ms, double *levels_ms);

/* Shutter accumulators: motion blur from two geometry keys and two views (additive; RT_ABI_VERSION stays 4). rt_accum_attach_shutter gives an
 * accumulator a shutter: the time of a sample is a pure function of its sample index, all samples of one time are rendered against the scene
 * updated to that time, and the accumulator adds them in sample order as it always does. No closest-hit kernel knows about time. The layer
 * keeps no sums of its own; it combines with RT_ACCUM_FEATURES, ids, light groups and sensor accumulators, on every single-GPU tree kind.
 * The rule, operation by operation: IEEE binary32 evaluated as written, no contraction. K = slices, B = block.
 *   Slice of a sample. For sample index s of any pixel: j = (s / B) mod K (integers); k = the log2(K) low bits of j in reverse order. With
 *     this order every power-of-two number of consecutive blocks of a progressive render covers the shutter evenly.
 *   Time of a slice. t_k = open + (close - open) * (((float)k + 0.5f) / (float)K).
 *   Geometry at t. For every float x of positions, normals and tangents, with x0 and x1 its values in key 0 and key 1:
 *       b = x0 + t * (x1 - x0)                       (three roundings)
 *       lo = x0 <= x1 ? x0 : x1;   hi = x0 <= x1 ? x1 : x0
 *       x(t) = !(b > lo) ? lo : (!(b < hi) ? hi : b)
 *     the blend held between the keys by comparisons alone. So every slice lies inside the union of the keys' bounds in floats, not only
 *     in real numbers (at t = 1 the unclamped b can leave [x0, x1]); a b that is NaN (keys of opposite sign whose difference overflows)
 *     gives lo; equal keys give key 0's bits, the sign of a zero included. Texcoords and material ids are the descriptor's at every t.
 *   Sensor at t (on the host; sensor1 == NULL: the accumulator's own view, untouched, at every t). P, fov_x, half_width, lens_radius and
 *     focus_distance are b of the same expression, without the clamp. R, U and F are blended per component in the same way, then each
 *     vector (x, y, z) is divided, component by component, by sqrtf(x*x + y*y + z*z), for R, U, F in that order. Kind and seed are sensor
 *     0's. The record is then made like any other (rt_sensor above). Two keys describe small rotations only: the blended axes are unit
 *     vectors but orthogonal only to first order in the angle between the keys.
 *   Rendering. rt_accum_render on an accumulator that holds n samples per pixel cuts the call's sample range [n, n + samples) into maximal
 *     runs of one slice (K = 1: the whole call). For each run it installs slice k: the geometry exactly as
 *     rt_update_geometry_device(the arrays at t_k, mode) leaves a scene, and the sensor record at t_k; then it adds the run's samples to every
 *     pixel as rt_accum_render does, with every layer the accumulator keeps. Sample s of pixel p is seeded from (seed, p, s) as ever.
 *     rt_stats of such a call: the counters and passes sum over its runs; kernel_ms spans the slice changes between them as well.
 *   On return from rt_accum_attach_shutter and from every render call the scene is what rt_update_geometry_device(key 0, mode) leaves, and
 *     the view the accumulator's own: every other entry point sees key 0. With n_triangles == 0 the geometry is never touched.
 * Exactness (in place of the accumulators' sentence): after any sequence of calls, S_p is the in-order binary32 sum over s < n of X(p, s),
 *   where X(p, s) is sample s of pixel p of rt_render_sensors with sensor(t_k) on a scene updated to geometry(t_k) in that mode, k the slice of
 *   s; E_p likewise over even s; n_p = n for every pixel; the sums of the other layers likewise. Consequences, bit for bit: K = 1 is a plain
 *   accumulator on the blended static scene; equal keys and sensor1 == NULL are a plain accumulator on a scene updated with key 0; how
 *   `samples` is split over calls changes nothing. The accumulator's packet policy is kept across slices (scheduling independence).
 * Cost. A slice change is one streaming blend plus rt_update_geometry_device's work without its pointer checks. When no emissive triangle (by
 *   material_ids) has a position float whose keys differ in any bit, an RT_UPDATE_REFIT slice skips the light half of the update (a list
 *   across the bus, a host build, a tree back): the tree it would build is key 0's bit for bit. Choose B so that a run's render time
 *   dominates the change (DESIGN.md "Shutter" quotes the measured figures).
 * rt_accum_attach_shutter: once per accumulator, before any call has added samples to it, on a scene whose only live accumulator it is. The
 *   keys are copied to device memory the accumulator owns (with RT_FLAG_DEVICE_FB they are device arrays under rt_update_geometry_device's
 *   buffer rules); the caller keeps theirs.
 *   RT_ERR_INVALID_ARG: a NULL argument; a second attach; an attach after samples were queued; another live accumulator on the scene;
 *     n_triangles neither 0 nor the scene's; a NULL array with n_triangles > 0; a misaligned device array or one that is not device memory of
 *     the scene's GPU; a non-finite position or a material id out of range in either key (found by the update's check kernel, lowest triangle
 *     named); K not a power of two in 1..1024; B == 0; !(0 <= open <= close <= 1); an unknown mode; a flag other than RT_FLAG_DEVICE_FB;
 *     sensor1 of another kind than the accumulator's view, or one rt_render_sensors refuses; a non-zero reserved word. Also:
 *     rt_accum_create* on a scene while an accumulator with a shutter lives. rt_update_geometry* keeps refusing the scene while any lives.
 *   RT_ERR_UNSUPPORTED: rt_accum_render_adaptive on an accumulator with a shutter (per-pixel counts would put one pass at several times);
 *     what rt_update_geometry refuses in that mode: RT_UPDATE_REFIT without RT_BUILD_WIDE, either key outside the wide tree's exponent range.
 *   After any refusal the scene and the accumulator are unchanged. (The exponent range has a lower end too: keys that cross so that a slice's
 *   extent collapses below 2^-52 where neither key's does make that render call return RT_ERR_UNSUPPORTED, with key 0 installed again.)
 * rt_accum_shutter_times: of the last rt_accum_render call, *slice_changes the slices it installed and *slice_change_ms their wall time in
 *   all (blend, update, sensor upload; the return to key 0 is not counted). A measurement aid, like rt_refit_times.
 * rt_accum_shutter_info: *static_lights 1 when the light half is skipped as described; *light_rebuilds the installs since attach, slices and
 *   returns to key 0, that built a light tree. Both: RT_ERR_INVALID_ARG for a NULL argument or an accumulator without a shutter. */
typedef struct rt_shutter_desc {
    uint32_t n_triangles;         /* the scene's, or 0: the geometry does not move (a camera-only shutter; every scene kind) */
    uint32_t mode;                /* RT_UPDATE_REFIT (RT_BUILD_WIDE scenes) or RT_UPDATE_REBUILD: how a slice's geometry is installed */
    const float *positions[2];    /* key 0 (t = 0) and key 1 (t = 1), 9*n floats each */
    const float *normals[2];      /* 9*n each */
    const float *tangents[2];     /* 9*n each */
    const float *texcoords;       /* 6*n: not interpolated */
    const uint32_t *material_ids; /* n: not interpolated */
    const rt_sensor *sensor1;     /* the view at t = 1; NULL: the view does not move. The accumulator's own view is t = 0; same kind required */
    float open, close;            /* 0 <= open <= close <= 1 */
    uint32_t slices;              /* K: a power of two, 1..1024 */
    uint32_t block;               /* B >= 1: consecutive samples that share a slice */
    uint32_t flags;               /* 0: host arrays; RT_FLAG_DEVICE_FB: device arrays on the scene's GPU, 4-byte aligned, idle on entry */
    uint32_t reserved[7];         /* 0 */
} rt_shutter_desc;                /* 128 bytes */
int rt_accum_attach_shutter(rt_accum *acc, const rt_shutter_desc *desc);
int rt_accum_shutter_times(rt_accum *acc, double *slice_change_ms, uint32_t *slice_changes);
int rt_accum_shutter_info(rt_accum *acc, uint32_t *static_lights, uint32_t *light_rebuilds);

/* Motion vectors: a first-hit optical-flow layer for accumulators (additive; RT_ABI_VERSION stays 4). rt_accum_attach_flow gives an accumulator
 * two geometry keys and an optional second view; every sample then also records the screen-space displacement, between the keys, of the
 * surface point its primary ray sees. The layer has the shape of the ids and the light groups: per-path records behind bounce 0's closest
 * hits, a fold in sample order, read and resolve entry points. It changes no other sum. include/rt_flowspec.h is this rule as code, for host
 * and device. The rule, operation by operation: IEEE binary32, evaluated as written, no contraction; vector expressions per component, left
 * to right.
 *   The point of a sample. Sample s of pixel p has the primary ray (o, d) that the sensor rule above makes of (sensor, p, s); its closest hit
 *     (k, b, c, t) is the one the scene's own traversal returns: the hit the feature sums and the ids use. The alpha coin is not consulted.
 *       a miss                                   the sample has no flow
 *       an analytic primitive, or n_triangles == 0   X0 = X1 = o + t * d
 *       a triangle of original index i           Xk = (V0k * ((1 - b) - c) + V1k * b) + V2k * c for k = 0, 1, from positions[k][9*i ..]
 *     (triangle::interop of the reference). Both points come from the same expression: a triangle whose keys are equal gives X0 == X1 bit
 *     for bit.
 *   Projection proj(sensor, W, H, X) -> (fx, fy, ok), the inverse of the sensor rule. v = X - P; r = dot(v, R), u = dot(v, U), f = dot(v, F),
 *     each (x*x' + y*y') + z*z'. tan_x, tan_y, half_fov and half_h are the host values of the sensor record.
 *       PINHOLE, THIN_LENS (through the lens centre)   ok = f > 0;  nx = (r / f) / tan_x;  ny = (-(u / f)) / tan_y
 *       ORTHOGRAPHIC  ok = f > 0;  nx = r / half_width;  ny = (-u) / half_h
 *       EQUIRECT      len = sqrtf((r*r + u*u) + f*f);  ok = len > 0;  nx = rt_atan2f_libm(r, f) / PI_F;
 *                     q = u / len held to [-1, 1] by comparisons (q < -1 ? -1 : q > 1 ? 1 : q);  ny = (-rt_asinf_libm(q)) / (PI_F * 0.5f)
 *       FISHEYE       rho = sqrtf(r*r + u*u);  th = rt_atan2f_libm(rho, f);  rr = th / half_fov
 *                     rho == 0: ok = f > 0, nx = ny = 0;  else ok = true, nx = rr * (r / rho), ny = (rr * ((-u) / rho)) / ((float)H / (float)W)
 *     then fx = (nx + 1) * (0.5f * (float)W), fy = (ny + 1) * (0.5f * (float)H). Pixel x covers [x, x + 1): the inverse of
 *     nx = 2 * (x + ox) / W - 1. The inverse is that of an orthonormal frame; R, U and F are used as given.
 *   Flow of a sample. (fx0, fy0, ok0) = proj(the accumulator's view, X0); (fx1, fy1, ok1) = proj(sensor1, or the same view, X1);
 *     dx = fx1 - fx0; dy = fy1 - fy0. EQUIRECT only, the seam: dx > 0.5f*W subtracts (float)W once, dx < -0.5f*W adds it once. The sample is
 *     VALID iff it hit, ok0 && ok1, and dx and dy are finite. The flow is not clipped to the image: a point that leaves the frame still has one.
 *   Per pixel, over its samples in sample order (one lane owns the pixel, no atomics):
 *       FS_p (2 floats) += (dx, dy) of every valid sample;  m_p (u32) counts them
 *       NT_p (float), NF_p (2 floats): a valid sample replaces them iff no valid sample came before, or its t < NT_p strictly: the nearest
 *         surface wins, a tie goes to the lowest s
 *     All four are functions of n_p alone, for any split over calls, passes and lists, any max_paths, sort mode and packet mode.
 *   Resolve. RT_FLOW_MEAN: flow = FS / (float)m; RT_FLOW_NEAREST: flow = NF; (0, 0) where m == 0. mask = (float)m / (float)n, 0 where n == 0.
 *   With flow attached S, E, n, features, ids, light groups, the image and every event counter are those of an accumulator without it, bit for
 *     bit; an accumulator without flow allocates and launches nothing new.
 * rt_accum_attach_flow: once per accumulator, before any call has added samples to it. The keys are copied to device memory the accumulator
 *   owns; the caller keeps theirs. Key 0 is the geometry the scene holds now: the caller's word, not checked.
 *   RT_ERR_INVALID_ARG: a NULL argument; a second attach; an attach after samples were added; n_triangles neither 0 nor the scene's; a NULL key
 *     with n_triangles > 0; a misaligned device array or one that is not device memory of the scene's GPU; a non-finite position in either key
 *     (found by the update's check kernel, lowest triangle named); an unknown flag; a non-zero reserved word; sensor1 of another kind than the
 *     accumulator's view, or one rt_render_sensors refuses.
 *   RT_ERR_UNSUPPORTED: flow together with a shutter, in either attach order: a slice's geometry is not key 0.
 *   RT_ERR_OOM (from a later render call): the per-path records (16 B per path of a pass) do not fit beside the wavefront workspace.
 *   After any refusal nothing is changed.
 * rt_accum_read_flow: the raw state (any pointer may be NULL): FS [p][2], m [p], NF [p][2], NT [p].
 * rt_accum_resolve_flow: flow [p][2] and mask [p] (either may be NULL), host buffers, or device buffers on the scene's GPU with
 *   RT_FLAG_DEVICE_FB (4-byte aligned, idle on entry), as rt_accum_resolve_labels. RT_ERR_INVALID_ARG: an unknown mode or flag.
 * Both reads: RT_ERR_INVALID_ARG for a NULL accumulator or one without flow. */
enum { RT_FLOW_MEAN = 0, RT_FLOW_NEAREST = 1 };
typedef struct rt_flow_desc {
    uint32_t n_triangles;      /* the scene's, or 0: no triangle moves (camera-only flow; every scene kind) */
    uint32_t flags;            /* 0: host arrays; RT_FLAG_DEVICE_FB: device arrays on the scene's GPU, 4-byte aligned, idle on entry */
    const float *positions[2]; /* key 0 (the geometry the scene holds now: the caller's word, not checked) and key 1; 9*n floats each, as rt_scene_desc */
    const rt_sensor *sensor1;  /* the view at key 1; NULL: the accumulator's own view. Same kind as the accumulator's view */
    uint32_t reserved[8];      /* 0 */
} rt_flow_desc;                /* 64 bytes */
int rt_accum_attach_flow(rt_accum *acc, const rt_flow_desc *desc);
int rt_accum_read_flow(rt_accum *acc, float *flow_sum /*[p][2]*/, uint32_t *valid /*[p]*/, float *near_flow /*[p][2]*/, float *near_t /*[p]*/);
int rt_accum_resolve_flow(rt_accum *acc, uint32_t mode, uint32_t flags, float *flow /*[p][2]*/, float *mask /*[p]*/);

/* Image-based lighting: a float radiance map as the scene's environment, optionally importance-sampled (additive; RT_ABI_VERSION stays 4).
 * rt_create's bg_texture is the reference's Scene::bg: an 8-bit texture with gamma, which clips an .hdr file to [0, 1]. rt_set_environment
 * replaces that lookup by a float map for a built scene. The texels are copied to device memory (float4 each); the caller keeps `rgb`.
 * The rule, operation by operation: IEEE binary32 evaluated as written, no contraction, unless double is named. W = width, H = height.
 *   Radiance   Le(dir) = bg_color * env(u, v), per component, with (u, v) = rt_bg_uv(dir) (rt_devspec.h), unchanged. env is Texture::sample's
 *     lookup (geometry.h:545-575) over the float texels: tx = wrap_repeat(u) * (float)W, ty = wrap_repeat(v) * (float)H, x0 = (int)tx,
 *     y0 = (int)ty, dx = tx - (float)x0, dy = ty - (float)y0, x1 = x0 + 1 (0 behind the last column), y1 likewise (row H - 1 wraps to row 0,
 *     as the reference's does), env = (1 - dx) * ((1 - dy) * t[y0][x0] + dy * t[y1][x0]) + dx * ((1 - dy) * t[y0][x1] + dy * t[y1][x1]).
 *     No 8-bit decode, no gamma. A 1x1 map returns bg_color * its texel without evaluating (u, v), like the reference's 1x1 path.
 *   Distribution (RT_ENV_IMPORTANCE), piecewise constant over the W x H cells; cell (i, j) = (y0, x0) of the lookup above, i.e.
 *     u in [j/W, (j+1)/W), v in [i/H, (i+1)/H) up to the float rounding of tx, ty.
 *     M_ij = max(0, lum(t[i][j]), lum(t[i1][j]), lum(t[i][j1]), lum(t[i1][j1])), i1 / j1 the wrapped successors: every texel a lookup inside
 *       the cell can read; lum(t) = (0.2126f * (bg.r * t.r) + 0.7152f * (bg.g * t.g)) + 0.0722f * (bg.b * t.b). So pdf > 0 wherever Le > 0.
 *     Omega_i = (2 pi / W) * (c_i - c_(i+1)) in double on the host, c_i = cos(pi * i / H) in double (c_0 = 1, c_H = -1): the solid angle
 *       of a cell of row i. w_ij = (double)M_ij * Omega_i.
 *     Prefix sums in double, in this order, for a sequence a_0 .. a_(n-1) (a row's w_ij, n = W; then the H row totals, n = H): C = ceil(n / 256);
 *       chunk c holds a_(cC) .. a_(cC + C - 1); L_k = the sum of its chunk's elements up to a_k, left to right; B_c = the sum of the totals of
 *       chunks 0 .. c-1, left to right; P_k = B_c + L_k. cdf[0] = 0, cdf[k+1] = (float)(P_k / P_(n-1)), cdf[n] = 1; a row of total 0 gets
 *       cdf[k+1] = (float)(k+1) / (float)n (its marginal cell is empty: nothing selects it).
 *     Tables: row_i[0..W] for every row, each normalised on its own, and marg[0..H] over the row totals. p_ij is DEFINED from the stored float
 *       tables, p_ij = (marg[i+1] - marg[i]) * (row_i[j+1] - row_i[j]), and pdf(dir) = p_ij / (float)Omega_i with (i, j) the cell of dir:
 *       a solid-angle density. Sampling and pdf agree by construction. A cell lighter than the float spacing of its table has p_ij = 0.
 *     A map whose weights are all zero has no distribution: the flag then acts as if it were not set.
 *   Sample, from four uniforms x0 .. x3 in [0, 1) (uniform_real(rng, 0, 1), in this order):
 *     i = the last index in [0, H) with marg[i] <= x0;  j = the last index in [0, W) with row_i[j] <= x1   (binary searches; never an empty cell)
 *     u = ((float)j + x2) / (float)W;  dy = c_i - x3 * (c_i - c_(i+1)) with the float edges   (uniform in solid angle inside the cell)
 *     r = sqrtf(max(0, 1 - dy * dy));  (s, c) = rt_sincos_libm((2 * PI_F) * u);  dir = (-(r * c), dy, -(r * s))   (inverts rt_bg_uv; the argument
 *     lies in [0, 2 pi], where rt_sincos_libm is verified). Only the direction is made: every pdf is evaluated from it afterwards.
 *   Mixture: with a distribution, shade()'s mix_dist (raytracer.h:381-407) gains the environment as one more equally weighted component, the
 *     last: {cosine, env} (k = 2) without emissive triangles, {cosine, lights, env} (k = 3) with them. pick = rng.below(k) where the reference
 *     draws its pick (a scene without lights draws none today and draws one now); the env sampler then makes its four draws;
 *     MIS_p = (sum of the k component pdfs) / (float)k. The alpha and technique coins keep their order; the VNDF branch and VNDF_FACTOR are untouched.
 *   Without a distribution only the miss branch changes: the random stream of every path is the one it has today.
 * Who sees it: every wavefront entry point (rt_render*, rt_render_views*, rt_render_rays*, rt_render_sensors*, rt_accum_*) through the one
 *   shade(); rt_bg_at returns the float lookup. rt_update_geometry* leaves the environment untouched. bg_color is the creation descriptor's.
 *   rt_set_environment(scene, NULL): back to what rt_create made of bg_texture; every entry point gives the bits it gave before.
 * RT_ERR_INVALID_ARG: a NULL scene; width outside 1..8192 or height outside 1..4096; NULL rgb; a texel that is NaN, infinite or negative; a bit
 *   of flags other than RT_ENV_IMPORTANCE; reserved != 0; a scene with a live accumulator (its sums are of the old environment: destroy it
 *   first; an accumulator created afterwards sees the new one). RT_ERR_UNSUPPORTED: a multi-GPU scene. After any refusal the scene is unchanged.
 * On a scene with a float environment RT_FLAG_MEGAKERNEL and RT_RNG_REFERENCE renders return RT_ERR_UNSUPPORTED (they are the reference's
 *   Scene::bg_at), as they do on a RT_BUILD_WIDE scene.
 * rt_env_pdf / rt_env_sample: probes of the distribution on the device's own tables: pdf(dir) for n directions (3 floats each, used as
 *   given), and the direction of n quadruples x0 .. x3. RT_ERR_INVALID_ARG without a distribution (no float environment, no flag, an all-zero
 *   map), for a NULL argument with n > 0, and for a uniform outside [0, 1). */
enum { RT_ENV_IMPORTANCE = 1 }; /* rt_environment.flags */
typedef struct rt_environment {
    uint32_t width, height; /* 1 .. 8192 x 1 .. 4096 */
    const float *rgb;       /* width*height*3 linear radiance, row 0 = +y pole; finite, >= 0 (else RT_ERR_INVALID_ARG) */
    uint32_t flags;         /* RT_ENV_*; any other bit refused */
    uint32_t reserved;      /* 0 */
} rt_environment;
int rt_set_environment(rt_scene *scene, const rt_environment *env); /* NULL: back to what rt_create made of desc.bg_texture */
int rt_env_pdf(rt_scene *scene, const float *dirs, uint32_t n, float *pdf_out);    /* probe: solid-angle pdf of the env distribution */
int rt_env_sample(rt_scene *scene, const float *xi4, uint32_t n, float *dirs_out); /* probe: 4 uniforms in [0,1) per direction */

int rt_film_rgb8(rt_scene *scene, const float *rgb, size_t n_pixels, uint8_t *out_rgb8);

const char *rt_last_error(void);
uint32_t rt_abi_version(void);
/* First 16 hex digits of the sha256 over the device-side sources this library was built from (csrc/device_sources.txt): lets a
 * caller (bench.py, __graft_entry__.build) check that the binary it measures is the tree it describes. */
const char *rt_source_stamp(void);
int rt_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_ABI_H */
