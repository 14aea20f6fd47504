/*
 * dcrt.h -- C ABI of the MI355X-native wavefront path tracer.
 *
 * This is the drop-in boundary for the hot path of
 * YaoTiancheng/DirectComputeRayTracing: the `CWavefrontPathTracer` plug-in
 * (Source/PathTracer.h:6-26, Source/WavefrontPathTracer.cpp:70-1162) and the
 * scene buffers `CScene` flattens for it (Source/Scene.cpp:273-608).
 *
 * Conventions (every entry point):
 *   - plain C types, pointers and sizes; no C++ or torch types cross the ABI;
 *   - return int status: 0 = ok, negative = error (see DCRT_E_*); nothing throws;
 *   - one tracer handle per HIP device; calls on a handle are serialised by the caller;
 *   - all GPU work of a tracer is ordered on the stream passed to dcrt_tracer_create
 *     (NULL = the tracer's own non-blocking stream).
 *
 * Wire format: the structs below reproduce the reference's GPU layouts byte for
 * byte (Appendix B of SURVEY.md): Vertex 44 B, BVHNode 32 B, Material 52 B,
 * SLight 28 B, float4x3 48 B (HLSL column-major), so a maintainer can hand the
 * reference's CScene arrays straight through.
 */
#ifndef DCRT_H_
#define DCRT_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCRT_API __attribute__((visibility("default")))

/* ---- status codes ---------------------------------------------------- */
#define DCRT_OK              0
#define DCRT_E_INVALID_ARG  -1
#define DCRT_E_HIP          -2   /* a HIP runtime call failed               */
#define DCRT_E_NO_SCENE     -3   /* render before dcrt_tracer_upload_scene   */
#define DCRT_E_IO           -4   /* file could not be read / parsed         */
#define DCRT_E_LIMIT        -5   /* a reference limit was exceeded          */
#define DCRT_E_NO_DEVICE    -6   /* no HIP device visible                   */

/* ---- constants shared with the reference shaders ----------------------- */
/* Shaders/LightSharedDef.inc.hlsl:6-12 */
#define DCRT_LIGHT_INDEX_INVALID        0xFFFFFFFFu
#define DCRT_LIGHT_FLAGS_POINT_LIGHT        0x1u
#define DCRT_LIGHT_FLAGS_MESH_LIGHT         0x2u
#define DCRT_LIGHT_FLAGS_DIRECTIONAL_LIGHT  0x4u
#define DCRT_LIGHT_FLAGS_ENVIRONMENT_LIGHT  0x8u
/* Shaders/Material.inc.hlsl:6-19 */
#define DCRT_MATERIAL_FLAG_ROUGHNESS_TEXTURE 0x20u
#define DCRT_MATERIAL_FLAG_IS_TWOSIDED       0x40u
#define DCRT_MATERIAL_FLAG_MULTISCATTERING   0x80u
#define DCRT_MATERIAL_FLAG_INTERNAL_SCATTERING_SHIFT 8
#define DCRT_MATERIAL_FLAG_INTERNAL_SCATTERING_MASK  0x300u
#define DCRT_MATERIAL_FLAG_TYPE_MASK         0xFu
#define DCRT_MATERIAL_TYPE_DIFFUSE          0
#define DCRT_MATERIAL_TYPE_PLASTIC          1
#define DCRT_MATERIAL_TYPE_CONDUCTOR        2
#define DCRT_MATERIAL_TYPE_DIELECTRIC       3
#define DCRT_MATERIAL_TYPE_THIN_DIELECTRIC  4
/* Shaders/InternalScatteringMode.inc.hlsl:4-6 */
#define DCRT_INTERNAL_SCATTERING_IGNORE   0
#define DCRT_INTERNAL_SCATTERING_SINGLE   1
#define DCRT_INTERNAL_SCATTERING_MULTIPLE 2
/* Shaders/InstanceSharedDef.inc.hlsl:4-5 */
#define DCRT_INSTANCE_FLAG_OPAQUE             0x1u
#define DCRT_INSTANCE_MATERIAL_OVERRIDE_NONE  0xFFFFFFFFu
/* Shaders/BVHSharedDef.inc.hlsl:4 */
#define DCRT_BVHNODE_MISC_MASK_PRIMITIVE_COUNT 0x1FFFFFFFu
/* Scene.h:108-109 */
#define DCRT_MAX_RAY_BOUNCE   20
#define DCRT_MAX_LIGHT_COUNT  5000
/* Shaders/BxDFTextureDef.inc.hlsl:4-9 */
#define DCRT_BXDFTEX_BRDF_SIZE_X 32
#define DCRT_BXDFTEX_BRDF_SIZE_Y 32
#define DCRT_BXDFTEX_BRDF_DIELECTRIC_SIZE_X 32
#define DCRT_BXDFTEX_BRDF_DIELECTRIC_SIZE_Y 16
#define DCRT_BXDFTEX_BRDF_DIELECTRIC_SIZE_Z 16

/* ---- feature variants (WavefrontPathTracer.cpp:554-590 shader defines) -- */
#define DCRT_FEATURE_GGX_SAMPLE_VNDF          0x01u  /* GGX_SAMPLE_VNDF (default on)            */
#define DCRT_FEATURE_NO_FRONT_TO_BACK         0x02u  /* BVH_NO_FRONT_TO_BACK_TRAVERSAL (off)    */
#define DCRT_FEATURE_LIGHT_VISIBLE            0x04u  /* LIGHT_VISIBLE (default on)              */
#define DCRT_FEATURE_WATERTIGHT               0x08u  /* WATERTIGHT_RAY_TRIANGLE_INTERSECTION(on)*/
#define DCRT_FEATURE_ALLOW_ANYHIT             0x10u  /* ALLOW_ANYHIT_SHADER (off): opacity test on
                                                        non-opaque instances (HitShader.inc.hlsl:86-113) */
#define DCRT_FEATURE_DEFAULT (DCRT_FEATURE_GGX_SAMPLE_VNDF | DCRT_FEATURE_LIGHT_VISIBLE | DCRT_FEATURE_WATERTIGHT)

/* ---- Appendix-B layouts ------------------------------------------------ */
/* Shaders/Vertex.inc.hlsl:8-14 -- 44 bytes */
typedef struct dcrt_vertex {
    float position[3];
    float normal[3];
    float tangent[3];
    float texcoord[2];
} dcrt_vertex;

/* Shaders/BVHNode.inc.hlsl:8-14 -- 32 bytes.
 * misc = primCount(or TLAS-leaf instance index) << 3 | (TLAS leaf ? 4 : 0) | split axis */
typedef struct dcrt_bvh_node {
    float bbox_min[3];
    float bbox_max[3];
    uint32_t right_child_or_prim_index;
    uint32_t misc;
} dcrt_bvh_node;

/* Shaders/Material.inc.hlsl:23-33 -- 52 bytes */
typedef struct dcrt_material {
    float albedo[3];
    int32_t albedo_texture_index;
    float ior[3];
    float roughness;
    float tex_tiling[2];
    float opacity;
    uint32_t flags;
    int32_t opacity_texture_index;
} dcrt_material;

/* Shaders/LightSharedDef.inc.hlsl:15-20 -- 28 bytes. For mesh lights the
 * second float3 holds (triangle offset, triangle count, instance) as uint bits. */
typedef struct dcrt_light {
    float radiance[3];
    float position_or_triangle_range[3];
    uint32_t flags;
} dcrt_light;

/* HLSL `float4x3` in a StructuredBuffer, column-major: m[c*4 + r] = M[r][c],
 * row-vector convention p' = mul(float4(p,1), M) (Scene.cpp:431-444). 48 bytes. */
typedef struct dcrt_float4x3 {
    float m[12];
} dcrt_float4x3;

/* Bindless scene texture (Texture2D<float4> g_Textures[], Scene.cpp:586-608). */
#define DCRT_TEXTURE_FORMAT_RGBA8_SRGB 0   /* DXGI_FORMAT_R8G8B8A8_UNORM_SRGB */
#define DCRT_TEXTURE_FORMAT_R8_UNORM   1   /* DXGI_FORMAT_R8_UNORM            */
typedef struct dcrt_texture {
    uint32_t width;
    uint32_t height;
    uint32_t format;            /* DCRT_TEXTURE_FORMAT_*            */
    const uint8_t* pixels;      /* tightly packed rows              */
} dcrt_texture;

/* The flattened scene: exactly what Scene.cpp:273-608 uploads. Host pointers. */
typedef struct dcrt_flat_scene {
    const dcrt_vertex* vertices;            uint32_t vertex_count;
    const uint32_t* triangles;              uint32_t triangle_count;   /* 3 indices / triangle */
    const dcrt_bvh_node* bvh_nodes;         uint32_t bvh_node_count;   /* TLAS first, then BLASes */
    uint32_t tlas_node_count;
    const uint32_t* material_ids;                                       /* one per triangle */
    const dcrt_float4x3* instance_transforms; uint32_t instance_count;  /* 2N: forward, inverse */
    const uint32_t* instance_light_indices;                             /* N */
    const uint32_t* instance_flags;                                     /* N */
    const uint32_t* instance_material_overrides;                        /* N */
    const dcrt_material* materials;         uint32_t material_count;
    const dcrt_light* lights;               uint32_t light_count;       /* mesh, env, punctual */
    uint32_t environment_light_index;       /* #mesh lights, or DCRT_LIGHT_INDEX_INVALID */
    const dcrt_texture* textures;           uint32_t texture_count;
    /* Environment cube (TextureCube<float3>): 6 faces (+X,-X,+Y,-Y,+Z,-Z) of
     * size x size texels, RGB float, NULL when the scene has none. */
    const float* env_cube_rgb;              uint32_t env_cube_size;
    uint32_t bvh_traversal_stack_size;      /* CScene::m_BVHTraversalStackSize */
} dcrt_flat_scene;

/* The six R16_UNORM BxDF lookup tables (BxDFTexturesBuilding.cpp:171-175,265-270,379-384). Main
 * tables: the directional albedo at cos = max(x * 0.032258, 0.0001), alpha = y * step (0.032258
 * for brdf, 0.066667 for the arrays), ior = 1 + (slice % 16) * 0.133333; slices 0-15 see the
 * boundary from outside ("leaving"), 16-31 from the dense side ("entering"). Each *_avg texel is
 * the cosine-weighted average of one row of its main table by the trapezoid rule over the 32
 * columns, 2 / 31 * (f(0) * 0.0001 / 2 + sum_{i=1..30} f(i) * (i * 0.032258) + f(31) / 2), taken
 * on the float table before it is clamped; row (slice, alpha) goes to [slice / 16][slice % 16][alpha]. */
#define DCRT_LUT_BRDF_COUNT            (32 * 32)
#define DCRT_LUT_BRDF_AVG_COUNT        (32)
#define DCRT_LUT_BRDF_DIELECTRIC_COUNT (32 * 16 * 32)
#define DCRT_LUT_BRDF_DIELECTRIC_AVG_COUNT (16 * 16 * 2)
#define DCRT_LUT_BSDF_COUNT            (32 * 16 * 32)
#define DCRT_LUT_BSDF_AVG_COUNT        (16 * 16 * 2)
typedef struct dcrt_bxdf_luts {
    uint16_t brdf[DCRT_LUT_BRDF_COUNT];                         /* [alpha 32][cos 32]            */
    uint16_t brdf_avg[DCRT_LUT_BRDF_AVG_COUNT];                 /* [alpha 32]                    */
    uint16_t brdf_dielectric[DCRT_LUT_BRDF_DIELECTRIC_COUNT];   /* [slice 32][alpha 16][cos 32]  */
    uint16_t brdf_dielectric_avg[DCRT_LUT_BRDF_DIELECTRIC_AVG_COUNT]; /* [slice 2][ior 16][alpha 16] */
    uint16_t bsdf[DCRT_LUT_BSDF_COUNT];                         /* [slice 32][alpha 16][cos 32]  */
    uint16_t bsdf_avg[DCRT_LUT_BSDF_AVG_COUNT];                 /* [slice 2][ior 16][alpha 16]   */
} dcrt_bxdf_luts;

/* Union of SControlConstants / SNewPathConstants / SMaterialConstants
 * (WavefrontPathTracer.cpp:34-63,372-428). */
typedef struct dcrt_frame_params {
    float camera_transform[16];   /* row-major float4x4, translation in row 3 (Camera.cpp:87-96) */
    uint32_t resolution[2];       /* current film width, height                   */
    float film_size[2];
    float aperture_radius;        /* CalculateApertureDiameter() * 0.5            */
    float focal_distance;
    float film_distance;          /* CalculateFilmDistance()                      */
    uint32_t blade_count;
    float blade_vertex_pos[2];    /* cos/sin(pi / blades) * aperture radius       */
    float aperture_base_angle;
    uint32_t frame_seed;
    uint32_t max_bounce_count;
    uint32_t light_count;
    uint32_t environment_light_index;
    uint32_t features;            /* DCRT_FEATURE_* */
} dcrt_frame_params;

/* Film reconstruction (Scene.h:131-136, SampleConvolution.cpp:100-130).
   Every entry point that takes a dcrt_filter_params answers DCRT_E_INVALID_ARG (with a
   dcrt_last_error text, the film and the device filter untouched) to a filter above
   DCRT_FILTER_LANCZOS and to a radius that is NaN, negative or >= 2^30 (the window bounds
   floor(c -/+ radius) must fit an int for every film coordinate). */
#define DCRT_FILTER_BOX      0
#define DCRT_FILTER_TRIANGLE 1
#define DCRT_FILTER_GAUSSIAN 2
#define DCRT_FILTER_MITCHELL 3
#define DCRT_FILTER_LANCZOS  4
typedef struct dcrt_filter_params {
    uint32_t filter;              /* DCRT_FILTER_* */
    float radius;
    float gaussian_alpha;
    float mitchell_b;
    float mitchell_c;
    uint32_t lanczos_tau;         /* 0 reads as 3, the reference's default (Scene.h:136) */
} dcrt_filter_params;

/* Ray / hit records of the kernel-level boundary (WavefrontPathTracing.hlsl:3-17). */
typedef struct dcrt_ray {
    float origin[3];
    float t_max;
    float direction[3];
    float t_min;
} dcrt_ray;                       /* 32 bytes, SRay */
typedef struct dcrt_ray_hit {
    float t;                      /* +inf on a miss                                   */
    float u, v;
    uint32_t triangle_id;         /* bit 31 = backface                                */
    uint32_t instance_index;
} dcrt_ray_hit;                   /* 20 bytes, SRayHit */

/* Tracer configuration (CWavefrontPathTracer::Create, WavefrontPathTracer.cpp:25-28). */
typedef struct dcrt_tracer_config {
    uint32_t path_pool_size;      /* slots; 0 = default (2^20 on MI355X)             */
    uint32_t iterations_per_render; /* m_IterationPerFrame; 0 = default              */
    int32_t device;               /* HIP device ordinal                               */
    void* stream;                 /* hipStream_t or NULL                              */
    uint32_t debug_rng;           /* nonzero: keep each pixel's terminal RNG state    */
} dcrt_tracer_config;

/* Counters since the last dcrt_tracer_reset_stats (or create). */
typedef struct dcrt_ray_stats {
    uint64_t extension_rays;      /* EXTENSION_RAY_CAST rays traced                   */
    uint64_t shadow_rays;         /* SHADOW_RAY_CAST rays traced                      */
    uint64_t new_paths;           /* paths started by the completed images (one per
                                     rendered pixel, halo rows included, per image)   */
    uint64_t iterations;          /* RenderOneIteration equivalents launched          */
    uint64_t images_completed;    /* images finished by render / render_images        */
    uint64_t early_finished;      /* paths finished at their last shaded bounce (dcrt_tracer_info.early_finish):
                                     each cast one more extension ray, counted above, that no pass shaded */
} dcrt_ray_stats;

/* Rows of the film a tracer renders and convolves (multi-GPU film tiling).
 * The H rows are cut into K = N * k stripes of floor/ceil(H / K) rows, k = round(H / (N *
 * stripe_height)) (at least 1); stripe j = rows [j*H/K, (j+1)*H/K) belongs to rank j % N.
 * A rank path-traces its rows plus halo_rows rows beyond each stripe edge and convolves
 * only its own rows, so the SUM of all ranks' films is the one-tracer film bit for bit. */
typedef struct dcrt_film_partition {
    uint32_t world_size;          /* N; 1 = whole film                                */
    uint32_t rank;
    uint32_t stripe_height;       /* target stripe height in rows                     */
    uint32_t halo_rows;           /* >= floor(filter radius + 0.5); 0 = 2             */
} dcrt_film_partition;

/* Traversal work counters of the extension / shadow casts
 * (SRayTraversalCounters semantics, SceneRayTrace.h:13-19): node visits =
 * iterationCounter (BVHAccel.inc.hlsl:121), triangle tests, BLAS entries. */
typedef struct dcrt_traversal_stats {
    uint64_t ext_node_visits, ext_triangle_tests, ext_blas_entries;
    uint64_t shadow_node_visits, shadow_triangle_tests, shadow_blas_entries;
    uint64_t ext_launches;
    double ext_kernel_ms;         /* summed HIP-event time of the timed EXTENSION_RAY_CAST launches */
    uint64_t ext_max_node_visits, shadow_max_node_visits;   /* the longest ray of each kind since
                                     the last reset (merged cast kernel, instrumented)      */
    uint64_t material_launches;   /* timed MATERIAL launches (ext_timing) and their summed   */
    double material_kernel_ms;    /* HIP-event time                                          */
    uint64_t control_launches;    /* timed CONTROL(+NEW_PATH) launches, likewise             */
    double control_kernel_ms;
} dcrt_traversal_stats;

/* What the tracer chose for the uploaded scene (diagnostics; bench.py reports it). */
typedef struct dcrt_tracer_info {
    uint32_t path_pool_size;      /* slots after rounding to whole CONTROL workgroups     */
    uint32_t scene_in_lds;        /* 1: the whole BVH + triangles sit in the cast kernel's
                                     LDS scene cache (the LDS-only cast variant)          */
    uint32_t cached_nodes, cached_triangles;   /* how much of the scene the LDS cache holds */
    uint32_t cast_block;          /* cast-kernel workgroup size                          */
    uint32_t traversal_stack;     /* LDS stack rows per lane                             */
    uint32_t material_generic;    /* 1: the any-scene MATERIAL variant                   */
    uint32_t pair_traversal;      /* 1: the cast kernel expands node pairs (scene beyond L2), over the device
                                     child-pair node order */
    uint32_t control_grid, material_grid;   /* CONTROL / MATERIAL workgroups per launch  */
    uint32_t cast_grid;           /* persistent cast-kernel workgroups (resident on the chip) */
    uint32_t material_lds;        /* bytes of MATERIAL's LDS scene copy (0: not used)      */
    uint32_t cast_identity;       /* 1: the cache-only cast kernel without instance space
                                     (every instance's inverse exactly the identity); 2: the
                                     same over the entry-free node order (no BLAS-entry step) */
    uint32_t stack_lds_rows;      /* LDS stack rows per lane of the launched cast kernel: traversal_stack + 2,
                                     or ring_rows                                          */
    uint32_t ring_rows;           /* 0, or the LDS window (rows) of a spilling traversal stack: deeper
                                     entries live in a per-lane global column              */
    uint32_t cast_waves_per_cu;   /* resident waves per CU of the launched cast kernel      */
    uint32_t shadow_cells;        /* 0, or R: the merged cast tests shadow rays against the point light's
                                     6 * R * R direction cells (dcrt_shadow_cells_build) instead of walking the BVH */
    uint32_t shadow_cell_max_leaves;   /* leaves in the fullest cell, and the mean over the cells */
    float shadow_cell_mean_leaves;
    uint32_t shadow_inline;       /* 1: MATERIAL tests the shadow rays against those cells itself, as the next launch
                                     stands (frame features, instrumentation): no shadow-queue record, no result word;
                                     0: they take the shadow queue to the cast (DCRT_FUSED_SHADOW=0, no table, any-hit,
                                     counters, the row-cost probe) */
    uint32_t shading_tables;      /* DCRT_SHADING_TABLES as it stands for the scene, one bit per piece of scene-constant
                                     shading work taken out of the per-hit path: 1: no BSDF pdf for a delta light's
                                     sample; 2: the plastic dielectric LUT read from per-material float rows; 4: the hit's frame
                                     from a per-triangle table */
    uint32_t dielectric_row_bytes;   /* bytes of those rows (528 per material; 0: none -- bit 2 off, no plastic
                                        material, or more than 64 materials) and how many of them sit in MATERIAL's LDS behind material_lds */
    uint32_t dielectric_row_lds;
    uint32_t frame_table_bytes;   /* 0, or the bytes (48 per triangle) of the per-triangle world-space frames -- normal,
                                     tangent, geometry normal -- that MATERIAL reads per hit instead of rebuilding them
                                     (bit 4 of shading_tables): scenes of the opaque, delta-lit MATERIAL variant whose every
                                     BLAS has one instance and whose whole shading data sits in MATERIAL's LDS */
    uint32_t early_finish;        /* DCRT_EARLY_FINISH as the next launch stands: 1 (2: even path slots only, a test
                                     value): MATERIAL finishes a path at its last shaded bounce -- its last ray is
                                     cast and counted, no pass shades its hit, its sample is the same bits; 0: off
                                     (the knob, a mesh or environment light, any-hit, the row-cost probe) */
} dcrt_tracer_info;

typedef struct dcrt_tracer dcrt_tracer;
typedef struct dcrt_scene dcrt_scene;

/* ===== version / device ================================================== */
/* ABI version of this header: bumped whenever a struct changes size or an entry point its
 * meaning (2: dcrt_tracer_info grew cast_waves_per_cu / ring_rows / stack_lds_rows; 3: it grew
 * shadow_cells / shadow_cell_max_leaves / shadow_cell_mean_leaves; 4: shadow_inline; 5: shading_tables /
 * dielectric_row_bytes / dielectric_row_lds / frame_table_bytes; 6: early_finish, and dcrt_ray_stats grew
 * early_finished). A caller
 * compiled against another header checks dcrt_abi_version() == DCRT_ABI_VERSION before it
 * passes any struct (a smaller dcrt_tracer_info would be written past its end). Added entry
 * points with structs of their own (the scene updates, the output views, the film denoiser)
 * leave it as it is: nothing an older caller passes has changed. */
#define DCRT_ABI_VERSION 6
DCRT_API int dcrt_abi_version(void);
DCRT_API const char* dcrt_version(void);
DCRT_API const char* dcrt_last_error(void);
DCRT_API int dcrt_device_count(int* out_count);

/* ===== host scene: CScene + loaders + BVHAccel (Scene.cpp, BVHAccel.cpp) ==== */
DCRT_API int dcrt_scene_create(dcrt_scene** out_scene);
DCRT_API void dcrt_scene_destroy(dcrt_scene* scene);
/* CScene::Reset (Scene.cpp:626-660): resolution, camera defaults, clears content. */
DCRT_API int dcrt_scene_reset(dcrt_scene* scene, uint32_t resolution_width, uint32_t resolution_height);
/* CScene::LoadFromFile (Scene.cpp:103-624): .obj (WavefrontOBJLoading.cpp) or .xml (SceneXMLLoading.cpp). */
DCRT_API int dcrt_scene_load_from_file(dcrt_scene* scene, const char* path);
/* Equivalent of UI "Create -> Point/Directional Light" (ImGui.cpp:322-331). */
DCRT_API int dcrt_scene_add_punctual_light(dcrt_scene* scene, const float position[3], const float euler_angles[3],
                                           const float color[3], int is_directional);
/* Edit / delete punctual light `index` (ImGui.cpp:351-372, 468-497); the lights after a
 * removed one keep their order. DCRT_E_INVALID_ARG for an index out of range. */
DCRT_API int dcrt_scene_set_punctual_light(dcrt_scene* scene, uint32_t index, const float position[3],
                                           const float euler_angles[3], const float color[3], int is_directional);
DCRT_API int dcrt_scene_remove_punctual_light(dcrt_scene* scene, uint32_t index);
/* Delete the environment light (ImGui.cpp:360-366); DCRT_E_INVALID_ARG without one. */
DCRT_API int dcrt_scene_remove_environment_light(dcrt_scene* scene);
/* What the edits since the last dcrt_scene_acquire_dirty changed (Scene.h:211-215, Camera.h:14).
 * An edit re-flattens only its own arrays (dcrt_scene_get_flat's materials / lights /
 * instance_flags; no vertex, triangle, node or transform is copied), and the tracer takes them
 * through dcrt_tracer_update_materials / _lights / _instance_flags. DCRT_DIRTY_SCENE asks for a
 * full dcrt_tracer_upload_scene: set by load and reset, and whenever an environment cube
 * appears, disappears or changes (the reference calls OnSceneLoaded then, ImGui.cpp:360-366,
 * 520-538). DCRT_DIRTY_CAMERA: new frame parameters (camera / lens). Every bit also means the
 * image restarts (LaunchRendererLoop.cpp:203-204). */
#define DCRT_DIRTY_LIGHTS          0x01u   /* punctual-light edits, environment colour        */
#define DCRT_DIRTY_MATERIALS       0x02u   /* material fields, multiscattering, opacity       */
#define DCRT_DIRTY_INSTANCE_FLAGS  0x04u   /* opacity / opacity texture (with MATERIALS)      */
#define DCRT_DIRTY_CAMERA          0x08u   /* dcrt_scene_set_camera / _set_lens               */
#define DCRT_DIRTY_SCENE           0x10u
/* Returns the bits and clears them. */
DCRT_API int dcrt_scene_acquire_dirty(dcrt_scene* scene, uint32_t* out_bits);
/* Rebuild every flat array (what each edit did before the partial paths; the full-reload
 * side of tools/bench_scene_update.py and of the tests' byte comparison); DCRT_E_NO_SCENE
 * before any content is loaded. */
DCRT_API int dcrt_scene_flatten(dcrt_scene* scene);
/* Constant environment light (SceneXMLLoading.cpp:1454-1467); cube may be NULL. */
DCRT_API int dcrt_scene_set_environment_light(dcrt_scene* scene, const float color[3],
                                              const float* cube_rgb, uint32_t cube_size);
DCRT_API int dcrt_scene_set_camera(dcrt_scene* scene, const float position[3], const float euler_angles[3]);
/* Camera / film parameters (Scene.h:118-137): camera_type 0 = pinhole, 1 = thin lens. */
DCRT_API int dcrt_scene_set_lens(dcrt_scene* scene, int camera_type, float fov_x, float focal_length,
                                 float focal_distance, float relative_aperture, uint32_t blade_count,
                                 float aperture_rotation, const float film_size[2]);
DCRT_API int dcrt_scene_set_max_bounce(dcrt_scene* scene, uint32_t max_bounce);
DCRT_API int dcrt_scene_set_filter(dcrt_scene* scene, const dcrt_filter_params* filter);
DCRT_API int dcrt_scene_get_filter(const dcrt_scene* scene, dcrt_filter_params* out_filter);
DCRT_API int dcrt_scene_get_resolution(const dcrt_scene* scene, uint32_t* width, uint32_t* height);
/* Edit material i (UI material editing, ImGui.cpp:560-660). */
DCRT_API int dcrt_scene_get_material_count(const dcrt_scene* scene, uint32_t* out_count);
DCRT_API int dcrt_scene_set_material(dcrt_scene* scene, uint32_t index, int material_type, const float albedo[3],
                                     float roughness, const float ior[3], const float k[3],
                                     int multiscattering, int two_sided);
/* SMaterial as the scene holds it before UpdateMaterialGPUData translates it
 * (Material.h:14-30, Scene.cpp:742-774): the oracle's own flattening reads this. */
typedef struct dcrt_material_setting {
    float albedo[3];
    float roughness;
    float ior[3];
    float opacity;
    float k[3];
    float tiling[2];
    uint32_t material_type;               /* DCRT_MATERIAL_TYPE_* */
    int32_t albedo_texture_index;         /* -1 = INDEX_NONE */
    int32_t opacity_texture_index;
    uint32_t internal_scattering_mode;    /* DCRT_INTERNAL_SCATTERING_* */
    uint32_t multiscattering;             /* m_Multiscattering */
    uint32_t is_two_sided;
    uint32_t has_roughness_texture;
} dcrt_material_setting;
DCRT_API int dcrt_scene_get_material_setting(const dcrt_scene* scene, uint32_t index, dcrt_material_setting* out_setting);
/* The UI's "Multiscattering" checkbox (ImGui.cpp:620-626): only plastic, conductor and
 * dielectric materials have it (DCRT_E_INVALID_ARG for diffuse / thin dielectric). Both
 * loaders force the flag off (SceneXMLLoading.cpp:869, WavefrontOBJLoading.cpp:318). */
DCRT_API int dcrt_scene_set_material_multiscattering(dcrt_scene* scene, uint32_t index, int enable);
/* Material opacity and opacity texture (ImGui.cpp:630-650, SMaterial::m_Opacity /
 * m_OpacityTextureIndex); texture index -1 = none. Recomputes the instance OPAQUE flags
 * (Scene.cpp:57-80, 785-800). */
DCRT_API int dcrt_scene_set_material_opacity(dcrt_scene* scene, uint32_t index, float opacity,
                                             int32_t opacity_texture_index);
/* Shader feature toggles of the scene (Scene.h:140-146: m_IsGGXVNDFSamplingEnabled,
 * m_TraverseBVHFrontToBack, m_IsLightVisible, m_WatertightRayTriangleIntersection,
 * m_AllowAnyHitShader) as DCRT_FEATURE_* bits; get_frame_params reports them. */
DCRT_API int dcrt_scene_set_features(dcrt_scene* scene, uint32_t features);
DCRT_API int dcrt_scene_get_features(const dcrt_scene* scene, uint32_t* out_features);
/* Flattened buffers; pointers stay valid until the scene is modified or destroyed. */
DCRT_API int dcrt_scene_get_flat(dcrt_scene* scene, dcrt_flat_scene* out_flat);
/* The frame constants Render() would upload (WavefrontPathTracer.cpp:372-428). */
DCRT_API int dcrt_scene_get_frame_params(const dcrt_scene* scene, uint32_t frame_seed, dcrt_frame_params* out_params);
/* BVH statistics: node counts and depth (Scene.cpp:169-207). */
DCRT_API int dcrt_scene_get_bvh_info(const dcrt_scene* scene, uint32_t* tlas_nodes, uint32_t* total_nodes,
                                     uint32_t* max_stack_size);

/* The scene content as loaded, before BVHAccel reordered it -- the inputs of
 * Mesh::BuildBVH / BuildTLAS (Mesh.cpp:59-79, Scene.cpp:160-215): mesh i's vertices,
 * triangles (mesh-local vertex indices) and material ids in load order; instance j's
 * mesh index and XMFLOAT4X3 transform (4 rows of 3) in load order. Each mesh's pointers
 * stay valid until the scene is reset, loads more content or is destroyed. Used to check the BVH build against an independent one. */
typedef struct dcrt_obj_mesh dcrt_obj_mesh;
DCRT_API int dcrt_scene_get_content_counts(const dcrt_scene* scene, uint32_t* out_meshes, uint32_t* out_instances);
DCRT_API int dcrt_scene_get_loaded_mesh(dcrt_scene* scene, uint32_t mesh, dcrt_obj_mesh* out_mesh);
DCRT_API int dcrt_scene_get_instance(const dcrt_scene* scene, uint32_t instance, uint32_t* out_mesh_index,
                                     float out_transform[12]);

/* The rest of CScene's state before UpdateLight/Material/InstanceFlagsGPUData and
 * Render() flatten it (Scene.h:118-160, Camera.h, Scene.cpp:570-584, 672-807,
 * WavefrontPathTracer.cpp:372-428): what the oracle's own flattening is driven from. */
typedef struct dcrt_scene_settings {
    uint32_t resolution[2];
    uint32_t max_bounce_count;
    uint32_t camera_type;                 /* 0 = pinhole, 1 = thin lens */
    float fov_x, focal_length, focal_distance, relative_aperture;
    uint32_t aperture_blade_count;
    float aperture_rotation;
    float film_size[2];
    float camera_position[3];             /* CCamera::m_Position */
    float camera_euler_angles[3];         /* CCamera::m_EulerAngles (pitch, yaw, roll) */
    uint32_t features;                    /* DCRT_FEATURE_* */
    uint32_t has_environment_light;
    float environment_color[3];           /* SEnvironmentLight::m_Color */
    const float* env_cube_rgb;            /* the environment texture (NULL = none) */
    uint32_t env_cube_size;
    uint32_t mesh_light_count, punctual_light_count, material_count, texture_count;
} dcrt_scene_settings;
DCRT_API int dcrt_scene_get_settings(const dcrt_scene* scene, dcrt_scene_settings* out_settings);
/* SMeshLight i (Scene.h:42-46): the instance it lights (load order) and its radiance. */
DCRT_API int dcrt_scene_get_mesh_light(const dcrt_scene* scene, uint32_t index, uint32_t* out_instance,
                                       float out_color[3]);
/* SPunctualLight i (Scene.h:27-40). */
DCRT_API int dcrt_scene_get_punctual_light(const dcrt_scene* scene, uint32_t index, float out_position[3],
                                           float out_euler_angles[3], float out_color[3], int* out_is_directional);
/* SMeshInstance::m_MaterialIdOverride of instance j (load order; 0xFFFFFFFF = none). */
DCRT_API int dcrt_scene_get_instance_material_override(const dcrt_scene* scene, uint32_t instance,
                                                       uint32_t* out_override);

/* Standalone BVHAccel::BuildBLAS + PackBVH over one triangle soup
 * (BVHAccel.cpp:376-447). out_nodes holds 2*triangle_count-1 entries at most;
 * out_reordered_indices 3*triangle_count; out_reordered_triangles triangle_count. */
DCRT_API int dcrt_bvh_build_blas(const dcrt_vertex* vertices, const uint32_t* indices, uint32_t triangle_count,
                                 dcrt_bvh_node* out_nodes, uint32_t* out_node_count,
                                 uint32_t* out_reordered_indices, uint32_t* out_reordered_triangles,
                                 uint32_t* out_max_depth, uint32_t* out_max_stack_size);

/* OBJ loading into meshes, before any BVH build:
 *  - DCRT_OBJ_SCENE_LAYOUT: the meshes CScene::LoadFromWavefrontOBJFile builds
 *    (WavefrontOBJLoading.cpp:409-465): one mesh per OBJ shape, RH->LH transform
 *    (x negated), winding change, V flip, material ids offset by material_index_base;
 *  - 0: Mesh::LoadFromWavefrontOBJFile as the XML loader calls it
 *    (SceneXMLLoading.cpp:1334-1341): every shape into one mesh, no transform.
 * Vertices carry the MikkTSpace tangents (WavefrontOBJLoading.cpp:147-153). */
#define DCRT_OBJ_SCENE_LAYOUT 1u
typedef struct dcrt_obj_meshes dcrt_obj_meshes;
struct dcrt_obj_mesh {
    const dcrt_vertex* vertices;
    uint32_t vertex_count;
    const uint32_t* indices;          /* 3 per triangle                         */
    const uint32_t* material_ids;     /* 1 per triangle (0xFFFFFFFF = none)      */
    uint32_t triangle_count;
};
/* The translated OBJ materials (WavefrontOBJLoading.cpp:305-338) of a load. */
typedef struct dcrt_obj_material {
    float albedo[3], ior, roughness, opacity;
    int32_t albedo_texture_index, opacity_texture_index;
} dcrt_obj_material;
DCRT_API int dcrt_obj_load(const char* path, uint32_t flags, uint32_t material_index_base, dcrt_obj_meshes** out);
DCRT_API int dcrt_obj_mesh_count(const dcrt_obj_meshes* meshes, uint32_t* out_count);
DCRT_API int dcrt_obj_get_mesh(const dcrt_obj_meshes* meshes, uint32_t index, dcrt_obj_mesh* out_mesh);
DCRT_API int dcrt_obj_material_count(const dcrt_obj_meshes* meshes, uint32_t* out_count);
DCRT_API int dcrt_obj_get_material(const dcrt_obj_meshes* meshes, uint32_t index, dcrt_obj_material* out_material);
DCRT_API void dcrt_obj_free(dcrt_obj_meshes* meshes);
/* The element / attribute tree the Mitsuba XML loader parses from `path` (what
 * SceneXMLLoading.cpp's walk over rapidxml's DOM reads, :247-581): per element in document
 * order "E<name>\n", "A<name>=<value>\n" per attribute, its children, "/\n". Writes at most
 * `capacity` bytes; *out_length = the full length (DCRT_E_LIMIT if it did not fit). */
DCRT_API int dcrt_xml_dump_tree(const char* path, char* out, uint32_t capacity, uint32_t* out_length);

/* ===== tracer: CWavefrontPathTracer on MI355X ============================== */
DCRT_API int dcrt_tracer_create(const dcrt_tracer_config* config, dcrt_tracer** out_tracer);  /* Create()  */
DCRT_API void dcrt_tracer_destroy(dcrt_tracer* tracer);                                        /* Destroy() */
/* OnSceneLoaded + the uploads of Scene.cpp:273-608. Copies everything to HBM. */
DCRT_API int dcrt_tracer_upload_scene(dcrt_tracer* tracer, const dcrt_flat_scene* scene);
/* Partial updates of the uploaded scene (CScene::UpdateMaterial / Light / InstanceFlagsGPUData,
 * Scene.cpp:672-807): only the named array goes to the device -- no geometry, no node
 * re-layout. DCRT_E_NO_SCENE before a scene is uploaded; material_count / instance_count must
 * equal the uploaded scene's (DCRT_E_INVALID_ARG); light_count may differ, 0 ..
 * DCRT_MAX_LIGHT_COUNT (DCRT_E_LIMIT above). Each call is ordered after the work already
 * enqueued on the tracer's stream and has copied the array on return. What the tracer derives
 * from materials and lights (the MATERIAL / drain variant, MATERIAL's LDS scene copy) follows;
 * captured graphs are dropped only when something baked into them changed, so a content-only
 * edit (a colour, a roughness, a moved light) keeps them. The film, the path state and the
 * environment cube are untouched: the caller restarts the image (dcrt_tracer_reset_image) and
 * sends frame parameters with the new light count, as the reference's frame loop does. */
DCRT_API int dcrt_tracer_update_materials(dcrt_tracer* tracer, const dcrt_material* materials, uint32_t material_count);
DCRT_API int dcrt_tracer_update_lights(dcrt_tracer* tracer, const dcrt_light* lights, uint32_t light_count);
DCRT_API int dcrt_tracer_update_instance_flags(dcrt_tracer* tracer, const uint32_t* flags, uint32_t instance_count);
/* Upload counters since dcrt_tracer_create. */
typedef struct dcrt_upload_stats {
    uint64_t scene_uploads, material_updates, light_updates, instance_flag_updates;
    uint64_t geometry_bytes;       /* H2D bytes of vertices, triangles, nodes, transforms, textures, cube */
    uint64_t shading_bytes;        /* H2D bytes of materials, lights, instance flags */
    uint64_t graph_invalidations;  /* times captured graphs were dropped */
} dcrt_upload_stats;
DCRT_API int dcrt_tracer_upload_stats(dcrt_tracer* tracer, dcrt_upload_stats* out_stats);
/* While a scene is uploaded, the render entry points refuse (DCRT_E_INVALID_ARG) frame
 * parameters whose light_count exceeds the lights the tracer holds. */
DCRT_API int dcrt_tracer_set_frame_params(dcrt_tracer* tracer, const dcrt_frame_params* params);
DCRT_API int dcrt_tracer_set_film_partition(dcrt_tracer* tracer, const dcrt_film_partition* partition);
/* Explicit film bands (cost-balanced film tiling): the tracer owns the rows of the
 * band_count ranges [bands[2i], bands[2i+1]) (ascending, disjoint, non-empty; rows past the film
 * are ignored), path-traces them plus halo_rows rows beyond each band (0 = 2) and convolves only
 * its own rows, so any cut of the film dealt to tracers sums to the one-tracer film bit for bit.
 * Replaces a dcrt_film_partition (and a later dcrt_tracer_set_film_partition replaces the bands). */
DCRT_API int dcrt_tracer_set_film_bands(dcrt_tracer* tracer, const uint32_t* bands, uint32_t band_count, uint32_t halo_rows);
/* Row-cost probe: enable != 0 clears and starts per-film-row counters of the rays the wavefront
 * casts (each MATERIAL pass adds its item's extension ray and, if it casts one, its shadow ray);
 * the counts are exact and schedule-independent. 0 stops them. Not a reference entry point: the
 * input of cost-balanced bands (directcomputeraytracing_amd/partition.py balanced_bands). */
DCRT_API int dcrt_tracer_set_row_cost_probe(dcrt_tracer* tracer, int enable);
DCRT_API int dcrt_tracer_read_row_cost(dcrt_tracer* tracer, uint32_t* out_rays_per_row);   /* film height entries */
/* Render(): run up to max_iterations wavefront iterations (0 = config value). */
DCRT_API int dcrt_tracer_render(dcrt_tracer* tracer, uint32_t max_iterations);
/* Render whole images: image s uses frame seed first_seed + s. Images are path-traced in
 * batches that share the path pool (new paths of the next image start as soon as slots
 * are idle); a completed batch is convolved into the film (SampleConvolution) image by
 * image, in order, so the film is the same as with one image at a time. */
DCRT_API int dcrt_tracer_render_images(dcrt_tracer* tracer, uint32_t first_seed, uint32_t image_count,
                                       const dcrt_filter_params* filter);
/* render_images generalised for pipelines that share a film's rows by interleaving images:
 * image k of the call has frame seed first_seed + k * seed_stride; with convolve == 0 the film
 * pass is skipped and image k's samples stay in slot k (at most 256 images, one batch) for
 * dcrt_tracer_image_sample_ptrs / dcrt_tracer_accumulate_images. No reference counterpart. */
DCRT_API int dcrt_tracer_render_images_strided(dcrt_tracer* tracer, uint32_t first_seed, uint32_t seed_stride,
                                               uint32_t image_count, int convolve, const dcrt_filter_params* filter);
/* Device pointers of image `image`'s sample textures (W*H R32G32F / RGBA32F) after a
 * render_images_strided call with convolve == 0. */
DCRT_API int dcrt_tracer_image_sample_ptrs(dcrt_tracer* tracer, uint32_t image, void** out_position, void** out_value);
/* SampleConvolution over image_count images whose sample textures sit at the given device
 * pointers (host arrays of image_count pointers each; every texture W*H of this tracer's film,
 * on its device), convolved in list order into this tracer's film (its own rows): the film of
 * several pipelines' interleaved images, bit for bit the one-pipeline film when the list is in
 * image order. Synchronous. */
DCRT_API int dcrt_tracer_accumulate_images(dcrt_tracer* tracer, const void* const* d_positions, const void* const* d_values,
                                           uint32_t image_count, const dcrt_filter_params* filter);
/* Allocate / capture now what dcrt_tracer_render_images(image_count) would on its first
 * call (the batch's sample textures, the iteration graph), e.g. before a timed region.
 * No reference counterpart (the reference allocates at Create and scene load). */
DCRT_API int dcrt_tracer_prepare_images(dcrt_tracer* tracer, uint32_t image_count);
/* Images per render_images batch (0 = automatic: as many as the path pool holds, at most
 * 64, the images cut into equal batches). */
DCRT_API int dcrt_tracer_set_image_batch(dcrt_tracer* tracer, uint32_t images);
/* 0 = wavefront (CWavefrontPathTracer, default), 1 = megakernel (CMegakernelPathTracer,
 * MegakernelPathTracing.hlsl) for dcrt_tracer_render_images. */
DCRT_API int dcrt_tracer_set_mode(dcrt_tracer* tracer, int mode);
/* The megakernel tracer's "Output" views (MegakernelPathTracer.cpp:208-212 s_OutputNames, in
 * that order; MegakernelPathTracing.hlsl:212-291): anything but PATH_TRACING renders the
 * camera ray's first hit only -- the shading normal or tangent as n * 0.5 + 0.5, the albedo,
 * green / red for a shading normal facing away from / towards the ray (Negative NdotV) or a
 * back- / front-face hit, black for a miss; ITERATION_COUNT is the ray's BVH node visits over
 * iteration_threshold as a grey level, red above the threshold, hit or miss. */
#define DCRT_OUTPUT_PATH_TRACING 0
#define DCRT_OUTPUT_SHADING_NORMAL 1
#define DCRT_OUTPUT_SHADING_TANGENT 2
#define DCRT_OUTPUT_ALBEDO 3
#define DCRT_OUTPUT_NEGATIVE_NDOTV 4
#define DCRT_OUTPUT_BACKFACE 5
#define DCRT_OUTPUT_ITERATION_COUNT 6
typedef struct dcrt_output_params {
    uint32_t output_type;          /* DCRT_OUTPUT_* (m_OutputType, default PATH_TRACING)            */
    uint32_t iteration_threshold;  /* m_IterationThreshold (default 20); 1..10000 for ITERATION_COUNT */
} dcrt_output_params;
/* Select the view. With a view selected, whatever dcrt_tracer_set_mode says,
 * dcrt_tracer_render_images renders one view image per seed (first-hit kernel + SampleConvolution,
 * every image convolved) and dcrt_tracer_render renders the whole view image of the current frame
 * seed into the sample textures in one call and reports it complete. A change of the type or
 * the threshold raises the film-clear trigger (MegakernelPathTracer.cpp:361-372). */
DCRT_API int dcrt_tracer_set_output(dcrt_tracer* tracer, const dcrt_output_params* params);
DCRT_API int dcrt_tracer_get_output(dcrt_tracer* tracer, dcrt_output_params* out_params);
DCRT_API int dcrt_tracer_reset_image(dcrt_tracer* tracer);                                     /* ResetImage() */
DCRT_API int dcrt_tracer_is_image_complete(dcrt_tracer* tracer, int* out_complete);           /* IsImageComplete() */
DCRT_API int dcrt_tracer_acquire_film_clear_trigger(dcrt_tracer* tracer, int* out_trigger);    /* AcquireFilmClearTrigger() */
DCRT_API int dcrt_tracer_clear_film(dcrt_tracer* tracer);
DCRT_API int dcrt_tracer_accumulate_film(dcrt_tracer* tracer, const dcrt_filter_params* filter);
DCRT_API int dcrt_tracer_read_film(dcrt_tracer* tracer, float* out_rgba);                      /* W*H*4 floats */
DCRT_API int dcrt_tracer_read_samples(dcrt_tracer* tracer, float* out_position, float* out_value); /* W*H*2, W*H*4 */
DCRT_API int dcrt_tracer_read_rng(dcrt_tracer* tracer, uint32_t* out_state);                   /* W*H*4 (debug_rng) */
DCRT_API int dcrt_tracer_film_device_ptr(dcrt_tracer* tracer, void** out_ptr);
/* The current image's sample textures in device memory (m_SamplePositionTexture R32G32F and
 * m_SampleValueTexture RGBA32F, row-major W x H of the frame resolution; Scene.cpp:863-885),
 * written by CONTROL / MATERIAL (WriteSample, RayTracingCommon.inc.hlsl:118-122): what the
 * reference's L1 SampleConvolution pass reads (SampleConvolution.cpp:89-170,
 * LaunchRendererLoop.cpp:295-297). Valid until the resolution or the image batch changes;
 * dcrt_tracer_accumulate_film is that pass on the tracer's own film. */
DCRT_API int dcrt_tracer_sample_device_ptrs(dcrt_tracer* tracer, void** out_position, void** out_value);
/* Device-to-device copy of the RGBA32F film (W*H*4 floats) into d_dst, e.g. an
 * RCCL buffer for the multi-GPU reduce; synchronous with the tracer stream. */
DCRT_API int dcrt_tracer_copy_film_device(dcrt_tracer* tracer, void* d_dst);
/* film += d_src (W*H*4 floats in device memory of the tracer's device), on the tracer
 * stream, synchronous. Combines the films of film partitions rendered by several
 * tracers of one GPU (concurrent pipelines): their supports are disjoint, so the sum
 * is the single-tracer film bit for bit. No reference counterpart (the reference has
 * one pipeline per device). */
DCRT_API int dcrt_tracer_add_film_device(dcrt_tracer* tracer, const void* d_src);
DCRT_API int dcrt_tracer_counters(dcrt_tracer* tracer, dcrt_ray_stats* out_stats);
/* counters != 0: traversal work counters in the cast kernels; ext_timing != 0: plain
 * (non-graph) launches with HIP events around every EXTENSION_RAY_CAST, MATERIAL and
 * CONTROL launch. */
DCRT_API int dcrt_tracer_set_instrumentation(dcrt_tracer* tracer, int counters, int ext_timing);
DCRT_API int dcrt_tracer_traversal_stats(dcrt_tracer* tracer, dcrt_traversal_stats* out_stats);
DCRT_API int dcrt_tracer_reset_stats(dcrt_tracer* tracer);
DCRT_API int dcrt_tracer_get_info(dcrt_tracer* tracer, dcrt_tracer_info* out_info);
/* Test hook of the spilling traversal stack (dcrt_tracer_info.ring_rows): the stack entries the
   ring cast kernel has moved to its spill columns since the scene upload (nonzero words of the
   zero-initialised columns; no stack entry is 0). 0 when the scene keeps its whole stack in LDS. */
DCRT_API int dcrt_tracer_debug_ring_spills(dcrt_tracer* tracer, uint64_t* out_words);
DCRT_API int dcrt_tracer_synchronize(dcrt_tracer* tracer);
DCRT_API int dcrt_tracer_get_luts(dcrt_tracer* tracer, dcrt_bxdf_luts* out_luts);
DCRT_API int dcrt_tracer_set_luts(dcrt_tracer* tracer, const dcrt_bxdf_luts* luts);

/* Kernel-level entry points used by the parity tests and the roofline bench:
 * one EXTENSION_RAY_CAST / SHADOW_RAY_CAST launch over a host ray batch. */
DCRT_API int dcrt_tracer_trace_rays(dcrt_tracer* tracer, const dcrt_ray* rays, uint32_t count, dcrt_ray_hit* out_hits,
                                    uint32_t features);
DCRT_API int dcrt_tracer_occluded(dcrt_tracer* tracer, const dcrt_ray* rays, uint32_t count, uint32_t* out_occluded,
                                  uint32_t features);
/* A host ray batch through the cast a render of the uploaded scene with `features` launches (the merged
 * EXTENSION + SHADOW cast's traversal: the same kernel variant, scene copy, LDS bytes and workgroup size).
 * kinds[i] == 0: an extension ray (closest hit, t_max infinite; out_hits[i] as dcrt_tracer_trace_rays writes
 * it, out_occluded[i] = 0); otherwise a shadow ray (first accepted hit below the ray's t_max: out_occluded[i],
 * out_hits[i] the miss record). `features` are taken as given: with DCRT_FEATURE_ALLOW_ANYHIT ray i carries
 * opacity_samples[i] into the any-hit shader (opacity_samples may be NULL only without the bit).
 * out_variant: the DCRT_CAST_VARIANT_* flags of the kernel that ran. */
#define DCRT_CAST_VARIANT_OPACITY    0x01u
#define DCRT_CAST_VARIANT_ALL_CACHED 0x02u
#define DCRT_CAST_VARIANT_PAIR       0x04u
#define DCRT_CAST_VARIANT_IDENT      0x08u
#define DCRT_CAST_VARIANT_RING       0x10u
#define DCRT_CAST_VARIANT_FLAT       0x20u
DCRT_API int dcrt_tracer_cast_rays(dcrt_tracer* tracer, const dcrt_ray* rays, const uint32_t* kinds, const float* opacity_samples,
                                   uint32_t count, uint32_t features, dcrt_ray_hit* out_hits, uint32_t* out_occluded,
                                   uint32_t* out_variant);
/* Device-resident variant for timing: rays/hits already in HBM, launched on the tracer stream. */
DCRT_API int dcrt_tracer_trace_rays_device(dcrt_tracer* tracer, const void* d_rays, uint32_t count, void* d_hits,
                                           uint32_t features);

/* ===== the point light's direction-cell table (shadow rays of one-point-light scenes) ===== */
/* The occlusion bits of shadow rays through the device function of the merged cast's streaming
 * shadow section. The rays must be built the way MATERIAL builds them -- origin
 * OffsetRayOrigin(P), direction normalize(L - P), t_max = |L - P| for the scene's point light L --
 * since the table is keyed by direction; dcrt_tracer_occluded is the comparison partner.
 * DCRT_E_NO_SCENE when the uploaded scene has no table (dcrt_tracer_info.shadow_cells == 0). */
DCRT_API int dcrt_tracer_trace_occlusion_cells(dcrt_tracer* tracer, const dcrt_ray* rays, uint32_t count,
                                               uint32_t* out_occluded, uint32_t features);
typedef struct dcrt_shadow_cells_info {
    uint32_t resolution;      /* R: 6 * R * R cells; 0: the scene is not eligible              */
    uint32_t leaf_count;      /* triangle leaves (bits of a mask in use)                       */
    uint32_t node_count;      /* nodes of the entry-free array                                 */
    uint32_t max_leaves;      /* most leaves in one cell                                       */
    float mean_leaves;        /* mean leaves per cell                                          */
    float r0;                 /* no triangle may come closer to the light than this            */
} dcrt_shadow_cells_info;
/* The table as upload_scene builds it for a flat scene, on the host (needs no device): the cell
 * masks (6 * R * R words, or NULL), the 128 leaf words (or NULL: word k < leaf_count = leaf k's node |
 * its guard count << 10 | the index of its first guard word << 16; a guard word is the node of an
 * ancestor whose box is tested beside the leaf's) and the entry-free nodes they index (up to
 * node_capacity; or NULL).
 * resolution 0 = the default. An ineligible scene answers DCRT_OK with out_info->resolution == 0
 * and the reason in dcrt_last_error(). The cell of a direction: dcrt_shadow_cell_indices. */
DCRT_API int dcrt_shadow_cells_build(const dcrt_flat_scene* scene, uint32_t resolution, dcrt_shadow_cells_info* out_info,
                                     uint64_t* out_cells, uint32_t* out_leaf_words, dcrt_bvh_node* out_nodes,
                                     uint32_t node_capacity);
/* Cells (indices into the masks) of `count` directions w (3 floats each), pointing from the light to
 * the ray: the negated ray directions. */
DCRT_API int dcrt_shadow_cell_indices(uint32_t resolution, const float* w, uint32_t count, uint32_t* out_cells);

/* ===== post-processing + image output (PostProcessing.cpp, PostProcessings.hlsl,
 *       SumLuminance.hlsl, SaveImageToFile.cpp) ============================== */
typedef struct dcrt_postfx_params {
    int32_t enabled;          /* m_IsPostFXEnabled (default 1); 0 = rgb / w only          */
    int32_t auto_exposure;    /* m_IsAutoExposureEnabled (default 1): log-average luminance */
    float ev100;              /* manual EV100: CalculateEV100(N, t, ISO) or m_ManualEV100  */
    float luminance_white;    /* m_LuminanceWhite (default 1), Reinhard max white          */
} dcrt_postfx_params;
/* Defaults of Scene.h:181-185 with EV100 from the scene's camera (PostProcessing.cpp:39-42). */
DCRT_API int dcrt_scene_get_postfx_params(const dcrt_scene* scene, dcrt_postfx_params* out_params);
/* The 255 linear thresholds between consecutive sRGB8 codes (R8G8B8A8_UNORM_SRGB encode). */
DCRT_API int dcrt_srgb_encode_thresholds(float out_thresholds[255]);
/* Tone-map the film into sRGB8 RGBA (W*H*4 bytes); optional sum of log luminance (auto exposure). */
DCRT_API int dcrt_tracer_resolve_image(dcrt_tracer* tracer, const dcrt_postfx_params* params, uint8_t* out_rgba8,
                                       float* out_sum_log_luminance);
/* ===== film denoiser ========================================================
 * A variance-guided, edge-avoiding a-trous wavelet filter (Dammertz et al. 2010 with the spatial
 * variance guidance of SVGF, Schied et al. 2017; no temporal part, no depth guide) for the 1-16 spp
 * films of an interactive loop. No reference counterpart. Inputs are three W x H RGBA32F images in
 * film convention (sum w*L, sum w): the colour film and two guide films holding the first hit's
 * shading normal (stored as n * 0.5 + 0.5, the view's encoding) and albedo.
 *
 * All arithmetic is fp32 in exactly this order (no contraction, correctly rounded / and sqrt,
 * exp = the det_exp of dcrt_device_math_eval function 2), so a float32 restatement matches bit
 * for bit (tests/denoise_ref.py):
 *   resolve(f) = f.w > 0 ? f.rgb / f.w : 0;  c = resolve(colour), a = resolve(albedo),
 *   n = 2 * resolve(normal) - 1;  kn = 1 / (sigma_normal * sigma_normal), ka likewise (0 for a
 *   sigma of 0: the term is off);  d = demodulate ? max(a, 1e-3) per channel : 1;
 *   lum(x) = x.r * 0.299 + x.g * 0.587 + x.b * 0.114;  h = [1/16, 1/4, 3/8, 1/4, 1/16],
 *   g = [1/4, 1/2, 1/4];  |v|^2 = v.x * v.x + v.y * v.y + v.z * v.z;  every sum runs dy outer,
 *   dx inner, ascending, by sequential adds from 0, and skips the taps outside the image.
 *   1. c_0 = c / d.
 *   2. Over the 7 x 7 window q = p + (dx, dy): wg = exp(-(|n_q - n_p|^2 * kn + |a_q - a_p|^2 * ka)),
 *      l = lum(c_0(q)); m1 += l * wg, m2 += (l * l) * wg, ws += wg; mean = m1 / ws,
 *      var_0 = max(m2 / ws - mean * mean, 0).
 *   3. Pass i = 0 .. iterations - 1, step s = 2^i: over the 3 x 3 window at step 1,
 *      gs += var_i(q) * (g[dy+1] * g[dx+1]), gw += g[dy+1] * g[dx+1]; gv = gs / gw;
 *      kl = sigma_luminance > 0 ? 1 / (sigma_luminance * sqrt(gv) + 1e-6) : 0. Over the 5 x 5 taps
 *      q = p + s * (dx, dy): e = |lum(c_i(q)) - lum(c_i(p))| * kl + |n_q - n_p|^2 * kn + |a_q - a_p|^2 * ka,
 *      w = (h[dy+2] * h[dx+2]) * exp(-e); sum += c_i(q) * w, sv += var_i(q) * (w * w), ws += w;
 *      c_{i+1} = sum / ws, var_{i+1} = sv / (ws * ws).
 *   4. Output (c_N * d, 1): an RGBA32F image in film convention, so the resolve / post-processing
 *      path takes it as it takes the film.
 * Non-finite input pixels are out of scope: they spread through the windows that contain them. */
typedef struct dcrt_denoise_params {
    uint32_t iterations;       /* a-trous passes, 1..8 (default 5: steps 1, 2, 4, 8, 16)            */
    float sigma_luminance;     /* in standard deviations of the local luminance (default 4)        */
    float sigma_normal;        /* default 0.2                                                       */
    float sigma_albedo;        /* default 0.1                                                       */
    uint32_t demodulate;       /* nonzero (default): filter c / albedo, multiply the albedo back    */
} dcrt_denoise_params;
/* A sigma of 0 switches its term off; a negative or non-finite sigma, or iterations outside 1..8,
 * is DCRT_E_INVALID_ARG in every denoise call. */
DCRT_API int dcrt_denoise_default_params(dcrt_denoise_params* out_params);   /* needs no device */
/* The guides of images first_seed .. first_seed + image_count - 1: per seed the first-hit
 * Shading Normal and Albedo views (the kernel of dcrt_tracer_set_output, at the sub-pixel
 * positions of that seed's path-traced image), each convolved into a tracer-owned guide film
 * with the reconstruction filter of the tracer's last render_images / accumulate call
 * (DCRT_E_INVALID_ARG before any), after both guide films were cleared. The film, the selected
 * output, the film-clear trigger, the counters and the frame seed stay as they are; the sample
 * textures are overwritten, and a progressive dcrt_tracer_render image in flight starts over. On
 * a banded or partitioned tracer it renders the tracer's own rows, as a view render does, and the
 * guide films of the ranks sum as their films do. */
DCRT_API int dcrt_tracer_render_guides(dcrt_tracer* tracer, uint32_t first_seed, uint32_t image_count);
/* The guide films (W*H RGBA32F each) in device memory / copied out; DCRT_E_INVALID_ARG before
 * dcrt_tracer_render_guides at the current resolution. */
DCRT_API int dcrt_tracer_guide_device_ptrs(dcrt_tracer* tracer, void** out_normal, void** out_albedo);
DCRT_API int dcrt_tracer_read_guides(dcrt_tracer* tracer, float* out_normal_rgba, float* out_albedo_rgba);
/* Filter the tracer's film with its guide films into the tracer-owned denoised image.
 * DCRT_E_INVALID_ARG without guides rendered at the current resolution, and on a banded or
 * partitioned tracer (its film lacks the neighbours' rows: reduce films and guides, then
 * dcrt_tracer_denoise_device on the sums). Synchronous, on the tracer's stream. */
DCRT_API int dcrt_tracer_denoise(dcrt_tracer* tracer, const dcrt_denoise_params* params);
/* The same filter over caller-provided device images (width * height RGBA32F each, on the
 * tracer's device) into d_out, which must not overlap an input (DCRT_E_INVALID_ARG). The tracer's
 * own film is not used, so any tracer will do, e.g. rank 0 after the RCCL reduce. Synchronous. */
DCRT_API int dcrt_tracer_denoise_device(dcrt_tracer* tracer, const dcrt_denoise_params* params, uint32_t width, uint32_t height,
                                        const void* d_color, const void* d_normal, const void* d_albedo, void* d_out);
/* ... and over host images (tests and tools). */
DCRT_API int dcrt_tracer_denoise_images(dcrt_tracer* tracer, const dcrt_denoise_params* params, uint32_t width, uint32_t height,
                                        const float* color, const float* normal, const float* albedo, float* out_rgba);
/* The result of the last dcrt_tracer_denoise (W*H*4 floats); DCRT_E_INVALID_ARG before one, or
 * after a resolution change. */
DCRT_API int dcrt_tracer_read_denoised(dcrt_tracer* tracer, float* out_rgba);
DCRT_API int dcrt_tracer_denoised_device_ptr(dcrt_tracer* tracer, void** out_ptr);
/* dcrt_tracer_resolve_image with the denoised image in the film's place. */
DCRT_API int dcrt_tracer_resolve_denoised(dcrt_tracer* tracer, const dcrt_postfx_params* params, uint8_t* out_rgba8,
                                          float* out_sum_log_luminance);
/* With ext_timing on (dcrt_tracer_set_instrumentation): the HIP-event times in ms of the kernels
 * of the last denoise call, in launch order -- prologue, variance estimate, pass 0 .. N-1.
 * Writes at most `capacity` entries; *out_count = the number of kernels (0 without ext_timing). */
DCRT_API int dcrt_tracer_denoise_timings(dcrt_tracer* tracer, float* out_ms, uint32_t capacity, uint32_t* out_count);

/* ===== film noise estimate and render-until-converged =======================
 * The half-buffer estimator (Dammertz et al. 2010, "A hierarchical automatic stopping condition for
 * Monte Carlo global illumination"; Cycles' adaptive sampling uses the same): beside the film a
 * second film, the half film, receives every other image, and the two are compared per pixel. No
 * reference counterpart.
 *
 * The tracer counts the images convolved into its film since the last clear, the film image count:
 * every film pass into the film counts (render_images / _strided with the film pass in either mode
 * and in the output views, accumulate_film, accumulate_images); the guide films and
 * add_film_device do not. While convergence is on, the image with 0-based count i also goes into
 * the half film exactly when i is even -- in the same pass, over the same rows, by the same
 * additions in the same order -- so the half film is bit for bit the film the even-counted images
 * alone would give.
 *
 * All arithmetic is fp32 in exactly this order (no contraction, correctly rounded / and sqrt), so a
 * float32 restatement matches bit for bit (tests/noise_ref.py). Per pixel, f = film, h = half film:
 *   valid = f.w > 0 && h.w > 0 (a NaN weight is invalid);  c = f.rgb / f.w, a = h.rgb / h.w;
 *   d = (|c.r - a.r| + |c.g - a.g|) + |c.b - a.b|;  s = (c.r + c.g) + c.b;
 *   n = sqrt(fmaxf(s, 0))  (negative filter lobes can make s negative);
 *   e = valid ? d / (n + 1e-4f) : 0.  A valid pixel is converged when e <= threshold (a NaN e is
 *   valid and not converged).
 * Per 16 x 16 pixel tile (thread t = ty * 16 + tx): acc[t] = e (0 outside the image); for k = 128,
 * 64 .. 1: if t < k, acc[t] = acc[t] + acc[t + k]; the tile's valid and converged counts are
 * integers, its maximum is fmaxf over its e from 0 (NaN ignored); tile error = tile sum /
 * (float)valid count, 0 without a valid pixel.
 * Whole image: the tile sums (row-major tiles) in groups of 128 consecutive values, zero padded,
 * each reduced by the tree 64 .. 1 as above, repeated until one value remains (the luminance
 * reduction's order); counts summed as integers; max_error = fmaxf of the tile maxima,
 * max_tile_error = fmaxf of the tile errors, both from 0. */
typedef struct dcrt_noise_stats {
    uint32_t images;            /* film image count (0 from dcrt_tracer_noise_device)     */
    uint32_t valid_pixels, converged_pixels;
    float mean_error;           /* total / (float)valid_pixels; 0 when none              */
    float max_error, max_tile_error;
} dcrt_noise_stats;
/* enable != 0 allocates the half film (W x H RGBA32F, 16 B per pixel, only while enabled); 0 frees
 * it. Either way the film and the half film are cleared, the film image count is reset and, on a
 * change, the captured graphs are dropped. Needs a film (frame parameters), as dcrt_tracer_clear_film
 * does; a later resolution change resizes the half film with the film. Default: off, and then
 * every film pass is the kernel it was before this existed. dcrt_tracer_clear_film clears both
 * films and resets the count. */
DCRT_API int dcrt_tracer_set_convergence(dcrt_tracer* tracer, int enable);
DCRT_API int dcrt_tracer_film_image_count(dcrt_tracer* tracer, uint32_t* out_images);
/* The half film: DCRT_E_INVALID_ARG while convergence is off. add_half_film_device is
 * dcrt_tracer_add_film_device on the half film (the half films of disjoint partitions or bands sum
 * as their films do). */
DCRT_API int dcrt_tracer_half_film_device_ptr(dcrt_tracer* tracer, void** out_ptr);
DCRT_API int dcrt_tracer_read_half_film(dcrt_tracer* tracer, float* out_rgba);                 /* W*H*4 floats */
DCRT_API int dcrt_tracer_add_half_film_device(dcrt_tracer* tracer, const void* d_src);
/* The estimate over the tracer's film and half film, on its stream; the one synchronisation is the
 * copy of the statistics. DCRT_E_INVALID_ARG with convergence off, with fewer than 2 film images,
 * or for a negative or NaN threshold. On a banded or partitioned tracer the rows it does not own
 * have weight 0 and are invalid. */
DCRT_API int dcrt_tracer_noise(dcrt_tracer* tracer, float threshold, dcrt_noise_stats* out_stats);
/* ... over caller-provided device images (width * height RGBA32F each, on the tracer's device);
 * the maps (width * height floats: e per pixel; ceil(width / 16) * ceil(height / 16) floats: tile
 * errors, row-major) are optional. The tracer's own film is not used: any tracer will do, e.g.
 * rank 0 after the reduce, or one without a scene. */
DCRT_API int dcrt_tracer_noise_device(dcrt_tracer* tracer, uint32_t width, uint32_t height, const void* d_film, const void* d_half,
                                      float threshold, void* d_pixel_map_or_null, void* d_tile_map_or_null,
                                      dcrt_noise_stats* out_stats);
/* The maps of the last dcrt_tracer_noise; DCRT_E_INVALID_ARG before one, or after a resolution
 * change. read_noise_maps takes a null pointer for a map it should skip (not for both). */
/* With ext_timing on (dcrt_tracer_set_instrumentation): launches and summed HIP-event time in ms
 * of the film passes into the film since dcrt_tracer_reset_stats (the in-graph pass is launched
 * every iteration and returns at once unless a batch completed). */
DCRT_API int dcrt_tracer_film_pass_timing(dcrt_tracer* tracer, uint64_t* out_launches, double* out_ms);
DCRT_API int dcrt_tracer_noise_map_device_ptrs(dcrt_tracer* tracer, void** out_pixel_map, void** out_tile_map);
DCRT_API int dcrt_tracer_read_noise_maps(dcrt_tracer* tracer, float* out_pixel_map, float* out_tile_map);
typedef struct dcrt_converge_params {
    float threshold;          /* per-pixel e                                                       */
    float target_fraction;    /* stop when converged_pixels >= target_fraction * valid_pixels
                                 (compared in double); in (0, 1]                                   */
    uint32_t min_images;      /* first check point, >= 2                                           */
    uint32_t max_images;      /* >= min_images                                                     */
    uint32_t check_interval;  /* >= 1                                                              */
} dcrt_converge_params;
/* Render until the estimate meets the target. The check points are the film image counts
 * min_images, min_images + check_interval, ..., capped at max_images; between them it renders with
 * dcrt_tracer_render_images, the image with film image count i from seed first_seed + i, so the
 * film it leaves at count n is bit for bit that of dcrt_tracer_render_images(first_seed, n). It
 * stops at the first check point that meets the target (*out_converged = 1) or at max_images
 * (0); *out_stats is the last estimate. The film is not cleared: the caller does that. Refuses
 * what dcrt_tracer_noise and dcrt_tracer_render_images refuse, and parameters out of range. */
DCRT_API int dcrt_tracer_render_converged(dcrt_tracer* tracer, uint32_t first_seed, const dcrt_converge_params* params,
                                          const dcrt_filter_params* filter, dcrt_noise_stats* out_stats, int* out_converged);

/* ===== adaptive sampling: trace only the film blocks that are still noisy ====
 * The film is cut into 8 x 8 pixel blocks, blocksX = ceil(W / 8) per row, block index by * blocksX
 * + bx. While adaptive sampling is on, the tracer keeps a strictly ascending list of active blocks,
 * and dcrt_tracer_render_images / _strided (wavefront and megakernel mode, with or without the film
 * pass) start one path per image in the in-film pixels of the listed blocks only. Every other
 * pixel of the image's sample textures holds the sentinel sample -- position (+inf, +inf), value
 * 0 -- to which all five reconstruction filters give the weight +0, so the film pass over them
 * is bit for bit the film of the traced samples alone (tests/adaptive_ref.py). With the film pass
 * off, the kept slots hold the sentinel too, so dcrt_tracer_accumulate_images on another tracer
 * gives the same film. The output views, dcrt_tracer_render_guides and the progressive
 * dcrt_tracer_render ignore the list. dcrt_ray_stats.new_paths counts the pixels started. No
 * reference counterpart.
 *
 * A block is active when some film pixel (x, y) with bx*8 - m <= x <= bx*8 + 7 + m and by*8 - m
 * <= y <= by*8 + 7 + m (m = the margin, in pixels) is not converged: invalid, or !(e <= threshold)
 * with valid and e of the film noise estimate above (a NaN e is not converged). The margin keeps
 * every block sampling that a noisy pixel's filter window reaches. */
typedef struct dcrt_adaptive_report {
    uint32_t images;          /* images rendered by the call                                       */
    uint32_t check_points;    /* noise estimates taken                                             */
    uint64_t pixel_samples;   /* paths started: the sum over the images of their listed pixels     */
    uint32_t active_blocks;   /* the list's length on return                                       */
    uint32_t total_blocks;    /* blocksX * ceil(H / 8)                                             */
} dcrt_adaptive_report;
/* enable != 0 allocates the flag and list buffers (4 B each per block, only while enabled) and sets
 * the list to every block; 0 frees them. On a change the captured graphs are dropped. Needs a film
 * (frame parameters); DCRT_E_INVALID_ARG on a partitioned or banded tracer, and while it is on
 * dcrt_tracer_set_film_partition (world_size > 1) and dcrt_tracer_set_film_bands are refused.
 * Default: off, and then every launch is what it was before this existed. A resolution change and
 * dcrt_tracer_clear_film (dcrt_tracer_set_convergence clears too) reset the list to every block. */
DCRT_API int dcrt_tracer_set_adaptive(dcrt_tracer* tracer, int enable);
/* The list from host memory: strictly ascending, every index < blocksX * ceil(H / 8), else
 * DCRT_E_INVALID_ARG with the list untouched. count 0 is legal: nothing is left to sample, and
 * dcrt_tracer_render_images then returns DCRT_E_INVALID_ARG before anything is launched. */
DCRT_API int dcrt_tracer_set_sample_blocks(dcrt_tracer* tracer, const uint32_t* blocks, uint32_t count);
/* Writes at most `capacity` indices; *out_count = the list's length. */
DCRT_API int dcrt_tracer_get_sample_blocks(dcrt_tracer* tracer, uint32_t* out_blocks, uint32_t capacity, uint32_t* out_count);
/* The list rebuilt from the tracer's own film and half film, on its stream; the one
 * synchronisation is the copy of the count. Refuses what dcrt_tracer_noise refuses. margin
 * 0xFFFFFFFF: the window rows of the last film pass's filter (what the halo check uses). */
DCRT_API int dcrt_tracer_update_sample_blocks(dcrt_tracer* tracer, float threshold, uint32_t margin, uint32_t* out_active);
/* The same kernels over caller-provided device images (width * height RGBA32F each): one uint32
 * flag per block (optional) and the ascending list (room for every block). Any tracer will do,
 * adaptive or not, with or without a scene. */
DCRT_API int dcrt_tracer_sample_blocks_device(dcrt_tracer* tracer, uint32_t width, uint32_t height, const void* d_film,
                                              const void* d_half, float threshold, uint32_t margin, void* d_flags_or_null,
                                              void* d_list, uint32_t* out_count);
/* With ext_timing on (dcrt_tracer_set_instrumentation): the HIP-event times in ms of the last mask
 * kernel, the last compaction kernel (update_sample_blocks / sample_blocks_device) and the last
 * sentinel fill of the sample slots; 0 for one that has not run with ext_timing on. */
DCRT_API int dcrt_tracer_adaptive_timings(dcrt_tracer* tracer, float* out_mask_ms, float* out_compact_ms, float* out_fill_ms);
/* dcrt_tracer_render_converged with the block list in the loop. It starts on every block; at each
 * check point (as there) it renders up to the point's film image count, the image with count i
 * from seed first_seed + i, takes the estimate, stops with *out_converged = 1 if the target is
 * met or with 0 at max_images, else rebuilds the list (update_sample_blocks(threshold, margin);
 * margin 0xFFFFFFFF: the window rows of `filter`) and stops with 1 if it is empty. The list is
 * rebuilt from every block each time, so blocks can wake up again; it stays in place on return
 * (dcrt_tracer_clear_film resets it). out_report may be null. */
DCRT_API int dcrt_tracer_render_adaptive(dcrt_tracer* tracer, uint32_t first_seed, const dcrt_converge_params* params,
                                         uint32_t margin, const dcrt_filter_params* filter, dcrt_noise_stats* out_stats,
                                         int* out_converged, dcrt_adaptive_report* out_report_or_null);

/* ===== firefly re-weighting: a cascaded film =================================
 * Zirr, Hanika and Dachsbacher, "Re-weighting Firefly Samples for Improved Finite-Sample Monte
 * Carlo Estimates" (CGF 2018). Beside the film, K cascade films each receive the part of every
 * sample that belongs to their brightness band; a resolve pass keeps a band at a pixel only to the
 * extent that enough samples of similar brightness landed nearby. It is consistent: a feature of
 * non-zero probability gathers support as images accumulate and its weight goes to 1; what it costs
 * is a downward bias at low image counts. The film itself is never altered. No reference
 * counterpart. Off by default, and then every film pass is the launch it was before this existed.
 *
 * All arithmetic is fp32 in exactly this order (no contraction, correctly rounded /), so a float32
 * restatement matches bit for bit (tests/firefly_ref.py).
 *   Scales: s_0 = start, s_j = s_{j-1} * base, float32 products on the host; r = 1 / base and
 *   d = 1 - r, float32 on the host too. The kernels and the reference use these numbers.
 *   Y(v) = fmaxf(0, v.r * 0.299f + v.g * 0.587f + v.b * 0.114f), the film kernels' weights, summed
 *   left to right.
 *   Split of a sample v of luminance Y into (band, alpha): Y <= s_0 (and a NaN Y, which fmaxf
 *   makes 0): band 0, alpha 1. Y > s_{K-1}: band K - 1, alpha 1 -- nothing is clamped. Otherwise
 *   band = the j with s_j < Y <= s_{j+1} and alpha = fminf(fmaxf((s_j / Y - r) / d, 0), 1).
 *   Cascade `band` takes alpha * v.rgb, cascade band + 1 (if there is one) takes (1 - alpha) * v.rgb,
 *   1 - alpha rounded to float32 first; with exact arithmetic a sample counts once across the two:
 *   alpha Y / s_j + (1 - alpha) Y / s_{j+1} = 1.
 *   Accumulation: cascade film j is W x H RGBA32F. Per film pass and pixel, with the film pass's
 *   windows and weights w (images in order, window rows then columns): sum_j = 0 per image;
 *   sum_j = sum_j + (share_j(v) * w) per tap whose sample has a share in j -- the share first, then
 *   times w, per channel -- and C_j.rgb = C_j.rgb + sum_j after each image. (A tap without a share
 *   in j adds nothing, which equals adding +0.) C_j.w is never written: it stays 0 from the clear,
 *   and the film's own .w is the weight sum for every cascade.
 *   Resolve at pixel p, W(p) = film.w, N = (float)image count:
 *   count_i(q) = (N * Y(C_i(q).rgb)) / (W(q) * s_i), 0 for a q outside the image or with
 *   !(W(q) > 0);  T_i(p) = the sum of count_i(q) over the 3 x 3 pixels q around p, sequential adds
 *   from 0, rows then columns;  S_j = (T_{j-1} + T_j) + T_{j+1} without the terms outside [0, K);
 *   omega_0 = 1, omega_j = fminf(fmaxf((S_j - 1) / min_support, 0), 1) for j >= 1: a sample does
 *   not support itself.  acc = C_0(p).rgb; acc = acc + C_j(p).rgb * omega_j for j = 1 .. K-1;
 *   out(p) = (acc / W(p), 1), and (0, 0, 0, 0) where !(W(p) > 0).
 * The output is film convention, as the denoised image is: dcrt_tracer_denoise_device takes it as
 * its colour input and the resolve / post-processing path takes it as it takes the film.
 * Non-finite sample values are out of scope, as for the denoiser.
 * The defaults (6, 1, 8, 3) come from a float64 prototype on a synthetic run only; nobody has
 * measured them on a render. */
typedef struct dcrt_firefly_params {
    uint32_t cascades;   /* K, 2..8            (default 6) */
    float start;         /* s_0 > 0, luminance (default 1) */
    float base;          /* b > 1              (default 8) */
    float min_support;   /* kappa > 0          (default 3) */
} dcrt_firefly_params;
/* K outside 2..8, a non-finite float, start <= 0, base <= 1, min_support <= 0 or an s_{K-1} that is
 * not finite is DCRT_E_INVALID_ARG in every call that takes the parameters. */
DCRT_API int dcrt_firefly_default_params(dcrt_firefly_params* out_params);   /* needs no device */
/* With params: allocates the K cascade films (K * W * H * 16 B, only while on); null: frees them
 * and switches the feature off. Either way the film, the half film if any and the cascades are
 * cleared and the film image count is reset; on a change of K, start or base, or of on / off, the
 * captured graphs are dropped -- a change of min_support alone reallocates and drops nothing (it
 * still clears). Needs a film (frame parameters); a later resolution change resizes the cascades
 * with the film, dcrt_tracer_clear_film clears them, and the parameters persist across
 * dcrt_tracer_upload_scene. While on, every film pass into the film (render_images / _strided in
 * either mode and in the output views, accumulate_film, accumulate_images) also launches the
 * cascade pass over the same images, so the cascades' image count is the film's; the guide films
 * are not covered, and dcrt_tracer_add_film_device, a partition of world_size > 1 and film bands
 * are DCRT_E_INVALID_ARG (the film would hold what the cascades lack). On a partitioned or banded
 * tracer set_firefly itself is DCRT_E_INVALID_ARG: reduce film and cascades yourself, then
 * dcrt_tracer_firefly_resolve_device. get_firefly: *out_enabled, and the parameters when on. */
DCRT_API int dcrt_tracer_set_firefly(dcrt_tracer* tracer, const dcrt_firefly_params* params_or_null);
DCRT_API int dcrt_tracer_get_firefly(dcrt_tracer* tracer, int* out_enabled, dcrt_firefly_params* out_params);
/* The resolve over the tracer's film and cascades into the tracer-owned re-weighted image.
 * DCRT_E_INVALID_ARG while the feature is off or before any image reached the film. Synchronous. */
DCRT_API int dcrt_tracer_firefly_resolve(dcrt_tracer* tracer);
/* The result of the last dcrt_tracer_firefly_resolve (W*H*4 floats); DCRT_E_INVALID_ARG before
 * one, or after a resolution change or a set_firefly. */
DCRT_API int dcrt_tracer_read_firefly(dcrt_tracer* tracer, float* out_rgba);
DCRT_API int dcrt_tracer_firefly_device_ptr(dcrt_tracer* tracer, void** out_ptr);
/* dcrt_tracer_resolve_image with the re-weighted image in the film's place. */
DCRT_API int dcrt_tracer_resolve_firefly(dcrt_tracer* tracer, const dcrt_postfx_params* params, uint8_t* out_rgba8,
                                         float* out_sum_log_luminance);
/* dcrt_tracer_denoise with the re-weighted image of the last dcrt_tracer_firefly_resolve in the film's place as the
 * colour input (the guides are the film's); the result is the tracer's denoised image, as dcrt_tracer_denoise's.
 * DCRT_E_INVALID_ARG before a resolve, or without guides rendered at the current resolution. */
DCRT_API int dcrt_tracer_denoise_firefly(dcrt_tracer* tracer, const dcrt_denoise_params* params);
/* The K cascade films, K * W*H*4 floats, cascade 0 first / their K device pointers (`capacity`
 * entries of room; *out_count = K). DCRT_E_INVALID_ARG while the feature is off. */
DCRT_API int dcrt_tracer_read_cascades(dcrt_tracer* tracer, float* out_rgba);
DCRT_API int dcrt_tracer_cascade_device_ptrs(dcrt_tracer* tracer, void** out_ptrs, uint32_t capacity, uint32_t* out_count);
/* The resolve over caller-provided device images (width * height RGBA32F each, on the tracer's
 * device; d_cascades: params->cascades host-side pointers to device images) into d_out, which must
 * not overlap an input. image_count >= 1. The tracer's own film is not used: any tracer will do,
 * e.g. rank 0 after the reduce, or one without a scene. Synchronous. */
DCRT_API int dcrt_tracer_firefly_resolve_device(dcrt_tracer* tracer, const dcrt_firefly_params* params, uint32_t width, uint32_t height,
                                                uint32_t image_count, const void* d_film, const void* const* d_cascades, void* d_out);
/* With ext_timing on (dcrt_tracer_set_instrumentation): the HIP-event times in ms of the last
 * cascade pass launched on its own (the megakernel mode, the output views, accumulate_film,
 * accumulate_images; the pass inside the wavefront iteration is launched every iteration, returns at
 * once unless a batch completed, and is not timed) and of the last resolve; 0 for one that has
 * not run with ext_timing on. */
DCRT_API int dcrt_tracer_firefly_timings(dcrt_tracer* tracer, float* out_cascade_ms, float* out_resolve_ms);

/* ===== environment importance sampling ==========================================
 * The environment light is sampled with a uniform direction and pdf 1 / (4 pi), as in the reference
 * (DCRT_ENV_SAMPLING_UNIFORM, the default: every result is then what it was before this existed). With
 * DCRT_ENV_SAMPLING_IMPORTANCE and an environment cube in the scene, light samples follow the cube's
 * power instead. No reference counterpart. tests/env_importance_ref.py restates all of this in float64.
 *
 * Texels. n = env_cube_size. Texel (f, y, x) has the face coordinates sc = (2x + 1) / n - 1 and tc =
 * (2y + 1) / n - 1: the (sc, tc) of the cube lookup, with its face table and axis signs.
 * Weight. Y = max(0, 0.299 r + 0.587 g + 0.114 b) of the texel in float32, products summed left to
 * right (the film kernels' luminance; fmaxf semantics: a NaN counts 0). M = the largest Y over the texel's
 * 3 x 3 neighbourhood clamped inside the face -- the lookup clamps its bilinear taps inside the face, so
 * anywhere in a texel it reads only that neighbourhood. w = M (4 / n^2) (1 + sc^2 + tc^2)^(-3/2) in float64.
 * Table. P = w / sum(w); rows r = f n + y. Stored as float32: P [6n][n], the per-row conditional CDF
 * [6n][n], the marginal CDF over rows [6n]; both CDFs are float64 sums in ascending index order, each
 * stored CDF's last entry is exactly 1, a row whose total is 0 has a conditional CDF of zeros and the
 * marginal never selects it. The table depends on the cube alone: dcrt_tracer_update_lights does not
 * rebuild it. If sum(w) is 0 or not finite there is no table and sampling stays uniform ("inactive").
 * Density. pdf(wi) = (1 - e) P(texel(wi)) (n^2 / 4) (1 + sc^2 + tc^2)^(3/2) + e / (4 pi), e = 1/16, with
 * (sc, tc) the face coordinates of wi and texel(wi) the face, ix = clamp(floor(u n)) and iy =
 * clamp(floor(v n)) of the lookup's own u = (sc + 1) / 2 and v = (tc + 1) / 2. Light sampling returns this
 * density of the direction it produced, and light evaluation the same function: bitwise equal for one wi.
 * Sampling. From the same three numbers as uniform sampling -- the light selector, then a, then b: if a < e
 * the uniform-sphere direction of (a / e, b); else with a' = (a - e) / (1 - e) the row is the first r with
 * marginal[r] > a', the column the first c with cdf[r][c] > b, the remainders fa = (a' - lo) / (hi - lo) and
 * fb likewise (each clamped below 1) place the point inside the texel, sc = 2 (c + fb) / n - 1, tc =
 * 2 (y + fa) / n - 1, and the direction is the inverse of the lookup's face map, normalised. Radiance
 * (lookup times the light's colour), the infinite distance and the division by the light count are unchanged. */
#define DCRT_ENV_SAMPLING_UNIFORM 0
#define DCRT_ENV_SAMPLING_IMPORTANCE 1
/* The mode: set on an uploaded scene, as the scene edits are (DCRT_E_NO_SCENE without one), and kept across
 * every later dcrt_tracer_upload_scene; another value is DCRT_E_INVALID_ARG. The table is built at once (and at
 * every later upload, while the mode is on). A scene without a cube accepts the mode and stays uniform. A change of what the kernels sample by drops the captured graphs;
 * film and path state are not touched: restart the image, as after a scene edit. */
DCRT_API int dcrt_tracer_set_environment_sampling(dcrt_tracer* tracer, int mode);
/* *mode: the mode set; *active: 1 while a table stands for the uploaded scene and the mode is on. Either
 * pointer may be null. */
DCRT_API int dcrt_tracer_get_environment_sampling(dcrt_tracer* tracer, int* mode, int* active);
/* The table as stored: prob and row_cdf 6 n n floats, marginal_cdf 6 n floats (null: not wanted).
 * DCRT_E_NO_SCENE when inactive. */
DCRT_API int dcrt_tracer_read_environment_distribution(dcrt_tracer* tracer, float* prob, float* row_cdf, float* marginal_cdf);
/* The HIP-event time in ms of the last table build's three kernels (0: none built). */
DCRT_API int dcrt_tracer_environment_build_timing(dcrt_tracer* tracer, float* out_ms);

/* ===== Russian roulette ==========================================================
 * A path runs to max_bounce_count unless it leaves the scene or its BSDF sample is rejected. With Russian
 * roulette on, a path whose throughput has fallen is ended at random and the survivors are weighted up, which
 * leaves every pixel's expectation as it was and removes the late, dim bounces' rays. Off by default: every
 * result is then bit for bit what it was before this existed. No reference counterpart. tests/roulette_ref.py
 * restates the rule in numpy float32.
 *
 * Where. At a shaded vertex whose bounce index b (0 at the camera ray's hit) is >= start_bounce, and only when
 * the vertex's BSDF sample was accepted (bsdf nonzero and pdf nonzero). T' is the throughput after the sample,
 * T' = T * bsdf * |n . wi| / pdf, all float32.
 * Survival probability. q = fminf(fmaxf(fmaxf(fmaxf(T'.x, T'.y), T'.z), min_survival), max_survival), with
 * fmaxf / fminf semantics, so q is always in [min_survival, max_survival]: a NaN component does not count (all
 * three NaN: min_survival) and an infinite one gives max_survival.
 * q >= 1. Nothing happens and no random number is drawn: with min_survival = max_survival = 1 the result is the
 * roulette-off result bit for bit.
 * Draw order. Otherwise u is the path's next random number, drawn immediately after the three numbers of the
 * BSDF sample (the lobe selector, then the two sample coordinates). In the wavefront mode that is before the
 * vertex's opacity draws (ALLOW_ANYHIT_SHADER: extension ray, then shadow ray); in the megakernel mode it is
 * before anything the next bounce draws.
 * Outcome. u < q: the path goes on with T' / q, a division per component (not a multiplication by 1 / q).
 * Otherwise the path ends exactly as one whose BSDF sample was rejected: no extension ray, and the vertex's
 * shadow ray, if it has one, is still cast and its light sample still added.
 * Untouched. The vertex's light sample uses the throughput from before the roulette; the BSDF pdf carried to
 * the next vertex's MIS weight and the delta flag are as without it; shadow rays are never rouletted.
 * Depends on nothing but the path's own random numbers and throughput: pool size, image batch, film bands and
 * the kernel route (early finish, drain, fused shadow test) do not change a bit of the result.
 * Output views, dcrt_tracer_render_guides, the noise estimate, render_converged, adaptive sampling and the
 * denoiser are unaffected and work on top of it unchanged. */
typedef struct dcrt_roulette_params {
    uint32_t enable;          /* 0: off (the other fields are kept and ignored) */
    uint32_t start_bounce;    /* first bounce index tested; <= DCRT_MAX_RAY_BOUNCE */
    float    min_survival;    /* 0 < min_survival <= max_survival <= 1 */
    float    max_survival;
} dcrt_roulette_params;       /* 16 bytes */
/* The suggested setting, still off: enable 0, start_bounce 2, min_survival 0.05, max_survival 1. Needs no device. */
DCRT_API int dcrt_roulette_default_params(dcrt_roulette_params* out);
/* The setting lives on the tracer: kept across dcrt_tracer_upload_scene and the partial updates, read at the
 * start of every image beside max_bounce_count (no captured graph depends on it). DCRT_E_INVALID_ARG unless
 * 0 < min_survival <= max_survival <= 1 (non-finite values fail that) and start_bounce <= DCRT_MAX_RAY_BOUNCE;
 * the setting then stays as it was. Film and path state are not touched: restart the image, as after
 * dcrt_tracer_set_frame_params. */
DCRT_API int dcrt_tracer_set_roulette(dcrt_tracer* tracer, const dcrt_roulette_params* params);
DCRT_API int dcrt_tracer_get_roulette(dcrt_tracer* tracer, dcrt_roulette_params* out);
/* The kernels' roulette on count given throughputs T' (3 floats each) with u in place of the path's draw (tests):
 * out_q the survival probability, out_survive 1 where the path goes on (q >= 1 or u < q) else 0, out_scaled the
 * throughput it goes on with (T' / q; T' itself where q >= 1 or the path ends). Of params only min_survival and
 * max_survival are read; they are checked as the setter checks them. */
DCRT_API int dcrt_device_roulette(dcrt_tracer* tracer, const dcrt_roulette_params* params, const float* throughputs,
                                  const float* u, uint32_t count, float* out_q, uint32_t* out_survive, float* out_scaled);

/* ===== light selection ===========================================================
 * Next-event estimation picks its light as floor(sel * light_count) and, inside a mesh light, its triangle as
 * floor(triSel * triangle_count), as in the reference (DCRT_LIGHT_SAMPLING_UNIFORM, the default: every result
 * is then bit for bit what it was before this existed). With DCRT_LIGHT_SAMPLING_POWER lights are picked in
 * proportion to their power and a lamp's triangles in proportion to their area, from a table built by device
 * kernels at upload. No reference counterpart. tests/light_table_ref.py restates all of this in float64.
 *
 * Weights, float64; n = the lights uploaded. Y(c) = max(0, 0.299 r + 0.587 g + 0.114 b) in float32, products
 * summed left to right (the film kernels' and the environment table's luminance; a NaN counts 0).
 *   point light        w = 4 pi Y(radiance)
 *   directional light  w = pi R^2 Y(radiance)
 *   mesh light         w = pi Y(radiance) A, A = the sum over its triangle range, in ascending order, of a_t: the
 *                      world-space area as light sampling computes it -- float32, 0.5 * length(cross(w2 - w0,
 *                      w1 - w0)) of the transformed vertices -- counting 0 below 1e-6 or when not finite
 *   environment light  w = 4 pi . pi R^2 Y(colour) Ybar; Ybar = 1 without a cube, else sum(Y(texel) omega) /
 *                      sum(omega) over the texels in index order, omega = (4 / n^2) (1 + sc^2 + tc^2)^(-3/2) at the
 *                      texel's centre (the environment section's face coordinates), both sums float64
 * R = half the diagonal of the uploaded BVH root's box (float32 bounds, float64 arithmetic), taken at
 * dcrt_tracer_upload_scene and kept for later light edits.
 * Probabilities. P(l) = (1 - e) w_l / sum(w) + e / n, e = 1/16 (the environment table's uniform share: every light
 * stays reachable and 1 / P <= 16 n). P(t | l) = a_t / A_l. Stored as float32: lightProb[n], lightCdf[n], and for
 * the E = sum of the mesh lights' triangle counts emissive triangles in light order triProb[E] and triCdf[E] (a CDF
 * per light), triBase[n] (uint32: the first entry of light l; a light that is no mesh light has no entries). CDFs are
 * float64 sums in ascending order, normalised, rounded once; each CDF's last entry is exactly 1. A mesh light with
 * A = 0 has w = 0 and a triangle CDF of zeros: selecting it gives pdf 0 and radiance 0. sum(w) zero or not finite:
 * no table ("inactive": uniform selection). Also inactive: a scene whose only light is not a mesh light.
 * Sampling. The same numbers in the same order as uniform selection: sel, then what the kind draws. The light is
 * the first l with lightCdf[l] > sel; a mesh light's triangle the first k with triCdf[triBase[l] + k] > triSel
 * (triangle triangle_offset + k); both clamped to the last index. Point on the triangle, environment direction and
 * radiance are unchanged.
 * Density. One function serves light sampling and light evaluation. The selection factor is P(l) for a point,
 * directional or environment light -- the kind's own pdf (1 for the delta lights) times lightProb[l] in place of the
 * division by light_count -- and for a mesh light (lightProb[l] * triProb[triBase[l] + k]) / a_t, zero where a_t
 * counts 0, in place of 1 / area / triangle_count / light_count; the pdf is that factor times d^2 / cos, all float32
 * in this order. Light sampling thus reports the density it draws from, 1 / A_l over the lamp times d^2 / cos times
 * P(l): the reference's doubled sampler pdf (Light.inc.hlsl:50,61) does not carry into this mode.
 * Frames. While a table stands, a render or probe whose frame.light_count differs from n is DCRT_E_INVALID_ARG. */
#define DCRT_LIGHT_SAMPLING_UNIFORM 0
#define DCRT_LIGHT_SAMPLING_POWER 1
typedef struct dcrt_light_table_info {
    uint32_t light_count;        /* n */
    uint32_t triangle_entries;   /* E */
    double   scene_radius;       /* R */
    double   total_weight;       /* sum(w) */
} dcrt_light_table_info;         /* 24 bytes */
/* The mode: set on an uploaded scene, as the scene edits are (DCRT_E_NO_SCENE without one), and kept across every
 * later dcrt_tracer_upload_scene; another value is DCRT_E_INVALID_ARG. The table is built at once, at every later
 * upload and at every dcrt_tracer_update_lights while the mode is on (an edit that keeps the lights' count, kinds,
 * triangle ranges and instances rewrites lightProb and lightCdf in place and keeps the captured graphs; any other
 * rebuilds the table and drops them). Film and path state are not touched: restart the image. */
DCRT_API int dcrt_tracer_set_light_sampling(dcrt_tracer* tracer, int mode);
/* *mode: the mode set; *active: 1 while a table stands for the uploaded scene and the mode is on. Either pointer
 * may be null. */
DCRT_API int dcrt_tracer_get_light_sampling(dcrt_tracer* tracer, int* mode, int* active);
/* The table as stored: light_prob, light_cdf n floats, tri_base n words, tri_prob, tri_cdf E floats (null: not
 * wanted; take n and E from a first call with only out_info). DCRT_E_NO_SCENE when inactive. */
DCRT_API int dcrt_tracer_read_light_distribution(dcrt_tracer* tracer, dcrt_light_table_info* out_info, float* light_prob,
                                                 float* light_cdf, uint32_t* tri_base, float* tri_prob, float* tri_cdf);
/* The HIP-event time in ms of the last table build's kernels (0: none built). */
DCRT_API int dcrt_tracer_light_table_build_timing(dcrt_tracer* tracer, float* out_ms);

/* 24-bit BMP writer ("Save Image to File", SaveImageToFile.cpp:92-182). */
DCRT_API int dcrt_write_bmp(const char* path, uint32_t width, uint32_t height, const uint8_t* rgba8);

/* Deterministic transcendental helpers shared by kernels (parity tests): function 0 sin, 1 cos,
   2 exp, 3 atan, 4 log (the det_* polynomials), 5 the fast reciprocal rcp_ieee, 6 IEEE 1/x. */
DCRT_API int dcrt_device_math_eval(dcrt_tracer* tracer, int function, const float* x, uint32_t count, float* out_y);

/* One material's BSDF at chosen directions (tests): MATERIAL's own bsdf_frame / evaluate_bsdf /
   evaluate_bsdf_pdf / sample_bsdf in the frame normal = geometric normal = (0,0,1), tangent =
   (1,0,0), with the tracer's current LUTs (dcrt_tracer_set_luts); no scene is needed. albedo holds
   a conductor's k. Of `features` only DCRT_FEATURE_GGX_SAMPLE_VNDF is read. DCRT_SHADING_TABLES' rows bit
   is read at every call (the tracer reads it at uploads and edits): with it the probe builds the
   material's rows of the dielectric LUT and takes MATERIAL's path over them. */
typedef struct dcrt_bsdf_probe_material {
    uint32_t type;                        /* DCRT_MATERIAL_TYPE_* */
    float albedo[3];
    float ior[3];
    float alpha;
    uint32_t two_sided, multiscattering;
    uint32_t internal_scattering_mode;    /* DCRT_INTERNAL_SCATTERING_* */
} dcrt_bsdf_probe_material;               /* 44 bytes */
/* count (wi, wo) pairs, 3 floats each: f (3 per pair) and pdf. */
DCRT_API int dcrt_device_bsdf_eval(dcrt_tracer* tracer, const dcrt_bsdf_probe_material* material, uint32_t features,
                                   const float* wi, const float* wo, uint32_t count, float* out_f, float* out_pdf);
/* count wo and (sx, sy, sel) triples: wi, f (3 each), pdf and the delta flag (0 / 1). */
DCRT_API int dcrt_device_bsdf_sample(dcrt_tracer* tracer, const dcrt_bsdf_probe_material* material, uint32_t features,
                                     const float* wo, const float* u, uint32_t count, float* out_wi, float* out_f,
                                     float* out_pdf, uint32_t* out_delta);

/* The shading frame of chosen hit records of the uploaded scene (tests): MATERIAL's hit reconstruction in
   the form that may take the per-triangle frame table, over `count` records of 4 words each -- u, v (floats,
   any bit pattern: a -0 among them), the triangle index and the instance index (uint32 bits) -- with the
   scene's table (use_table != 0; DCRT_E_NO_SCENE when the scene has none: a BLAS with two instances) or
   without it. out_frames: 9 floats per record, the world-space normal, tangent and geometry normal. */
DCRT_API int dcrt_device_frame_probe(dcrt_tracer* tracer, const uint32_t* records, uint32_t count, int use_table, float* out_frames);

/* The stages between the ray casts and the BSDF at chosen inputs (tests; tests/shading_ref.py is their float64
   reference): the path kernels' own generate_ray, hit_to_intersection, sample_light, evaluate_light and
   sample_env, on the uploaded scene and the current frame parameters (dcrt_tracer_set_frame_params). A null
   pointer with a nonzero count is DCRT_E_INVALID_ARG, as is an index outside the scene.
   camera_ray: `count` film samples (2 floats each: the film point in [0, 1]^2) and aperture numbers (3 floats
   each) -> world-space ray origins and directions, 3 floats each. Needs frame parameters only. */
DCRT_API int dcrt_device_camera_ray(dcrt_tracer* tracer, const float* film_samples, const float* aperture_samples, uint32_t count,
                                    float* out_origins, float* out_directions);
/* Hit records as dcrt_device_frame_probe takes them (bit 31 of the triangle word: the backface bit) -> per record
   16 floats -- world-space position, normal, tangent, geometry normal, albedo (3 each), alpha -- and 3 words --
   the material type, flags (1 two-sided, 2 backface, 4 multiscattering, internal scattering mode << 4), the
   instance's light index. use_table != 0: the form of the hit reconstruction that takes the frame table
   (DCRT_E_NO_SCENE when the scene has none); 0: the per-hit form. */
DCRT_API int dcrt_device_intersection_probe(dcrt_tracer* tracer, const uint32_t* records, uint32_t count, int use_table,
                                            float* out_floats, uint32_t* out_words);
/* Light sampling from `count` points (3 floats) with xoshiro128** states (4 words) over the frame's light_count
   lights -> per point 8 floats -- radiance, wi (3 each), pdf, distance -- and 5 words -- the delta flag, the
   state after the draws (1 for a punctual light, 4 for a mesh light, 3 for the environment). A state whose
   draws select past the lights or the scene's triangles is refused. */
DCRT_API int dcrt_device_light_sample(dcrt_tracer* tracer, const float* points, const uint32_t* rng_states, uint32_t count,
                                      float* out_floats, uint32_t* out_words);
/* Light evaluation of `count` (light index, triangle index) word pairs and 7 floats each -- the light's normal at
   the hit, wi, distance -> radiance (3 floats) and pdf. */
DCRT_API int dcrt_device_light_eval(dcrt_tracer* tracer, const uint32_t* light_triangle, const float* normal_wi_distance,
                                    uint32_t count, float* out_radiance_pdf);
/* The environment cube at `count` directions (3 floats) -> rgb. DCRT_E_NO_SCENE without a cube. */
DCRT_API int dcrt_device_env_lookup(dcrt_tracer* tracer, const float* directions, uint32_t count, float* out_rgb);

/* The instance whose BLAS holds each triangle of a flat scene (host only; the frame table's eligibility
   rule): out_instances[t], UINT32_MAX for a triangle no instance reaches. Returns DCRT_OK and *out_single_use
   = 1 where every reached triangle belongs to one instance, 0 where a BLAS has two instances or the tree is
   malformed (out_instances is then unspecified). */
DCRT_API int dcrt_flat_scene_triangle_instances(const dcrt_flat_scene* scene, uint32_t* out_instances, uint32_t capacity, int* out_single_use);

#ifdef __cplusplus
}
#endif

#endif /* DCRT_H_ */
