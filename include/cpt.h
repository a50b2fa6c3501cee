/*
 * cpt.h — C-ABI of the MI355X path-tracing integrator (libcpt.so).
 *
 * This is the drop-in boundary for the reference's hot path (DearPoca/CppPathTracer,
 * cuSrc/path_tracer.cu:124-175 `SamplePixel` and everything it reaches).  Plain C types
 * only: no HIP, CUDA or torch types cross it.  Every function returns an int status
 * (0 = CPT_OK); no exception crosses the ABI.  The reference logs CUDA errors and
 * continues (path_tracer.cu:54-57, 279-283); here the status is returned and the message
 * is kept in cpt_last_error().
 *
 * Which reference interface each entry point replaces (file:line under the reference):
 *
 *   cpt_create / cpt_destroy        PathTracer construction + InitBuffers' cudaMallocs
 *                                   (path_tracer.cu:44-115); the reference never frees.
 *   cpt_set_scene                   SceneBVH::AddObject + BuildBVH + BuildBVHInGpu
 *                                   (bvh.cu:22-29, 116-120, 97-114), reached from
 *                                   PathTracer::AddObject / InitPipeline (path_tracer.cu:29-34, 308-314).
 *   cpt_update_object(s)            SceneBVH::UpdateObject (bvh.cu:144-157).
 *   cpt_set_env_texture             PocaTextureUtils::AddTexByFile (textures.cu:14-62) +
 *                                   the sky load in InitBuffers (path_tracer.cu:47).
 *   cpt_bind_texture                AddTexByFile for a material texture: the handle the app
 *                                   stores in Material::tex_ (material.h:21-25), sampled by
 *                                   Material::GetKd (material.cu:11-18).
 *   cpt_set_frame                   InitBuffers' per-pixel buffers (path_tracer.cu:44-115),
 *                                   plus a row window/list for multi-GPU row tiling.
 *   cpt_init_rng                    InitCuRand kernel (path_tracer.cu:36-42, 99-107).
 *   cpt_camera_get_copy             MotionalCamera::GetCopy (motional_camera.cu:177-200).
 *   cpt_render                      The SamplePixel launch in PipelineLoop
 *                                   (path_tracer.cu:264-283), `spp` passes at once.
 *   cpt_read_accum / cpt_read_aux   The per-pixel render_target / normal / depth buffers
 *                                   written by SamplePixel (path_tracer.cu:172-174).
 *   cpt_denoise_mix                 Denoising + Mix + BGRA8 readback (path_tracer.cu:177-254,
 *                                   285-303).
 *   cpt_denoise_mix_band            The same for one row band of a multi-GPU display (the
 *                                   Denoising/Mix launch restricted to rows y0..y1-1; the
 *                                   band's renderer also renders a 3-row halo).
 */
#ifndef CPT_H_
#define CPT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPT_ABI_VERSION 1

enum cpt_status {
    CPT_OK = 0,
    CPT_ERR_INVALID_ARG = 1,
    CPT_ERR_NO_DEVICE = 2,
    CPT_ERR_HIP = 3,
    CPT_ERR_OUT_OF_MEMORY = 4,
    CPT_ERR_STATE = 5,       /* e.g. render before scene/frame/rng were set */
    CPT_ERR_UNSUPPORTED = 6,
    /* A kernel had to abandon work (e.g. a tail-consolidation hand-over timed out, so some
     * pixels were not finished); reported by the next synchronising call on the context
     * (cpt_synchronize, cpt_read_accum, cpt_read_rng, cpt_render with CPT_RENDER_SYNC, ...),
     * like the reference's logged CUDA errors (path_tracer.cu:279-283).  Sticky until read. */
    CPT_ERR_DEVICE = 7
};

/* PrimitiveType::Enum (object.h:7-15) and MaterialType::Enum (material.h:5-15). */
enum cpt_primitive_type { CPT_PRIM_SPHERE = 0, CPT_PRIM_PLATFORM = 1, CPT_PRIM_CYLINDER = 2 };
enum cpt_material_type {
    CPT_MAT_DIFFUSE = 0,
    CPT_MAT_METAL = 1,   /* shaded by MirrorHitShader (material.cu:151-153 swap, kept) */
    CPT_MAT_MIRROR = 2,  /* shaded by MetalHitShader  (material.cu:154-156 swap, kept) */
    CPT_MAT_GLASS = 3,
    CPT_MAT_TEST = 4     /* falls through to Diffuse (material.cu:160-161) */
};

/* Layout-identical to CUDA float3 (12 bytes, 4-byte aligned). */
typedef struct cpt_float3 { float x, y, z; } cpt_float3;

/* Material (material.h:17-35), 40 bytes. */
typedef struct cpt_material {
    int32_t type;              /* @0  cpt_material_type */
    uint8_t have_tex;          /* @4  nonzero: kd = the texture bound to u.tex (cpt_bind_texture) */
    uint8_t pad_[3];
    union {                    /* @8  union { float3 kd_; cudaTextureObject_t tex_; } */
        cpt_float3 kd;
        uint64_t tex;
    } u;
    float refractive_index;    /* @24 */
    float emit_intensity;      /* @28 */
    float smoothness;          /* @32 */
    float reflectivity;        /* @36 */
} cpt_material;

/* Object (object.h:17-32), 72 bytes. */
typedef struct cpt_object {
    int32_t type;              /* @0  cpt_primitive_type */
    int32_t pad_;
    cpt_material material;     /* @8  */
    cpt_float3 center;         /* @48 */
    float radius;              /* @60 sphere, cylinder */
    float y_pos;               /* @64 platform */
    float height;              /* @68 cylinder */
} cpt_object;

/* MotionalCamera (motional_camera.h:8-24), 136 bytes.  u/v/w/top_left/horizontal/vertical
 * are the GetCopy() outputs; cpt_camera_get_copy() fills them. */
typedef struct cpt_camera {
    cpt_float3 vup;            /* @0   */
    int32_t width, height;     /* @12, @16 */
    uint32_t cur_sample_idx;   /* @20  */
    cpt_float3 origin;         /* @24  */
    cpt_float3 look_at;        /* @36  */
    float view_fov;            /* @48  degrees */
    float dist_to_focus;       /* @52  */
    float lens_radius;         /* @56  */
    float move_speed;          /* @60  */
    cpt_float3 u, v, w;        /* @64, @76, @88 */
    cpt_float3 top_left_corner;/* @100 */
    cpt_float3 horizontal;     /* @112 */
    cpt_float3 vertical;       /* @124 */
} cpt_camera;

/* Per-render counters for the algorithmic byte model. */
typedef struct cpt_stats {
    uint64_t segments;     /* TraceRay calls                          */
    uint64_t node_visits;  /* non-sentinel nodes popped (bvh.cu:173)  */
    uint64_t prim_tests;   /* IntersectionTest calls (bvh.cu:176)     */
    uint64_t hits;
    uint64_t misses;
} cpt_stats;

typedef struct cpt_ctx cpt_ctx;

/* cpt_render flags */
#define CPT_RENDER_ACCUMULATE 0x1u   /* add into the accumulator instead of overwriting it   */
#define CPT_RENDER_AUX        0x2u   /* write first-hit normal + depth of the last pass       */
#define CPT_RENDER_STATS      0x4u   /* count segments/nodes/prims/hits/misses (slower)       */
#define CPT_RENDER_SYNC       0x8u   /* block until the render finished                        */
#define CPT_PATH_MEGAKERNEL   0x000u /* per-lane path regeneration megakernel (default)        */
#define CPT_PATH_WAVEFRONT    0x100u /* SoA wavefront: extend / shade / compact per bounce      */
/* Near-first BVH walk: each ray walks the node order of its direction octant (near child of
 * every split first), and equal distances go to the primitive the reference order meets
 * first.  It finds the same closest hit as the reference's right-first DFS
 * (bvh.cu:167-205) unless a primitive's computed hit distance lies outside its own box's
 * computed slab interval by rounding (DESIGN.md §Ordered walk).  Node/prim counts
 * (CPT_RENDER_STATS) are then this walk's counts, not the reference's. */
#define CPT_TRAVERSAL_ORDERED 0x200u
/* With CPT_TRAVERSAL_ORDERED: test each leaf where the walk meets it.  By default the ordered
 * walk parks a leaf and runs the parked leaves of a wave together (DESIGN.md §Ordered walk,
 * parked leaves); the closest hits are the same, but the node/prim counts then depend on which rays
 * share a wave.  This flag makes them a per-ray property (the oracle's diagnostic walk). */
#define CPT_TRAVERSAL_PLAIN_LEAVES 0x400u
/* Megakernel pixel schedule: a short pilot render (1..4 passes from the current RNG states,
 * nothing written back) measures each 8x8 tile's work, and the render then dequeues the tiles
 * heaviest first (longest processing time first).  Results are identical to the row-major
 * tile order (a pixel's stream depends only on (seed, x, y)); the heaviest pixel chains start
 * at once, which shortens the tail when the image has few pixels per lane (row tiles on many
 * GPUs, DESIGN.md §Cost schedule).  Ignored by CPT_PATH_WAVEFRONT. */
#define CPT_SCHEDULE_COST 0x800u
/* Megakernel tail consolidation: once the pixel queue is drained, the
 * waves of a workgroup hand their chains over at pass boundaries so that each SIMD runs fewer,
 * fuller waves while chains finish.  Identical results.  By default it runs when spp >= 512 and
 * the frame holds more than 1 and at most 4 pixels per lane of the persistent grid (a
 * strong-scaled row tile on 2-7 GPUs at 1080p);
 * these flags force it on or off (on needs spp > 1).  Only the 4-wide walk consolidates
 * (CPT_TRAVERSAL_ORDERED with a 4-wide walk tree, cpt_get_walk_info [2] > 0).  A hand-over that
 * cannot complete ends the render with CPT_ERR_DEVICE, never with silently missing pixels. */
#define CPT_SCHEDULE_CONSOLIDATE    0x1000u
#define CPT_SCHEDULE_NO_CONSOLIDATE 0x2000u
/* Megakernel pixel schedule without a pilot, for renders of few passes that repeat over the
 * same frame (the DispatchRay loop, path_tracer.cu:256-306): the tiles are dequeued heaviest
 * first by the work of the context's PREVIOUS render with this flag -- each tile's RNG draws,
 * read off the XORWOW Weyl counters (d advances by 362437 per draw), which follow the path
 * lengths -- and the first render in a frame uses the row-major order.  Identical results;
 * ignored with CPT_SCHEDULE_COST and by CPT_PATH_WAVEFRONT. */
#define CPT_SCHEDULE_PREVIOUS       0x4000u

int cpt_abi_version(void);
const char* cpt_status_string(int status);
int cpt_get_device_count(int* count);

int cpt_create(int device, cpt_ctx** out);
int cpt_destroy(cpt_ctx* ctx);
/* Last error message of ctx (or of the last failed cpt_create when ctx is NULL). */
const char* cpt_last_error(const cpt_ctx* ctx);
/* Launch on `hip_stream` (a hipStream_t) instead of the context's own stream; NULL restores it.
 * Ordering rule: when the call changes the stream in use, everything the context has queued on the
 * stream it leaves runs before anything it queues on the new one afterwards (an event recorded on
 * the old stream that the new one waits for; no host wait), so a render in flight and the next
 * call never share the accumulator, the RNG planes or the dequeue word, and a synchronising call
 * after the switch also waits for the old stream's work.  The stream being left must still exist
 * at the call (restore NULL before destroying a stream of yours).  Naming the stream already in
 * use changes nothing. */
int cpt_set_stream(cpt_ctx* ctx, void* hip_stream);

/* Host-side MotionalCamera::GetCopy: computes the basis and corner vectors, increments
 * cur_sample_idx (motional_camera.cu:177-200). */
int cpt_camera_get_copy(cpt_camera* cam);

/* Builds the reference's median-split BVH over `objs` (objects copied by value, like
 * bvh.cu:43) and uploads it.  n_objs may be 0 (every ray misses). */
int cpt_set_scene(cpt_ctx* ctx, const cpt_object* objs, int n_objs);
/* Replace object `index` (AddObject order) and refit the ancestors' boxes. */
int cpt_update_object(cpt_ctx* ctx, int index, const cpt_object* obj);
/* The same for n objects at once (SceneBVH::UpdateObject, bvh.cu:122-157), refit on the GPU:
 * the host names the updated leaves and their ancestors (O(n x depth)), kernels rewrite the
 * boxes bottom-up in every device copy of both trees (reference order, walk orders, 4-wide
 * image); topology as built.  The refit is a function of the leaves only, so the result equals
 * n single updates in any order (a repeated index: the last object wins).  Returns after the
 * device copies are updated.  An edit that turns an object into a platform or back rebuilds
 * like cpt_update_objects_rebuild. */
int cpt_update_objects(cpt_ctx* ctx, int n, const int* indices, const cpt_object* objs);
/* The same edits, with the ordered walk's SAH tree rebuilt from the edited objects on the host
 * and all orders re-linearised and uploaded (the reference order is refit either way): restores
 * the walk tree's quality after large motions.  Same images. */
int cpt_update_objects_rebuild(cpt_ctx* ctx, int n, const int* indices, const cpt_object* objs);
/* Material slots the scene holds (deduplicated per value, cpt_set_scene; a device refit that
 * gives objects new materials appends slots, and once more than twice the referenced ones
 * (+ 16) are held, the unreferenced slots are dropped with a rebuild). */
int cpt_get_material_count(cpt_ctx* ctx, int* n);
/* Host wall time of the last cpt_update_objects[_rebuild] call, ms. */
int cpt_last_update_ms(cpt_ctx* ctx, float* ms);
/* Exports the BVH in the reference's node order (Divide creation order): per node
 * boxes[6] = {min xyz, max xyz}, links[4] = {is_object, left, right, object index}. */
int cpt_scene_bvh_export(cpt_ctx* ctx, float* boxes, int32_t* links, int capacity, int* n_nodes);
/* Same BVH build without a context or a GPU (host only), same export format. */
int cpt_bvh_build_host(const cpt_object* objs, int n_objs, float* boxes, int32_t* links, int capacity, int* n_nodes);

/* Environment map, RGBA8 rows of `valid_cols` texels (the reference uploads only
 * logical_width/4 texels per row, textures.cu:32-33; texels at x >= valid_cols read 0).
 * Sampler: normalized coords, mirror addressing, bilinear, c/255 (textures.cu:36-44).
 * Ordering rule: waits for the context's queued work before the texels are replaced, so a render
 * launched without CPT_RENDER_SYNC keeps the sky it was launched with, and the next one has the
 * new sky. */
int cpt_set_env_texture(cpt_ctx* ctx, const uint8_t* rgba, int logical_width, int height, int valid_cols);

/* cudaTextureAddressMode / cudaTextureFilterMode values of AddTexByFile's arguments. */
#define CPT_ADDRESS_WRAP   0
#define CPT_ADDRESS_CLAMP  1
#define CPT_ADDRESS_MIRROR 2   /* AddTexByFile's default */
#define CPT_ADDRESS_BORDER 3   /* border colour 0 */
#define CPT_FILTER_POINT   0
#define CPT_FILTER_LINEAR  1   /* AddTexByFile's default */

/* Binds texels to a material texture handle (replacing an earlier binding).  A textured
 * material (have_tex != 0) takes its diffuse colour from the texture bound to u.tex:
 * GetKd is always called at normalized (0, 0) (material.cu:31,56,95,140 pass no uv), so
 * the colour is that one sample, taken once per material when the scene is prepared.
 * Emission keeps reading kd_, i.e. the bits of the handle, as the reference's union does
 * (material.cu:36).  Layout as cpt_set_env_texture; a material whose handle is unbound
 * makes cpt_set_scene / cpt_render fail with CPT_ERR_INVALID_ARG.  Binding after
 * cpt_set_scene re-prepares the materials. */
int cpt_bind_texture(cpt_ctx* ctx, uint64_t handle, const uint8_t* rgba, int logical_width, int height,
                     int valid_cols, int address_mode, int filter_mode);

/* Per-pixel buffers for a width x height frame; the context renders the global image rows
 * listed in `rows` (n_rows of them; rows == NULL means 0..height-1).  Pixel i of the
 * context's buffers is (x = i % width, y = rows[i / width]). */
int cpt_set_frame(cpt_ctx* ctx, int width, int height, const int32_t* rows, int n_rows);
/* curand_init(seed, (x << 32) | y, 0) for every pixel of the context (InitCuRand). */
int cpt_init_rng(cpt_ctx* ctx, uint64_t seed);
int cpt_read_rng(cpt_ctx* ctx, uint32_t* planar6);          /* [6][n_rows*width]: v0..v4, d */
int cpt_write_rng(cpt_ctx* ctx, const uint32_t* planar6);

/* `spp` SamplePixel passes for every pixel of the context, each pass continuing the
 * pixel's XORWOW stream; the accumulator holds rgb sums + pass count per pixel.
 * max_depth in [0, 32] (MAX_RECURSION_DEPTH_SET, path_tracer.h:13).  Asynchronous unless
 * CPT_RENDER_SYNC. */
int cpt_render(cpt_ctx* ctx, const cpt_camera* cam, int spp, int max_depth, uint32_t flags);
int cpt_synchronize(cpt_ctx* ctx);
int cpt_read_accum(cpt_ctx* ctx, float* rgba);               /* [n_rows*width][4] */
int cpt_clear_accum(cpt_ctx* ctx);
int cpt_read_aux(cpt_ctx* ctx, float* normal3, float* depth); /* either may be NULL */
/* Checkpoint / resume (the reference keeps its running state only in device memory,
 * path_tracer.cu:91-99): restore the accumulator ([rows*W][4]: rgb sums + pass count) and the
 * first-hit normal / depth buffers from host copies made with cpt_read_accum / cpt_read_aux.
 * With cpt_write_rng, a render (and the display path) resumes bit for bit. */
int cpt_write_accum(cpt_ctx* ctx, const float* rgba);
int cpt_write_aux(cpt_ctx* ctx, const float* normal3, const float* depth);
/* The cost schedule's pilot alone (for cost-balanced row partitions across ranks, tiling.py):
 * `passes` passes from the context's current RNG states (nothing is written back), the work of
 * each 8x8 tile's heaviest pixel -- its segments + node visits + primitive tests, the walk of
 * `flags`' CPT_TRAVERSAL_* bits; the maximum over the tile's pixels, not their sum -- into
 * out[tile] (tiles row-major over the context's rows: ((n_rows+7)/8) x ((width+7)/8); n_out at
 * least that).  Synchronous. */
int cpt_tile_costs(cpt_ctx* ctx, const cpt_camera* cam, int passes, int max_depth, uint32_t flags, uint32_t* out,
                   size_t n_out);
/* Top-up render (an addition: the reference gives every pixel the same passes,
 * path_tracer.cu:124-175).  Every pixel of the context runs d further SamplePixel passes, d its
 * deficit to `target`: with count the pixel's accumulator count (its .w), d = target - (int)count
 * (truncation) when count is finite and 0 <= count < target, else 0 (at or past the target,
 * negative, NaN, +-inf).  The passes continue the pixel's XORWOW stream and add to its accumulator
 * exactly as a cpt_render of d passes with CPT_RENDER_ACCUMULATE would for that pixel.  A pixel with
 * d == 0 is not written at all: its accumulator, RNG words and (CPT_RENDER_AUX) first-hit normal
 * and depth keep their bits.  Meant for the frame cpt_reproject_accum[_tracked] leaves, whose
 * counts are uneven: the passes go to the disoccluded pixels instead of to every pixel alike.
 *
 * One plan and one megakernel launch on the context's stream, no host wait: each 8x8 tile is keyed
 * by its largest deficit, the tiles are sorted by key (descending, ties row-major), and the launch
 * dequeues the tiles with a deficit in that order, their number read from device memory.
 * target in [1, 2^20], max_depth in [0, 32], else CPT_ERR_INVALID_ARG.  flags: CPT_TRAVERSAL_*,
 * CPT_RENDER_STATS, CPT_RENDER_AUX, CPT_RENDER_SYNC; CPT_RENDER_ACCUMULATE is implied and may be
 * passed.  CPT_ERR_UNSUPPORTED: CPT_PATH_WAVEFRONT, CPT_SCHEDULE_PREVIOUS, CPT_SCHEDULE_COST,
 * CPT_SCHEDULE_CONSOLIDATE (a top-up launch never consolidates).  State errors as cpt_render's, and
 * CPT_ERR_STATE while an adaptive render is pending; nothing is written on an error.  Works on
 * row-tiled contexts as cpt_render does.  Like cpt_render it leaves an adaptive result's moments,
 * the display state, the G-buffer and the reprojection history as they were.  Asynchronous unless
 * CPT_RENDER_SYNC; cpt_last_render_ms covers the plan and the launch, cpt_last_kernel_stats the
 * launch alone. */
int cpt_render_to_count(cpt_ctx* ctx, const cpt_camera* cam, int target, int max_depth, uint32_t flags);
/* The last cpt_render_to_count's plan since cpt_set_frame (CPT_ERR_STATE if none; an addition: the
 * reference gives every pixel the same passes): the 8x8 tiles with a deficit, the pixels with a
 * deficit and the sum of the deficits (the passes the call runs).  Each output may be NULL.  Waits
 * for the call. */
int cpt_topup_info(cpt_ctx* ctx, uint32_t* tiles, uint64_t* pixels, uint64_t* passes);
/* HOST ONLY, no GPU: the deficit rule above, the function the device runs (an addition: the
 * reference gives every pixel the same passes).  target outside [1, 2^20] or a NULL d:
 * CPT_ERR_INVALID_ARG. */
int cpt_topup_deficit_host(float count, int target, int* d);
/* Adaptive render (an addition: the reference gives every pixel the same passes,
 * path_tracer.cu:124-175).  Rounds of `batch` passes; after a round every 8x8 tile whose pixels
 * have all converged leaves the list of tiles the next round renders, and so does every tile at
 * max_spp.  A pixel's estimate is the luminance (0.2126, 0.7152, 0.0722) of each round's batch
 * mean; it has converged when the standard error of the mean of its k >= 2 batch means is at most
 * rel_error * max(mean, 1e-3) (a NaN never converges).  No tile leaves before min_spp passes.
 *
 * Every pixel's accumulator (rgb sums and count) and RNG state end bit for bit as a cpt_render of
 * that pixel's own number of passes leaves them: each round is cpt_render's launch of `batch`
 * passes with `flags` (CPT_TRAVERSAL_*, CPT_RENDER_STATS, CPT_RENDER_AUX, CPT_SCHEDULE_[NO_]
 * CONSOLIDATE; CPT_SCHEDULE_COST runs its pilot once, before round 1, and the rounds filter that
 * order).  Without CPT_RENDER_ACCUMULATE round 1 overwrites the accumulator; with it the estimate
 * starts from the current accumulator (a resumed render starts a new estimate).  Counts are per
 * pixel, which cpt_gather_rows, cpt_denoise_mix, cpt_read_accum and cpt_write_accum already
 * expect: they need no change.
 * Rules (else CPT_ERR_INVALID_ARG): batch >= 1; min_spp and max_spp multiples of batch;
 * batch <= min_spp <= max_spp; min_spp >= 2 * batch unless min_spp == max_spp; rel_error >= 0.
 * CPT_ERR_UNSUPPORTED: CPT_PATH_WAVEFRONT, CPT_SCHEDULE_PREVIOUS.  Synchronous: the list's length
 * is read back after every round (cpt_adaptive_begin, then cpt_adaptive_step until it gives 0). */
int cpt_render_adaptive(cpt_ctx* ctx, const cpt_camera* cam, int min_spp, int max_spp, int batch, float rel_error,
                        int max_depth, uint32_t flags);
/* The adaptive render in two calls, for a caller that drives several contexts from one thread (row
 * tiles on several devices): cpt_adaptive_begin checks what cpt_render_adaptive checks, queues round
 * 1 with the read-back of its result on the context's stream and returns without waiting.
 * cpt_adaptive_step waits for the queued round's read-back alone (an event behind it), records the
 * round, and either queues the next round and returns the tiles it renders in *active_tiles, or,
 * when no tile is left, ends the render and returns 0 there; a context without rows ends at its
 * first step.  Call begin on every context, then step the unfinished ones in turn: every device
 * then has a round queued while the host waits on another.  The result is cpt_render_adaptive's.
 * Pending state: between a successful begin and the step that returns 0 the rounds own the
 * frame's buffers, and cpt_render, cpt_render_adaptive, cpt_adaptive_begin, cpt_set_frame,
 * cpt_filter_frame and cpt_gather_rows (the context as source or destination) return
 * CPT_ERR_STATE; so does cpt_adaptive_step with nothing pending, and the read-outs of an adaptive
 * result (there is none yet).  A step that fails ends the render: nothing is pending and the frame
 * holds no adaptive result.  cpt_destroy waits for a pending context's stream and frees it. */
int cpt_adaptive_begin(cpt_ctx* ctx, const cpt_camera* cam, int min_spp, int max_spp, int batch, float rel_error,
                       int max_depth, uint32_t flags);
int cpt_adaptive_step(cpt_ctx* ctx, int* active_tiles);
/* The last adaptive render since cpt_set_frame (CPT_ERR_STATE if none).  cpt_read_noise: each
 * pixel's relative standard error as its last round left it (the criterion's left side over its
 * right side's max(mean, 1e-3); +inf with fewer than two batch means), [n_rows*width], capacity in
 * floats.  cpt_adaptive_info: the rounds run, the tiles each one rendered (the first `capacity` of
 * them), and the pixel passes of all rounds; each output may be NULL. */
int cpt_read_noise(cpt_ctx* ctx, float* rel, size_t capacity);
int cpt_adaptive_info(cpt_ctx* ctx, int* rounds, uint32_t* active_tiles_per_round, int capacity,
                      uint64_t* passes_done);
/* HOST ONLY, no GPU: the criterion on a pixel's moments (m1 = sum of its k batch means, m2 = sum
 * of their squares) at rel_error t, the function the device runs. */
int cpt_adaptive_decide_host(float m1, float m2, float k, float t, int* converged, float* rel);
/* The adaptive render's per-pixel moments, planar [4][n_rows*width]: m1 (the sum of the pixel's k
 * batch means' luminance), m2 (the sum of their squares), k, rel (cpt_read_noise's plane);
 * capacity / count in floats, at least 4 * n_rows * width (else CPT_ERR_INVALID_ARG, nothing
 * written).  With cpt_read/write_accum, _rng and _aux they complete the checkpoint of an adaptive
 * session: cpt_write_moments marks the frame as holding an adaptive result with an empty round
 * record (cpt_adaptive_info: 0 rounds, 0 passes), so cpt_read_noise and cpt_filter_frame work on a
 * restored frame.  cpt_read_moments before either: CPT_ERR_STATE.  The moments of a render resumed
 * with CPT_RENDER_ACCUMULATE describe only the passes of that call, not the accumulator's earlier
 * ones; a plain cpt_render leaves them as they were. */
int cpt_read_moments(cpt_ctx* ctx, float* planar4, size_t capacity);
int cpt_write_moments(cpt_ctx* ctx, const float* planar4, size_t count);

/* Variance-guided a-trous filter of the frame an adaptive render left (an addition: the
 * reference's only filter is the per-pass Denoising + Mix, path_tracer.cu:177-254):
 * `levels` iterations (0..8) of a 5x5 B3-spline stencil at step 1, 2, 4, ... over the mean image
 * accumulator rgb / count, each tap weighted by the first-hit normals' agreement (max(Np.Nq, 0)
 * squared normal_sharpness_log2 times, 0..10) and by den / (den + d^2), d the luminance
 * difference and den = sigma_l^2 x the 3x3-prefiltered variance of the mean + 1e-10 (sigma_l
 * finite and >= 0); the variance of the mean (from the moments) is propagated through every level.
 * A pixel without a pass, with fewer than two batch means or with a value that is not finite is
 * left as it is and is no tap of another pixel.  Defaults in the wrappers: 5 levels, sigma_l 1,
 * sharpness 7 (the measurements behind sigma_l).  Bad arguments: CPT_ERR_INVALID_ARG.
 * Needs (else CPT_ERR_STATE) a full frame (rows == NULL, as cpt_denoise_mix), moments
 * (cpt_render_adaptive or cpt_write_moments) and first-hit normals (CPT_RENDER_AUX or
 * cpt_write_aux).  A row-tiled adaptive render is filtered on the frame context its tiles were
 * gathered into: cpt_gather_rows carries the moments.  Reads the accumulator, the moments and the normals and writes none of them (nor
 * the RNG); the result lives in buffers of its own until the next call or cpt_set_frame.
 * Asynchronous, on the context's stream. */
int cpt_filter_frame(cpt_ctx* ctx, int levels, float sigma_l, int normal_sharpness_log2);
/* The last cpt_filter_frame's result (CPT_ERR_STATE if none since cpt_set_frame): rgb
 * [n_rows*width][3] and the variance of the filtered mean [n_rows*width]; either may be NULL.
 * capacity_pixels below n_rows*width: CPT_ERR_INVALID_ARG, nothing written.  Waits. */
int cpt_read_filtered(cpt_ctx* ctx, float* rgb, float* variance, size_t capacity_pixels);
/* Device time of the last cpt_filter_frame, all its launches (HIP events on the context's stream);
 * waits for it. */
int cpt_last_filter_ms(cpt_ctx* ctx, float* ms);
/* HOST ONLY, no GPU: the functions the device runs.  cpt_filter_prepare_host: level 0 of npix
 * pixels from an accumulator [npix][4] and moments [4][npix] into out_rgbv [npix][4] (mean rgb,
 * variance of the mean) and out_valid [npix] (1 or 0).  cpt_filter_level_host: one level at
 * `step` (1..128) of a width x height plane in_rgbv with normals normal3 [npix][3] and validity
 * `valid` into out_rgbv (not in place). */
int cpt_filter_prepare_host(size_t npix, const float* accum_rgba, const float* moments_planar4, float* out_rgbv,
                            uint8_t* out_valid);
int cpt_filter_level_host(int width, int height, int step, const float* in_rgbv, const float* normal3, const uint8_t* valid,
                          float sigma_l, int normal_sharpness_log2, float* out_rgbv);
/* The same filter for a frame without moments: a plain cpt_render, a reprojected frame, one that
 * cpt_render_to_count topped up (an addition).  It reads the accumulator and the
 * frame's G-buffer (id and normal planes) and needs neither moments nor aux normals.  Level 0's
 * variance of the mean is spatial: over the 7x7 window of a pixel, among the pixels of the same
 * object id that hold a finite mean, the count-weighted variance of the luminance, each tap weighted
 * by the normals' agreement as above, scaled to the pixel's own count (0 for a pixel alone in its
 * window).  A pixel without a pass or with a value that is not finite is left as it is and is no
 * tap of another pixel.  The levels are cpt_filter_frame's, guided by the G-buffer's normals, with
 * one more stop: a tap of another object id is skipped, in the 3x3 variance prefilter too.
 * Argument ranges and CPT_ERR_INVALID_ARG as cpt_filter_frame.  CPT_ERR_STATE: no frame, a frame
 * that is not full (rows != NULL), no valid G-buffer, or an adaptive render pending.
 * THE G-BUFFER MUST BE THE ONE OF THE CAMERA THE ACCUMULATOR NOW BELONGS TO.  After any
 * cpt_reproject_* call it is (they leave `to`'s, and cpt_render_to_count keeps it); after a plain
 * cpt_render the caller runs cpt_gbuffer at the render's camera first.  The call cannot check this.
 * Writes only the filter's own planes (cpt_read_filtered and cpt_last_filter_ms serve both filters;
 * a call that fails its checks leaves an earlier result readable).  Asynchronous, on the context's
 * stream; no allocation after the frame's first filter call.  Defaults in the wrappers: 3 levels,
 * sigma_l 2, sharpness 3 (the sweep behind them). */
int cpt_filter_frame_spatial(cpt_ctx* ctx, int levels, float sigma_l, int normal_sharpness_log2);
/* HOST ONLY, no GPU: the functions cpt_filter_frame_spatial's kernels run.
 * cpt_filter_prepare_spatial_host: level 0 of a width x height frame from an accumulator [npix][4]
 * and the G-buffer's id [npix] and normal3 [npix][3] into out_rgbv and out_valid, as
 * cpt_filter_prepare_host's.  cpt_filter_level_id_host: cpt_filter_level_host with the stop at
 * object boundaries of `id` [npix]. */
int cpt_filter_prepare_spatial_host(int width, int height, const float* accum_rgba, const int32_t* id, const float* normal3,
                                    int normal_sharpness_log2, float* out_rgbv, uint8_t* out_valid);
int cpt_filter_level_id_host(int width, int height, int step, const float* in_rgbv, const float* normal3, const int32_t* id,
                             const uint8_t* valid, float sigma_l, int normal_sharpness_log2, float* out_rgbv);
/* First-hit queries (additions: the reference has no counterpart; its only first-hit data are the
 * normal and the constant depth 1e30 that SamplePixel writes, path_tracer.cu:172-174, and nothing
 * in it names the object a ray hits).  All of them walk SceneBVH::TraceRay
 * (bvh.cu:167-205) exactly as cpt_render's first segment does under the same `flags`, of which only
 * the CPT_TRAVERSAL_* bits are accepted (any other bit: CPT_ERR_INVALID_ARG).  They read the scene
 * and the camera and write none of the accumulator, RNG states, aux buffers, moments, filter planes
 * or display state; no RNG draw is made.  Per ray: the object's index in cpt_set_scene's (AddObject)
 * order, the winning intersector's distance t, the normal the reference's intersector forms, and
 * the material's GetKd(0, 0) (material.cu:11-18).  A miss gives -1, t = 1e30 (DEFAULT_RAY_TMAX), the
 * normal -dir (the integrator's Miss convention) and albedo 0.  The indices stay AddObject indices
 * through cpt_update_objects and cpt_update_objects_rebuild.  A missing scene (or, for cpt_gbuffer
 * and cpt_pick, frame): CPT_ERR_STATE; a NULL required pointer: CPT_ERR_INVALID_ARG; nothing is
 * written in either case.
 *
 * cpt_gbuffer: the G-buffer of the context's pixels, pixel i = (i % width, rows[i / width]) as in
 * cpt_set_frame.  A pixel's ray is RayGen's (motional_camera.cu:202-213) with the lens offset taken
 * as zero: the ray cpt_render shoots when lens_radius == 0, and the centre ray of a defocused
 * camera.  The camera must have the frame's size.  The result lives in buffers of its own on the
 * frame, allocated at the first call and dropped by cpt_set_frame.  Asynchronous, on the context's
 * stream; CPT_ERR_STATE while an adaptive render is pending. */
int cpt_gbuffer(cpt_ctx* ctx, const cpt_camera* cam, uint32_t flags);
/* The last cpt_gbuffer's result, or the G-buffer at `to` of a later cpt_reproject_accum
 * (CPT_ERR_STATE if neither since cpt_set_frame): id [n_rows*width], t
 * [n_rows*width], normal3 and albedo3 [n_rows*width][3]; any may be NULL.  capacity_pixels below
 * n_rows*width: CPT_ERR_INVALID_ARG, nothing written.  Waits. */
int cpt_read_gbuffer(cpt_ctx* ctx, int32_t* id, float* t, float* normal3, float* albedo3, size_t capacity_pixels);
/* The other half, with cpt_write_accum, cpt_write_rng, cpt_write_aux and cpt_write_moments the
 * checkpoint of a session: restores the G-buffer's planes from host copies of count_pixels pixels
 * each and makes the G-buffer valid (cpt_read_gbuffer and cpt_filter_frame_spatial then work).  A
 * NULL plane is left as it is, and is zero if it was never written.  Needs a frame (CPT_ERR_STATE);
 * count_pixels below n_rows*width: CPT_ERR_INVALID_ARG, nothing written.  Waits for the stream
 * first, as cpt_write_moments does. */
int cpt_write_gbuffer(cpt_ctx* ctx, const int32_t* id, const float* t, const float* normal3, const float* albedo3,
                      size_t count_pixels);
/* n rays from host arrays origin3 / dir3 [n][3] and tmin [n] (NULL: 0 for every ray) into the host
 * arrays id [n], t [n] and normal3 [n][3].  The direction is used as given, not normalised, as
 * TraceRay does (t is in units of its length; a miss's normal is -dir as given); tmax is 1e30.
 * Needs only a scene.  Synchronous; the device staging is sized before the launch. */
int cpt_trace_rays(cpt_ctx* ctx, size_t n, const float* origin3, const float* dir3, const float* tmin, uint32_t flags,
                   int32_t* id, float* t, float* normal3);
/* The object under pixel (x, y) of the image (0 <= x < width, 0 <= y < height, else
 * CPT_ERR_INVALID_ARG) and, when t is not NULL, its distance: cpt_gbuffer's id and t of that
 * pixel, by one ray.  *object = -1 and *t = 1e30 on a miss.  Synchronous. */
int cpt_pick(cpt_ctx* ctx, const cpt_camera* cam, int x, int y, uint32_t flags, int32_t* object, float* t);
/* Device time of the last cpt_gbuffer, cpt_trace_rays or cpt_pick kernel (HIP events on the
 * context's stream); waits for it. */
int cpt_last_query_ms(cpt_ctx* ctx, float* ms);
/* Reprojection of the accumulated frame to a moved camera (an addition: the reference throws the
 * history away when the camera moves, MotionalCamera::Refresh and Mix restarting at 1 / 1;
 * DESIGN.md §21).  `from` is the camera the accumulator was rendered with, `to` the new one, both
 * after cpt_camera_get_copy and of the frame's size.  For every pixel of `to` the call looks up its
 * first hit (for the sky: its direction, a point at infinity, so the sky follows rotations only) in
 * the frame as `from` saw it, blends the four accumulator pixels around that position bilinearly
 * (positions within 1/32 of a pixel snap to it) and keeps a tap only if it holds at least one pass
 * and finite rgb, saw the same object, and its own hit point lies within plane_tol x the new hit's
 * distance of the new hit's tangent plane.  The means and the pass counts are blended apart: a
 * pixel ends as (mean x n, n) with n = floor(min(blended count, max_history)), an integer as every
 * consumer of the accumulator expects, or as (0, 0, 0, 0) where less than 1/64 of the bilinear
 * weight was valid (disocclusions, the frame's new border): the next CPT_RENDER_ACCUMULATE render
 * starts those pixels afresh.  A pixel that maps exactly onto a valid old pixel of at most
 * max_history passes keeps that pixel's four floats unchanged, so from == to leaves such an
 * accumulator bit for bit as it was.
 * The call traces the G-buffer at `from` into history planes of its own and the G-buffer at `to`
 * into the frame's ordinary G-buffer (cpt_read_gbuffer afterwards returns `to`'s), both by
 * the walk of `flags` (CPT_TRAVERSAL_* bits only), then runs the look-up into a second plane that
 * becomes the accumulator.  It writes the accumulator and the G-buffer and nothing else of the
 * render state (RNG states, aux buffers, display state and filter planes stay), and drops the
 * frame's adaptive result, whose moments no longer describe the accumulator: cpt_read_noise,
 * cpt_read_moments and cpt_filter_frame return CPT_ERR_STATE until the next adaptive render or
 * cpt_write_moments.  Asynchronous, on the context's stream, ordered like every other call; its
 * planes are allocated at the first call and dropped by cpt_set_frame.
 * CPT_ERR_STATE: no scene, no frame, a frame that is not full (rows == NULL, as cpt_filter_frame;
 * a row-tiled render reprojects on the context its tiles were gathered into), an adaptive render
 * pending.  CPT_ERR_INVALID_ARG: a NULL camera, a camera of another size, max_history < 1, a
 * plane_tol that is negative or not finite, a flag bit outside CPT_TRAVERSAL_*.  Nothing is written
 * on an error.
 * Limits.  Static scene: both traces walk the current scene, so after cpt_update_objects the caller
 * clears the accumulator, accepts stale history on the moved objects, or uses the tracked calls
 * below (cpt_history_capture, cpt_reproject_accum_tracked).  Outgoing radiance is
 * reused as if it did not depend on the view: mirrors and glass lag until new passes outweigh
 * max_history.  The wrappers' defaults are max_history 32 and plane_tol 1e-2. */
int cpt_reproject_accum(cpt_ctx* ctx, const cpt_camera* from, const cpt_camera* to, int max_history, float plane_tol,
                        uint32_t flags);
/* Device time of the last cpt_reproject_accum, all its launches (HIP events on the context's
 * stream); waits for it.  cpt_last_reproject_launch_ms: the same split into ms3[0..2], the trace
 * at `from`, the trace at `to` and the look-up kernel. */
int cpt_last_reproject_ms(cpt_ctx* ctx, float* ms);
int cpt_last_reproject_launch_ms(cpt_ctx* ctx, float* ms3);
/* HOST ONLY, no GPU: the function the device runs, on a width x height frame.  cam0 / cam1: the
 * old and the new camera (after cpt_camera_get_copy, of that size); dir0 / dir1 [npix][3] their
 * centre-ray directions (the G-buffer's rays); id0, t0 the G-buffer at cam0 and id1, t1, normal1
 * the G-buffer at cam1; accum_in / accum_out [npix][4] (not the same array). */
int cpt_reproject_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height, const float* dir0,
                       const float* dir1, const int32_t* id0, const float* t0, const int32_t* id1, const float* t1,
                       const float* normal1, const float* accum_in, int max_history, float plane_tol, float* accum_out);
/* Reprojection of the display state to a moved camera (an addition, DESIGN.md §22: in the
 * reference's DispatchRay loop every camera move is a MotionalCamera::Refresh and the next Mix runs
 * at 1 / 1, path_tracer.cu:241-254, so the viewer sees a raw one-sample frame).  The look-up of
 * cpt_reproject_accum, with the same arguments, geometry and tap tests, applied to the Mix running
 * mean and the per-pixel sample counts that cpt_denoise_mix_history keeps beside it, not to the
 * accumulator.  What differs: a tap counts only inside the display's launch region W' x H'
 * (16*floor(W/16) x 16*floor(H/16)), with a count of at least 1 and a finite mean; the mean is
 * blended as it is (no division by the count) and the count beside it; a pixel ends as (blended
 * mean, n) with n = floor(min(blended count, max_history)), or as (0, 0, 0; 0) where less than 1/64
 * of the bilinear weight was valid, n < 1, or the pixel lies outside W' x H'.  A pixel that maps
 * exactly onto a valid old pixel of at most max_history samples keeps its mean and count unchanged,
 * so from == to leaves such a display state bit for bit as it was.  The next
 * cpt_denoise_mix_history then mixes each pixel at 1 / (its count + 1): pixels with history keep it,
 * the others restart.
 * The call traces as cpt_reproject_accum does (cpt_read_gbuffer afterwards returns `to`'s) and
 * runs the look-up into second mean and count planes that become the display state.  It writes the
 * display's mean and counts and the G-buffer, and nothing else: the accumulator, RNG states, aux
 * buffers, moments and filter planes stay, and so does the BGRA8 frame, which changes at the next
 * display pass.  After cpt_denoise_mix calls the counts are first set to the last cur_sample_idx
 * (see cpt_denoise_mix_history).  Asynchronous, on the context's stream, ordered like every other
 * call.  cpt_last_reproject_ms and cpt_last_reproject_launch_ms time the last call of either kind.
 * Errors: cpt_reproject_accum's, and CPT_ERR_STATE when there has been no display pass since
 * cpt_set_frame or the display holds a band (cpt_denoise_mix_band) and not the full frame.
 * Nothing is written on an error.  Limits: cpt_reproject_accum's. */
int cpt_reproject_display(cpt_ctx* ctx, const cpt_camera* from, const cpt_camera* to, int max_history, float plane_tol,
                          uint32_t flags);
/* HOST ONLY, no GPU: the function cpt_reproject_display's kernel runs, shaped like
 * cpt_reproject_host: mean_in / mean_out [npix][3] and count_in / count_out [npix] (in and out
 * not the same arrays) in place of the accumulator. */
int cpt_reproject_display_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height, const float* dir0,
                               const float* dir1, const int32_t* id0, const float* t0, const int32_t* id1, const float* t1,
                               const float* normal1, const float* mean_in, const float* count_in, int max_history,
                               float plane_tol, float* mean_out, float* count_out);
/* Tracked reprojection: the history kept through object edits as well as camera moves (an addition,
 * DESIGN.md §23; CPT_ABI_VERSION stays 1).  cpt_reproject_accum and cpt_reproject_display trace the
 * G-buffer at `from` in the current scene, which is wrong once an object has moved.  Here the
 * history's G-buffer is kept instead, with its camera and the objects as they were:
 *   cpt_history_capture(cam)        once, after rendering at cam: traces cam's G-buffer in the
 *                                   current scene (cpt_read_gbuffer afterwards returns it), copies
 *                                   its id and distance planes to the history's, remembers cam and
 *                                   snapshots the objects.  Writes nothing else.
 *   cpt_update_objects(...)         any number of edits, or none
 *   cpt_reproject_accum_tracked(to) / cpt_reproject_display_tracked(to)
 *                                   one trace, at `to` in the current scene, into the frame's
 *                                   G-buffer; then the look-up of the untracked call with one
 *                                   change: a new hit point P on object k is first mapped to the
 *                                   point P0 that object k held at the capture (cpt_object_motion),
 *                                   P0 is projected into the captured camera, and a tap's own old
 *                                   hit point is tested against the plane through P0 with the new
 *                                   normal (all the mappings keep normals).  Objects of kind
 *                                   CPT_MOTION_DROP end as zeros.  Sky pixels as in the untracked
 *                                   call.  Then `to`, its id and distance planes (the look-up
 *                                   kernel writes them to the history's second planes, which are
 *                                   swapped in: a ping-pong, no extra launch) and the current
 *                                   objects become the captured history: the next move again
 *                                   costs one trace.
 * With no edit since the capture the results are bit for bit those of cpt_reproject_accum(captured
 * cam, to) / cpt_reproject_display(captured cam, to), and no motion table is uploaded.
 * Side effects, asynchrony, argument checks and errors are the untracked calls' (nothing is written
 * on an error; the display variant keeps its "no display pass yet" and band errors), and
 * CPT_ERR_STATE when no history is captured.  cpt_set_scene and cpt_set_frame drop the captured
 * history, and so do cpt_reproject_accum and cpt_reproject_display, which trace their `from` into the
 * history's planes: a tracked call after an untracked one needs a new cpt_history_capture.  The
 * captured history describes one frame: the caller applies it to the accumulator or display state
 * that was rendered at the captured camera with the captured objects (cpt_history_info returns the
 * camera), and captures again after rendering elsewhere without a tracked call; cpt_update_object(s) and cpt_update_objects_rebuild keep it (ids are AddObject indices
 * through both).  cpt_last_reproject_ms / _launch_ms time tracked calls too; ms3[0], the trace that
 * did not run, reads 0.  A call after an edit derives the motion table on the host and uploads it
 * on the stream from one of two host copies used by turns; it waits on the host only for the upload
 * of the edited call before the last, if that is still queued.
 * Limits.  Only first-hit geometry is followed: a moved object's shadow and its reflection in
 * other objects lag until new passes outweigh max_history, as view-dependent radiance does in the
 * untracked calls.  No rotation (the primitives have none), no texture-coordinate changes, one
 * device, full frames. */
enum cpt_motion_kind {
    CPT_MOTION_SAME = 0,      /* geometry and material bytewise equal: P0 = P, untouched */
    CPT_MOTION_SPHERE = 1,    /* P0 = c0 + (P - c1) * (r0 / r1) */
    CPT_MOTION_CYLINDER = 2,  /* x, z as the sphere; y: c0.y + (P.y - c1.y) * (h0 / h1) */
    CPT_MOTION_PLATFORM = 3,  /* P0 = (P.x, y_pos0, P.z) */
    CPT_MOTION_DROP = 4       /* no history: the type or any material field changed, a radius or
                               * height used as a divisor is not finite or <= 0, or a scale is not
                               * finite */
};
/* One object's motion since the capture, 40 bytes: c0 / c1 the centre then and now (a platform:
 * y = its y_pos), s_xz = r0 / r1 and s_y = h0 / h1 (a sphere: r0 / r1), each formed once. */
typedef struct cpt_object_motion {
    int32_t kind;              /* @0  cpt_motion_kind */
    cpt_float3 c0;             /* @4  */
    cpt_float3 c1;             /* @16 */
    float s_xz;                /* @28 */
    float s_y;                 /* @32 */
    int32_t pad_;              /* @36 */
} cpt_object_motion;
int cpt_history_capture(cpt_ctx* ctx, const cpt_camera* cam, uint32_t flags);
int cpt_reproject_accum_tracked(cpt_ctx* ctx, const cpt_camera* to, int max_history, float plane_tol, uint32_t flags);
int cpt_reproject_display_tracked(cpt_ctx* ctx, const cpt_camera* to, int max_history, float plane_tol, uint32_t flags);
/* Whether a history is captured (*valid 0 / 1) and, when cam is not NULL and one is, its camera. */
int cpt_history_info(cpt_ctx* ctx, int* valid, cpt_camera* cam);
/* HOST ONLY, no GPU: the motion table of n objects as captured (old_objs) and as they are now
 * (new_objs), out_table [n]; and the functions the tracked kernels run, shaped like
 * cpt_reproject_host / cpt_reproject_display_host with the table of n_objs records (NULL with 0:
 * nothing moved).  An id1 outside [0, n_objs) with a table: CPT_ERR_INVALID_ARG. */
int cpt_object_motion_host(const cpt_object* old_objs, const cpt_object* new_objs, int n, cpt_object_motion* out_table);
int cpt_reproject_tracked_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height, const float* dir0,
                               const float* dir1, const int32_t* id0, const float* t0, const int32_t* id1, const float* t1,
                               const float* normal1, const float* accum_in, const cpt_object_motion* table, int n_objs,
                               int max_history, float plane_tol, float* accum_out);
int cpt_reproject_display_tracked_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height,
                                       const float* dir0, const float* dir1, const int32_t* id0, const float* t0,
                                       const int32_t* id1, const float* t1, const float* normal1, const float* mean_in,
                                       const float* count_in, const cpt_object_motion* table, int n_objs, int max_history,
                                       float plane_tol, float* mean_out, float* count_out);
/* Device-to-device copy of the accumulator (e.g. into an RCCL send buffer), ordered against the
 * caller's HIP stream `caller_stream` (NULL: the null stream) without blocking the host: the
 * context's stream first waits for the work queued on caller_stream so far (a fill of dst, a
 * collective still reading it), then copies, and caller_stream waits for the copy (work queued on
 * it next, e.g. the all-gather, reads the copied bytes).  When caller_stream is the context's own
 * launch stream (cpt_set_stream) the copy is simply queued there.  Device errors of the render
 * surface at the next synchronising call. */
int cpt_copy_accum_device(cpt_ctx* ctx, void* device_dst, size_t bytes, void* caller_stream);
/* Row-tile gather (multi-GPU row tiling; the single-GPU reference writes the
 * whole frame from SamplePixel, path_tracer.cu:172-174): places the rows `src` rendered -- its
 * accumulator, and its first-hit normals and depths when it rendered with CPT_RENDER_AUX --
 * into `dst`'s frame at the same global rows (dst must hold every one of them, e.g. a full
 * frame).  src and dst may live on different devices (the stitch reads src over xGMI with peer
 * access, enabled once per device pair; a staged peer copy where no peer path exists) or on the
 * same one.  Asynchronous: ordered after src's queued work and before src's later work by
 * events, with no host wait, so several gathers queue back to back; dst then holds the stitched
 * frame for its next call (cpt_synchronize, cpt_read_accum, cpt_read_aux, cpt_denoise_mix).
 * src's device errors are reported by src's own next synchronising call.
 * When src holds an adaptive result (cpt_render_adaptive, the begin / step pair, or
 * cpt_write_moments) its four moment planes are placed too, by a second kernel behind the first.
 * A dst without an adaptive result of its own first gets m1 = m2 = k = 0 and +inf noise everywhere
 * (a pixel before its second batch: rows no source covers are invalid for the filter), and dst
 * then holds an adaptive result with an empty round record, as after cpt_write_moments:
 * cpt_read_noise, cpt_read_moments and cpt_filter_frame work on it.  When the tiles are whole 8-row
 * blocks in ascending order the stitched moments are those of one context's adaptive render of the
 * frame.  A src without an adaptive result leaves dst's moments alone. */
int cpt_gather_rows(cpt_ctx* dst, cpt_ctx* src);
/* How the last cpt_gather_rows(dst, src) reached src's buffers (-1: no gather of the pair yet):
 * the stitch read them in place on the same device, read them over xGMI with peer access
 * (contexts on two devices), or read a staged hipMemcpyPeerAsync copy (no peer path, or
 * forced by cpt_set_debug_gather).  No reference counterpart: a test hook for §8(e). */
#define CPT_GATHER_SAME_DEVICE 0
#define CPT_GATHER_PEER 1
#define CPT_GATHER_STAGED 2
int cpt_last_gather_mode(cpt_ctx* dst, cpt_ctx* src, int* mode);
/* TEST HOOK: force dst's gathers through the staged peer copy (the fallback for device pairs
 * without peer access), so that branch runs on a one-GPU box too. */
int cpt_set_debug_gather(cpt_ctx* dst, int force_staged);
int cpt_get_stats(cpt_ctx* ctx, cpt_stats* out);
int cpt_reset_stats(cpt_ctx* ctx);
/* All 8 raw device counters (0-4 = cpt_stats; 5 = ordered-walk segments that failed the
 * winner certificate and took the reference walk (CPT_RENDER_STATS | CPT_TRAVERSAL_ORDERED);
 * 6 = 4-wide node visits read from global memory, i.e. past the LDS image's first 512 nodes). */
int cpt_get_raw_counters(cpt_ctx* ctx, uint64_t* out8);
/* DIAGNOSTIC (a library built with CPT_TIMELINE; CPT_ERR_STATE otherwise): the megakernel's
 * lane-occupancy timeline since the last call, n words (<= 4 x 4096 + 4): per 1.31 ms bin of
 * the device's 100 MHz clock (a ring of 4096 bins) busy-lane x ticks, wave x 64 x ticks, busy-lane
 * x ticks after the pixel queue ran dry, of level-0 waves; then the first tick a wave saw the
 * queue dry.  Clears it (tools/timeline.py). */
int cpt_debug_timeline(cpt_ctx* ctx, uint64_t* out, int n);
/* DIAGNOSTIC: the 16 wave-time stamp slots of a CPT_STAMPS build (cpt_stamps.hpp; all zero in
 * the shipped library), summed over the renders since the last cpt_reset_stats. */
int cpt_get_diag_counters(cpt_ctx* ctx, uint64_t* out16);
/* DIAGNOSTIC: the exec-mask census of a CPT_EXECDIAG build (cpt_stamps.hpp execdiag; all zero in
 * the shipped library): per code region r < 16, [r] entries, [16 + r] entries with <= 16 active
 * lanes, [32 + r] with <= 8, [48 + r] the sum of active lanes, since the last cpt_reset_stats. */
int cpt_get_execdiag_counters(cpt_ctx* ctx, uint64_t* out64);
/* Node counts of the scene's walk structures (host-side, no GPU work): [0] the reference
 * order (bvh.cu's tree, 32-B nodes), [1] each octant order of the binary walk tree, [2] the
 * 4-wide walk tree's nodes (112 B each in its compact image, the first 512 staged in LDS; 0 =
 * the ordered walk uses the binary orders), [3] the unbounded (platform) leaves tested before
 * the walk tree.  With [2] > 0, the `nodes` counter of an ordered render counts 4-wide node
 * visits. */
int cpt_get_walk_info(cpt_ctx* ctx, int32_t* out4);
/* DIAGNOSTIC: the device's node memory as the kernels read it, copied to `out` after the
 * context's queued work (a device refit included) has finished: with cpt_get_walk_info's counts,
 * [0] reference-order nodes of 32 B, then eight octant orders of [1] nodes each, then the 4-wide
 * image ([2] x 112 B, padded to a multiple of 32 B) and its leaf array (32-B nodes to the end;
 * image and leaves only when [2] > 0).  *n_bytes receives the size; out == NULL asks for the
 * size alone, and a capacity_bytes below it is CPT_ERR_INVALID_ARG (nothing written).  Launches
 * no kernel and changes no state.  No reference counterpart: a test hook for the device refit
 * (an addition to the ABI: CPT_ABI_VERSION stays 1). */
int cpt_debug_read_nodes(cpt_ctx* ctx, void* out, size_t capacity_bytes, size_t* n_bytes);
/* DIAGNOSTIC: one of the device-built lists of 8x8 tile ids the megakernel dequeues from, copied to
 * `out` (capacity in ids); *n receives its length.  which = 0: the cost schedule's order, all the
 * frame's tiles heaviest first, as the frame's last pilot left it (a CPT_SCHEDULE_COST render,
 * cpt_tile_costs, cpt_adaptive_begin with the flag).  which = 1: the order the last
 * CPT_SCHEDULE_PREVIOUS rebuild left for the next such render.  which = 2: the list the pending
 * adaptive round renders, between a successful cpt_adaptive_begin and the cpt_adaptive_step that
 * returns 0 (round 1 without the cost schedule has no list on the device: 0, 1, 2, ...).
 * which = CPT_TILE_ORDER_TOPUP (4): the active prefix of the last cpt_render_to_count's plan, the
 * tiles with a deficit, largest first, ties row-major (3 stays refused, as any unknown list).
 * CPT_ERR_STATE when the frame holds no such list; CPT_ERR_INVALID_ARG for another `which` or a
 * capacity below the length (nothing written).  WAITS: the copy is queued on the context's stream
 * and the stream is drained, so with which = 2 the call returns after the queued round (which only
 * reads that list: its compaction writes the other buffer).  Launches no kernel and changes no
 * state: the cpt_adaptive_step after it behaves as without it.  No reference counterpart: a test
 * hook for the tile lists (an addition to the ABI: CPT_ABI_VERSION stays 1). */
#define CPT_TILE_ORDER_TOPUP 4
int cpt_debug_read_tile_order(cpt_ctx* ctx, int which, uint32_t* out, size_t capacity, size_t* n);
/* Device time of the last cpt_render (HIP events on the launch stream); waits for it. */
int cpt_last_render_ms(cpt_ctx* ctx, float* ms);
/* Average device time of one launch of the last cpt_render's dominant kernel: the megakernel
 * (launches = 1; the cost schedule's pilot and sort are not included) or the wavefront's
 * extend/shade launches (their total / launches).  Waits for the render. */
int cpt_last_kernel_stats(cpt_ctx* ctx, float* avg_ms, int* launches);

/* Display path (path_tracer.cu:177-254): 5x5 edge-aware denoise of the current 1-spp
 * radiance (accumulator / pass count), running-mean Mix with weight 1/cur_sample_idx,
 * BGRA8 out (alpha byte untouched).  Needs a full frame (rows == NULL).  A pinned bgra_host
 * (cpt_host_register, hipHostMalloc, torch pin_memory) of a 16-aligned width is written by the
 * display kernel itself over PCIe; other memory gets a copy after it (the reference's
 * cudaMemcpy, path_tracer.cu:303). */
int cpt_denoise_mix(cpt_ctx* ctx, uint32_t cur_sample_idx, uint8_t* bgra_host);
/* cpt_denoise_mix with a Mix weight per pixel (an addition; the reference's Mix has
 * the frame's one cur_sample_idx, path_tracer.cu:241-254): the display state holds, beside the
 * running mean, each pixel's sample count n, and the pass mixes at 1 / (n + 1), the correctly
 * rounded f32 quotient, and stores n + 1.  The stencil, the weights, the clamp, the BGRA8 bytes,
 * the pinned-host path, the timing (cpt_last_display_ms), the conditions and the error codes are
 * cpt_denoise_mix's; full frame only.  From a zeroed display state (a new frame,
 * cpt_reset_display) k calls give the running mean and the bytes of cpt_denoise_mix(1), ..., (k),
 * bit for bit.  cpt_denoise_mix and cpt_denoise_mix_band do not maintain the counts: they record
 * their cur_sample_idx, and the first call that reads the counts afterwards (this one,
 * cpt_reproject_display, cpt_read_display_count) first sets every pixel of the launch region
 * W' x H' to the last recorded index on the stream, so the two kinds of pass can alternate.  Pixels
 * outside the launch region hold 0. */
int cpt_denoise_mix_history(cpt_ctx* ctx, uint8_t* bgra_host);
/* Pin / unpin a host buffer (hipHostRegister, mapped) so display frames reach it without a
 * staging copy -- e.g. the BGRA8 buffer the reference hands to its per-pass callback
 * (path_tracer.cu:303-304).  Unregister before freeing it. */
int cpt_host_register(void* ptr, size_t bytes);
int cpt_host_unregister(void* ptr);
/* Display path for output rows [y0, y1) of the 16-aligned launch (0 <= y0 < y1 <= 16*(H/16)),
 * for row-banded multi-GPU display: the context's frame rows (cpt_set_frame) must be one
 * ascending run covering [max(0, y0-3), min(16*(H/16), y1+3)) -- the band and the rows its
 * linear-offset stencil reaches (x +- 2 wraps into the next row).  The Mix running mean and the
 * BGRA8 output hold the band's rows only ((y1-y0) x W x 4 bytes to bgra_host, may be NULL); a
 * new band starts a fresh (zeroed) mean.  Byte-identical to rows y0..y1-1 of cpt_denoise_mix. */
int cpt_denoise_mix_band(cpt_ctx* ctx, uint32_t cur_sample_idx, int y0, int y1, uint8_t* bgra_host);
/* Device-to-device copy of the current display band's BGRA8 rows (for an RCCL gather), ordered
 * against caller_stream as cpt_copy_accum_device. */
int cpt_copy_bgra_device(cpt_ctx* ctx, void* device_dst, size_t bytes, void* caller_stream);
/* The output rows [y0, y1) the display buffers currently hold (cpt_denoise_mix: the whole
 * 16-aligned launch; cpt_denoise_mix_band: the band); 0, 0 before the first display pass. */
int cpt_display_band(const cpt_ctx* ctx, int* y0, int* y1);
/* The Mix running mean of the current display band ([(y1-y0)*W][3] floats: rows y0..y1-1; the
 * whole 16-aligned launch's rows for cpt_denoise_mix), read back for checking and checkpoints.
 * `capacity` is rgb's size in floats: CPT_ERR_INVALID_ARG (nothing written) when it is smaller
 * than the band (size it from cpt_display_band). */
int cpt_read_mix(cpt_ctx* ctx, float* rgb, size_t capacity);
/* The per-pixel sample counts beside that mean ([(y1-y0)*W] floats holding integers; no reference
 * counterpart), as cpt_denoise_mix_history and cpt_reproject_display see them: after
 * cpt_denoise_mix[_band] calls, the last cur_sample_idx inside the launch region.  `capacity` as
 * cpt_read_mix's, in floats. */
int cpt_read_display_count(cpt_ctx* ctx, float* count, size_t capacity);
/* Device time of the last display kernel (Denoising + Mix, the reference's per-pass log of
 * path_tracer.cu:261,300 split by kernel), from HIP events on the context's stream; waits
 * for it. */
int cpt_last_display_ms(cpt_ctx* ctx, float* ms);
/* Zero the Mix running mean and the per-pixel sample counts (the reference's buffer starts
 * uninitialised; here both are zeroed when the frame is created and by this call). */
int cpt_reset_display(cpt_ctx* ctx);

/* Presenting an HDR frame (an addition; the reference's only 8-bit output is the
 * display loop above, which owns its running mean, clamps to [0, 1] and writes 255.99 * linear):
 * the accumulator of any frame, or the last filter result, to BGRA8 through an exposure, a tone
 * curve and a transfer, and an exposure meter.  All of it is f32 + - * / in a stated order,
 * comparisons, integer operations and one table (cpt_present.hpp), so the device, the host hooks
 * below and a numpy restatement agree byte for byte.
 *   source colour c: CPT_PRESENT_ACCUM: n = accum.w; c = accum.xyz / n where n > 0 and finite,
 *     else c = 0 and the pixel is unsourced.  CPT_PRESENT_FILTERED: the rgb cpt_read_filtered reads.
 *   c' = c > 0 ? c : 0 (NaN, negatives, -0 become +0);  x = min(c' * e, 65504), e the exposure.
 *   y = CPT_TONE_CLAMP: min(x, 1);  CPT_TONE_REINHARD: min((x (1 + x / (w w))) / (1 + x), 1), w =
 *     `white`;  CPT_TONE_ACES: min(max((x (2.51 x + 0.03)) / (x (2.43 x + 0.59) + 0.14), 0), 1).
 *   byte = CPT_TRANSFER_LINEAR: (uint8_t)(255.99f * y), the reference's;  CPT_TRANSFER_SRGB: the
 *     number of k in 1..255 with T[k] <= y, T[k] the smallest float t with 255 oetf(t) >= k - 0.5.
 *   4 bytes per pixel: B, G, R, 255.
 * The exposure is a word in device memory (1 after cpt_set_frame), so a meter and a present queue
 * behind each other with no host round trip.  The meter: a pixel is metered if it is sourced and
 * l = luma(c') is finite and > 0; it adds one to word clamp((int)(bits(l) >> 20) - 888, 0, 255) of a
 * histogram (eight bins per octave from 2^-16 to 2^16), every other pixel to word 256.  With N the
 * sum of words 0..255: N == 0 leaves e; otherwise rank = min(N permille / 1000, N - 1), b the least
 * bin whose cumulative count exceeds rank, L the float with bits (b + 888) << 20, target = key / L,
 * and e <- target when adapt == 1, else e + (target - e) adapt.
 * All calls need a frame (any rows; CPT_ERR_STATE without one, while an adaptive render is pending,
 * and for CPT_PRESENT_FILTERED without a filter result), write only the present state (the BGRA
 * plane, the histogram, the exposure) and nothing at all when they fail; no allocation after the
 * frame's first of them. */
#define CPT_PRESENT_ACCUM    0
#define CPT_PRESENT_FILTERED 1
#define CPT_TONE_CLAMP    0
#define CPT_TONE_REINHARD 1
#define CPT_TONE_ACES     2
#define CPT_TRANSFER_LINEAR 0
#define CPT_TRANSFER_SRGB   1
/* Sets the exposure (finite, > 0; else CPT_ERR_INVALID_ARG), on the context's stream. */
int cpt_set_exposure(cpt_ctx* ctx, float exposure);
/* Meters `source` and moves the exposure, asynchronously on the context's stream.  key finite and
 * > 0, permille 0..1000, adapt in [0, 1]; else CPT_ERR_INVALID_ARG. */
int cpt_meter_exposure(cpt_ctx* ctx, int source, float key, int permille, float adapt);
/* The exposure and the last meter's 257 histogram words (zeros before the first); waits for the
 * stream.  Either pointer may be NULL. */
int cpt_read_exposure(cpt_ctx* ctx, float* exposure, uint32_t* hist257);
/* Presents `source` into the context's BGRA8 plane ([n_rows*width][4]), asynchronously.  white is
 * read by CPT_TONE_REINHARD only but must be > 0 and not NaN.  bgra_host, when not NULL, receives a
 * copy that follows the kernel on the stream (the kernel never writes host memory): wait with
 * cpt_synchronize before reading it. */
int cpt_present(cpt_ctx* ctx, int source, int tone, float white, int transfer, uint8_t* bgra_host);
/* The last cpt_present's plane: read back (capacity in bytes, at least n_rows*width*4; waits), or
 * copied on the device, ordered against caller_stream as cpt_copy_accum_device.  CPT_ERR_STATE
 * before the frame's first cpt_present. */
int cpt_read_present(cpt_ctx* ctx, uint8_t* bgra, size_t capacity);
int cpt_copy_present_device(cpt_ctx* ctx, void* device_dst, size_t bytes, void* caller_stream);
/* Device time of the last cpt_meter_exposure's or cpt_present's launches, whichever was later (HIP
 * events on the context's stream); waits for it. */
int cpt_last_present_ms(cpt_ctx* ctx, float* ms);
/* HOST ONLY, no GPU: the functions the kernels run.  `src`: [npix][4] floats, the accumulator, for
 * CPT_PRESENT_ACCUM; [npix][3], the filtered rgb, for CPT_PRESENT_FILTERED.  cpt_present_host writes
 * bgra [npix][4].  cpt_meter_host writes hist257 (may be NULL) and moves *exposure.
 * cpt_present_srgb_thresholds_host: the table, t256[0] = 0 and T[1..255].  Arguments as the device
 * calls'; CPT_ERR_INVALID_ARG likewise. */
int cpt_present_host(size_t npix, int source, const float* src, float exposure, int tone, float white, int transfer,
                     uint8_t* bgra);
int cpt_meter_host(size_t npix, int source, const float* src, float key, int permille, float adapt, float* exposure,
                   uint32_t* hist257);
int cpt_present_srgb_thresholds_host(float* t256);

/* Antialiased presentation (an addition; CPT_ABI_VERSION stays 1).  Every pass of a
 * pixel goes through the same point of it (RayGen has no pixel offset), so a frame converges to a
 * point-sampled image with stair-stepped silhouettes.  Shading is expensive and visibility cheap:
 * cpt_aa_coverage traces S x S first-hit rays inside each pixel on a geometric edge and attributes
 * every sub-sample to the pixel of the 3x3 block whose centre ray saw the same surface;
 * cpt_present_aa presents the coverage-weighted mix of those pixels' tone-mapped colours (after
 * Chajdas, McGuire, Luebke 2011).  The integrator, the accumulator and cpt_present are untouched.
 * All of it is f32 + - * /, RayGen's sqrt, comparisons and integers (cpt_antialias.hpp), so the
 * device, the host hooks below and a numpy restatement agree bit for bit.
 *   Sub-sample s = j S + i (0 <= i, j < S; S = 2 or 4) of pixel (x, y): RayGen's ray at zero lens
 *     offset through ((x + ox) / W, (y + oy) / H), ox = (2i + 1 - S) / 2S and oy alike (negative
 *     quotients at x = 0 or y = 0 are kept), tmin 0, tmax 1e30, walked as cpt_gbuffer walks under
 *     the same CPT_TRAVERSAL_* flags.
 *   Edge pixel p: some in-frame 8-neighbour q has id_q != id_p, or id_p >= 0 and
 *     (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z < normal_cos.  Other pixels trace nothing.
 *   Attribution: the block's pixels are k = 0..8 row-major, k = 4 is p.  A sub-sample that hit
 *     (id_s, n_s) matches an in-frame q of the block if id_q == id_s and (id_s == -1 or the dot
 *     product of n_s and n_q, formed as above, >= normal_cos); the nearest match wins, in integer
 *     units of 1/2S between (2i + 1 - S, 2j + 1 - S) and (2S dx, 2S dy), ties to k = 4, then to the
 *     lowest k; with no match it counts on k = 4 and the pixel is flagged unmatched.
 *   Coverage of p: nine counts c[0..8] summing to S x S (all on k = 4 for a non-edge pixel) and
 *     the flags CPT_AA_EDGE, CPT_AA_UNMATCHED.
 *   Resolve: per channel acc = 0, then for k ascending with c[k] > 0: acc = acc + float(c[k]) y_k,
 *     y_k cpt_present's value of that pixel after source, exposure and tone curve; out = acc / S^2
 *     (exact); the byte transfer is cpt_present's.  A pixel whose coverage is all on itself gets
 *     cpt_present's bytes exactly. */
#define CPT_AA_EDGE      1
#define CPT_AA_UNMATCHED 2
/* The coverage of the frame at `cam`, asynchronously on the context's stream.  First makes the
 * frame's G-buffer at `cam` exactly as cpt_gbuffer(ctx, cam, flags) does (a side effect: the
 * G-buffer and cpt_last_query_ms are that call's); nothing else of the frame is written.  Needs a
 * scene and a frame that holds every row 0..height-1 in order (CPT_ERR_STATE otherwise, and while
 * an adaptive render is pending); samples 2 or 4, normal_cos in [-1, 1], flags within
 * CPT_TRAVERSAL_*, a camera of the frame's size (CPT_ERR_INVALID_ARG otherwise).  A call refused
 * for its arguments, for the context's state or for a failed allocation writes nothing.  A HIP
 * failure behind the G-buffer's trace (an event, a launch: CPT_ERR_HIP) leaves the G-buffer at `cam`
 * and the coverage, if there was one, as the last successful call left it: run the call again
 * before cpt_present_aa.  The state is allocated at the frame's first call and dropped by cpt_set_frame;
 * re-run the call after a camera move or an object edit, as cpt_gbuffer. */
int cpt_aa_coverage(cpt_ctx* ctx, const cpt_camera* cam, uint32_t flags, int samples, float normal_cos);
/* The last cpt_aa_coverage's result: counts9 [npix][9] and flags [npix] (either may be NULL);
 * waits for the stream.  CPT_ERR_STATE before the frame's first cpt_aa_coverage. */
int cpt_read_aa_coverage(cpt_ctx* ctx, uint8_t* counts9, uint8_t* flags, size_t capacity_pixels);
/* cpt_present through the coverage: its arguments and errors, and CPT_ERR_STATE with no
 * cpt_aa_coverage since cpt_set_frame.  Writes cpt_present's plane, so cpt_read_present and
 * cpt_copy_present_device serve it, and cpt_last_present_ms times it. */
int cpt_present_aa(cpt_ctx* ctx, int source, int tone, float white, int transfer, uint8_t* bgra_host);
/* Device time of the last cpt_aa_coverage's edge and coverage kernels (its G-buffer trace is
 * cpt_last_query_ms's); waits for it. */
int cpt_last_aa_ms(cpt_ctx* ctx, float* ms);
/* HOST ONLY, no GPU: the functions the kernels run.  cpt_aa_rays_host: the samples^2 rays of pixel
 * (x, y) of a W x H image, origin3 / dir3 [samples^2][3] in sub-sample order.
 * cpt_aa_coverage_host: counts9 [npix][9] and flags [npix] from the G-buffer's id and normal3 planes
 * and every pixel's sub-sample hits sub_id [npix][samples^2], sub_normal3 [npix][samples^2][3] (-1
 * and any normal on a miss; read for edge pixels only).  cpt_present_aa_host: bgra [npix][4] from
 * `src` as cpt_present_host takes it and counts9 (a count on a pixel outside the frame:
 * CPT_ERR_INVALID_ARG).  Arguments as the device calls'; CPT_ERR_INVALID_ARG likewise. */
int cpt_aa_rays_host(const cpt_camera* cam, int W, int H, int samples, int x, int y, float* origin3, float* dir3);
int cpt_aa_coverage_host(int W, int H, int samples, float normal_cos, const int32_t* id, const float* normal3, const int32_t* sub_id,
                         const float* sub_normal3, uint8_t* counts9, uint8_t* flags);
int cpt_present_aa_host(int W, int H, int samples, int source, const float* src, const uint8_t* counts9, float exposure, int tone,
                        float white, int transfer, uint8_t* bgra);

/* Bloom for presented frames (an addition; CPT_ABI_VERSION stays 1).  The tone curve
 * sends every value far above the display's white to the same byte; bloom spreads the light above
 * a threshold over its neighbourhood in front of the curve, so a highlight's size tells how bright
 * it is.  cpt_bloom builds a pyramid of the source's bright pass; cpt_present_bloom is cpt_present
 * with the pyramid's sum added to each pixel before the tone curve.  All of it is f32 + - * /,
 * comparisons and integers in a stated order (cpt_bloom.hpp), so the device, the host hooks below
 * and a numpy restatement agree bit for bit.  min, c', x, the tone curves and the bytes are
 * cpt_present's above; luma(r, g, b) = (0.2126 r + 0.7152 g) + 0.0722 b as the meter's.
 *   Levels: level 0 is the frame, W x H; level l has w_l = (w_(l-1) + 1) / 2 columns (integer
 *     division) and h_l rows alike; `levels` L in 1..CPT_BLOOM_MAX_LEVELS is the coarsest.  Any frame
 *     size is allowed (a 1 x 1 frame has eight 1 x 1 levels).
 *   Bright pass of a pixel (level 0, never stored): x = min(c' e, 65504) per component, e the
 *     exposure word; l = luma(x); k = l > 0 ? max(l - threshold, 0) / l : 0; b = x k per component.
 *   Down-step from level l to l + 1 (l = 0..L-1; level 0 is b), per component: texel (X, Y) reads
 *     columns 2X-1, 2X, 2X+1, 2X+2 and rows 2Y-1..2Y+2 of level l, each index clamped into 0..w_l-1
 *     (0..h_l-1); each of the four rows first, r = (t0 + 3 t1) + (3 t2 + t3) over its columns, then
 *     B = ((r0 + 3 r1) + (3 r2 + r3)) * 0.015625 over the rows.
 *   Up-step from level l + 1 to texel (x, y) of level l: px = x >> 1, qx = px + 1 for odd x and
 *     px - 1 for even x, clamped into 0..w_(l+1)-1; py, qy alike; h(row) = 3 T[row][px] + T[row][qx];
 *     up = (3 h(py) + h(qy)) * 0.0625.
 *   Accumulation: U_L = B_L;  U_l = B_l + up(U_(l+1)) for l = L-1..1.  The glow of a frame pixel is
 *     g = up(U_1) at (x, y).
 *   Composite: x' = x + intensity g per component, y = the tone curve of min(x' * 1, 65504), and
 *     cpt_present's byte of y.  intensity 0, and a threshold above every luminance, give
 *     cpt_present's bytes.
 * The pyramid is in exposed units at the exposure of the build: meter, then bloom, then present. */
#define CPT_BLOOM_MAX_LEVELS 8
/* Builds U_1..U_levels of `source` (CPT_PRESENT_*) at the current exposure word, asynchronously on
 * the context's stream.  Needs a frame that holds every row 0..height-1 in order, no adaptive render
 * pending and, for CPT_PRESENT_FILTERED, a filter result (CPT_ERR_STATE otherwise).  An unknown
 * source, levels outside 1..CPT_BLOOM_MAX_LEVELS and a threshold that is negative, NaN or infinite:
 * CPT_ERR_INVALID_ARG.  Every check and every allocation (the pyramid, about a third of the frame in
 * float4 texels, and the present state, at the frame's first call) precedes the first write: a
 * refused call writes nothing.  Writes the pyramid alone.  Dropped by cpt_set_frame. */
int cpt_bloom(cpt_ctx* ctx, int source, float threshold, int levels);
/* cpt_present with the last cpt_bloom's glow: cpt_present's arguments and errors, intensity finite
 * and >= 0 (CPT_ERR_INVALID_ARG otherwise), a full frame as cpt_bloom, and CPT_ERR_STATE with no
 * cpt_bloom since cpt_set_frame.  `source` is the plane x is taken from; the glow is the pyramid's,
 * whatever it was built from.  Writes cpt_present's plane, so cpt_read_present and
 * cpt_copy_present_device serve it, and cpt_last_present_ms times it. */
int cpt_present_bloom(cpt_ctx* ctx, int source, int tone, float white, int transfer, float intensity, uint8_t* bgra_host);
/* U_level of the last cpt_bloom as [h_level][w_level][3] floats (level in 1..its levels; capacity
 * in texels); waits for the stream.  CPT_ERR_STATE before the frame's first cpt_bloom. */
int cpt_read_bloom(cpt_ctx* ctx, int level, float* rgb, size_t capacity_texels);
/* Device time of the last cpt_bloom's launches (HIP events); waits for it. */
int cpt_last_bloom_ms(cpt_ctx* ctx, float* ms);
/* HOST ONLY, no GPU: the functions the kernels run.  `src` as cpt_present_host takes it, for a
 * W x H frame.  cpt_bloom_host: U_level of a pyramid of `levels` as [h_level][w_level][3].
 * cpt_present_bloom_host: bgra [W*H][4], the pyramid built at `exposure` from the same plane.
 * Arguments as the device calls'; CPT_ERR_INVALID_ARG likewise. */
int cpt_bloom_host(int W, int H, int source, const float* src, float exposure, float threshold, int levels, int level, float* rgb);
int cpt_present_bloom_host(int W, int H, int source, const float* src, float exposure, float threshold, int levels, float intensity,
                           int tone, float white, int transfer, uint8_t* bgra);

/* HBM streaming-read ceiling of the device (the roofline peak, measured on
 * the box): `iters` grid-stride 16-B-per-lane read passes over a fresh `bytes`-byte buffer
 * (use >> 256 MiB so the Infinity Cache cannot serve it), GB/s from HIP events. */
int cpt_measure_read_bandwidth(cpt_ctx* ctx, size_t bytes, int iters, float* gbps);
/* DIAGNOSTIC: the same streaming read in the display kernel's access shapes, bytes_per_lane 4 (one
 * float per lane), 12 (three consecutive floats per lane) or 16 (one float4), one kernel
 * (k_read_pattern<bpl>) per shape: the known byte counts a rocprofv3 FETCH_SIZE pass is calibrated
 * against (tools/fetch_calibration.py). */
int cpt_measure_read_pattern(cpt_ctx* ctx, int bytes_per_lane, size_t bytes, int iters, float* gbps);
/* Host-only test hook (no GPU): the cap-disk bound a cylinder leaf carries (cpt_host_bvh.cpp
 * cap_disk_bound), the largest float c with  sqrtf(q) < radius  <=>  q <= c  for every float
 * q; the kernels decide the reference's cap test (object.cu:52-77) with it. */
int cpt_cap_disk_bound(float radius, float* out);
/* Device-math known-answer surface used by the parity tests: op 0 powf(a,b), 1 sinf(a),
 * 2 cosf(a), 3 asinf(a), 4 atanf(a), 5 (float)pow((double)a, 1.0/(double)b),
 * 6 (float)((double)a / (double)b) [IEEE f64 division], 7 a / b [f32 division],
 * 8 sqrtf(a), 9 pow(a, 5) as schlick computes it (dm::pow5f), 10 the BSDF lobe's short pow
 * lobe_pow(a, 1.0/(double)b) (the same float as op 5). */
int cpt_math_batch(cpt_ctx* ctx, int op, const float* a, const float* b, float* out, size_t n);
/* Device self-test of the exact-quotient kernel helper against the hardware IEEE f32 divide
 * over n hashed operand pairs (which: 0 all bit patterns, 1 slab-like ranges, 2 mid ranges).
 * which = 3: the f64 reciprocal helper rcp_d(d) against the IEEE 1.0 / (double)d for the first
 * n float bit patterns d (n = 2^32: all of them); which = 4: the f32 reciprocal helper rcp_f on
 * its domain (2^-126 <= |d| < 2^126, 0, inf, NaN) and rcp_f(sqrtf(d)) for every pattern.
 * which = 5: the f32 square-root helper sqrt_nn against sqrtf on its domain (+-0,
 * |x| >= 2^-96, inf, NaN).
 * which = 6: the display weight dn_weight (short exp + rounding guard) against its slow form
 * dn_weight_slow for the float bit patterns [0, n) (n = 2^31: every non-negative float, inf and
 * NaN); which = 7: counts the patterns whose guard sends them to the slow form (not an error).
 * which = 8: the BSDF lobe's short pow (lobe_pow) against (float)pow(x, y) of the full double
 * sequence for the float bit patterns x in [0, n), y = the double whose bits are `seed`;
 * which = 9: counts the x whose guard sends them to the full pow; which = 10: the lobe's short
 * sinf/cosf (lobe_sincos) against the full sequence for the float patterns [0, n); which = 11:
 * counts the guard's fallbacks there; which = 12: the sky fetch's short atanf and asinf
 * (miss_atanf, miss_asinf) against the full sequences for the float patterns [0, n); which = 13:
 * counts the patterns where either guard falls back (asinf: on [-1, 1]).
 * which = 14: the ordered walk's quotient-free winner certificate (cert_inside) against the exact
 * slab test on n hashed cases from `seed` (boxes, rays, distances within 16 ulps of a plane):
 * out[0] counts the cases it certifies and the exact test rejects (0 expected); which = 15 counts
 * the certified cases and which = 16 the cases the exact test passes.
 * which = 17: lobe_pow against (float)pow(x, y) at hashed material exponents, for the indices
 * [0, n): smoothness s = a hash of (seed, i >> 20) in [0, 6], y = 1.0 / (double)powf(1000, s) as the
 * material set-up forms it, x = a hash of (seed, i) over the float patterns of [2^-33, 1];
 * which = 18: counts the same pairs whose guard sends them to the full pow (17, 18: the failing
 * pairs are (x bits << 32 | s bits)).
 * out[0] receives the mismatch count (0 expected), out[1..out_len) up to out_len-1 failing
 * pairs as (a bits << 32 | d bits). */
int cpt_selftest_qdiv(cpt_ctx* ctx, int which, uint64_t n, uint64_t seed, uint64_t* out, int out_len);
/* TEST HOOK for the tail consolidation's error paths (all zero = normal operation): flags bit 0
 * starts every workgroup with a phantom live chain (a lost count: the keeper waves can never
 * see the workgroup drained), bit 1 makes hand-overs never publish their slot; the keeper's
 * idle-spin limit and the hand-over wait as log2 (0 = the defaults, 26 and 22).  A render that
 * trips either limit must end with CPT_ERR_DEVICE. */
int cpt_set_debug_consolidation(cpt_ctx* ctx, uint32_t flags, int keeper_spin_log2, int publish_wait_log2);
/* TEST HOOK that caps the megakernel's persistent grid (0, 0 = normal operation, the default), so
 * that frames small enough for the scalar oracle make every lane take several pixels in turn.
 * max_workgroups > 0: the render's launch and the cost pilot's (cpt_render with
 * CPT_SCHEDULE_COST, cpt_tile_costs) have at most that many workgroups (1024 lanes each with the
 * 4-wide walk's LDS image, 256 without), and so has cpt_aa_coverage's persistent kernel.
 * lanes_per_wave > 0: only the first lanes_per_wave lanes of each wave take pixels and handed-over
 * chains; the others stay idle (cpt_aa_coverage's kernel ignores this part).  Every kernel
 * instantiation is well defined for 1 <= lanes_per_wave < 64: the thresholds of the wide walk's
 * leaf rounds and of the deferred sky fetches are shares of the lanes at work, a walk is
 * suspended only after 40 lanes of its wave have finished theirs (never, below 41 lanes), the
 * static first take switches itself off, and a retiring wave hands over at most as many chains as
 * it holds (the levels below then queue chains they have no idle lane for yet, and take them as
 * lanes fall idle).  The image, the RNG end states and every counter the walk defines per ray are
 * unchanged; the render is slower.  The wavefront path has no persistent grid and ignores the
 * hook.  Negative values and lanes_per_wave > 64: CPT_ERR_INVALID_ARG. */
int cpt_set_debug_grid(cpt_ctx* ctx, int max_workgroups, int lanes_per_wave);
/* HOST ONLY, no GPU: the arithmetic that sizes a megakernel launch, the function every launch runs
 * with the context's own figures.  A device of `cus` compute units holding blocks_per_cu workgroups
 * of `block` lanes of the kernel each; `tiles` 8x8 tiles to render, lanes / replicate pixels per wave
 * (64, 1 in normal use); max_workgroups as in cpt_set_debug_grid.  workgroups: the launch's grid
 * (0: nothing is launched).  slab_chains (may be NULL): the chains the tail consolidation's
 * hand-over slab holds for that device, a workgroup's slots for each resident workgroup. */
int cpt_launch_grid_host(int cus, int blocks_per_cu, int block, int64_t tiles, int lanes, int replicate, int max_workgroups,
                         int* workgroups, uint64_t* slab_chains);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif  /* CPT_H_ */
