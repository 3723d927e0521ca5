/* rtx_amd.h — C-ABI of the MI355X-native real-time path tracer (librtx.so).
 *
 * Drop-in boundary for the reference's renderer API, class RayTracer
 * (/root/reference/src/kernel.cuh:431-470) and its config surface LoadConfig
 * (configLoader.cpp:5-27).  Plain C: opaque handle, plain pointers and sizes, status codes
 * instead of the reference's exit() on errors (cudaError.cuh:6-13).  Not thread-safe per
 * handle (same as the reference).  All output buffers are caller-owned host memory.
 *
 * Every entry point below names the reference interface it replaces.
 */
#ifndef RTX_AMD_H
#define RTX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_ERR_ARG (-1)         /* invalid argument / size */
#define RT_ERR_HIP (-2)         /* HIP runtime error (rt_last_error has the text) */
#define RT_ERR_IO (-3)          /* config / data file problem */
#define RT_ERR_STATE (-4)       /* call out of order (e.g. draw before init) */
#define RT_ERR_NO_DEVICE (-5)   /* no gfx950 device visible */
#define RT_ERR_DEVICE (-6)      /* a kernel reported a failure (rt_last_error has the text): the LBVH's
                                   TLAS workgroup timed out waiting for a batch; the frames since the
                                   last check may be wrong, the renderer re-armed itself; or
                                   rt_set_mesh_device met indices past its vertex count and read
                                   them as 0.  Reported
                                   once, by the call that finds it: rt_sync, rt_build_bvh, the draws
                                   and the reads (rt_get_buffer, rt_download, rt_get_ray_count,
                                   rt_save_image ...).  Setters (rt_set_*stream, rt_bind_buffer,
                                   rt_set_collective_hook, rt_upload_texture) never return it: they
                                   do their work and leave the report to the next such call */

typedef struct rt_context rt_context;

/* ---------------------------------------------------------------- lifecycle */

/* RayTracer::RayTracer(screenWidth, screenHeight), kernel.cuh:435-441, plus LoadConfig
 * (configLoader.cpp:5-27).  config_toml may be NULL (defaults) or a path to a TOML file with
 * the reference's [resolution] / [file] / [optimziation] tables; extensions: [scene]
 * chunkDim (VoxelsGenerator::kChunkDim, terrain.h:42), [render] spp, [render] device, [render]
 * geometryMotion (true | false, default false: rt_set_geometry_motion's initial state; any other
 * value is refused with RT_ERR_IO), [render] emitterSampling (true | false, default false) and [render]
 * emitterProbability (a number in [0, 1], default 0.5): rt_set_emitter_sampling's initial state; an
 * unparsable or out-of-range value is refused with RT_ERR_IO.  [render] signedDistance (true | false,
 * default false: rt_set_signed_distance's initial state; any other value is refused with RT_ERR_IO).
 * [tuning] (scheduling A/B aids; the defaults are the measured best): arena (bool),
 * streams ("cumask" | "prio"), tracePerCu / trace4PerCu (0: automatic), trace3ShortPerCu (a short queue
 * 3's workgroups per CU on one GPU; 0: all of them), chain ("serial" | "off" |
 * "always"), shadeOnSide (bool), shadeBlocksPerCu (synchronous frames; 0: the kernel's residency),
 * overlapAfter / cameraAfter (-1: automatic); the synchronous draws' launches ahead (rt_draw):
 * syncSpec (bool), specAfter (the kernel of this frame they follow: 1 shade), specShade (0 / 1 / 2:
 * the shade kernel never / beside the lean bounce kernels / always), specShadePerCu, specTracePerCu,
 * specChain (-1: by queue 3's length); the denoise list passes: dnSplit (0 / 1 / 2: two threads per
 * pixel never / in synchronous frames / always; default 0), dnFold (bool, default false: the last
 * a-trous pass over list 1 only); resumeSplit (0 / 1 / 2: resume<3> of the four-kernel
 * bounce chain as one kernel / split into the shading list's kernel and a lean pass / the lean pass on
 * a stream of its own in pipelined one-GPU frames).  [debug] (fault
 * injection, tests): bvhSkipPublish, bvhSkipPublishBuilds, bvhWaitMs.  The library reads no
 * environment variables. */
int rt_create(int screen_width, int screen_height, const char* config_toml, rt_context** out);

/* RayTracer::init, init.cu:53-410: builds the procedural default scene, allocates every device
 * resource, uploads blue-noise/sky tables, runs the frame-1 smooth normals.  Like the reference it
 * ignores [file] inputMeshFileName (its LoadTrianglesFromFile call is commented out, init.cu:78-82);
 * the extension [scene] meshFile loads a meshProcessor .bin instead (u32 count + count 128-B
 * Triangle records, init.cu:28-50; a shorter file is refused with RT_ERR_IO).  The scene is built
 * and checked before any device call (RT_ERR_IO / RT_ERR_ARG on any machine), then the device
 * (RT_ERR_NO_DEVICE without a gfx950). */
int rt_init(rt_context* ctx);

/* RayTracer::draw, kernel.cu:259-398 (with UpdateFrame, kernel.cu:61-137): one synchronous
 * frame.  rgba8_out (screen W*H*4) and hdr_out (render W*H*4 floats, pre-tone-map HDR) may
 * each be NULL.  With [optimziation] useDynamicResolution the render size follows the frame
 * time from the second frame on (rt_get_info's renderWidth/Height); size hdr_out for
 * maxWidth x maxHeight.
 * Synchronous draws (this one, and rt_draw_device without RT_DRAW_ASYNC) on one GPU launch the
 * next frame's camera-ray and shade kernels ahead, beside this frame's bounces and denoise, into
 * the other G-buffer set ([tuning] syncSpec): the draw still returns with its frame complete, and
 * those kernels may still run on the context's side stream.  The next draw uses their results only
 * when its launch parameters (camera, sky, size, frame number, materials, buffers) and the geometry
 * epoch (rt_update_vertices) equal theirs, and traces again otherwise; a change of the sky that
 * regenerates its tables (skyScalar, sunScalar, sunAngle, timeOfDay, sunAxisAngle, needRegenerate)
 * always does, also when no launch parameter moves with it (the two scalars);
 * any call that waits for the streams (rt_sync, the reads, the setters) discards them first.
 * Parameters only the denoise and post chain read (pass, post, denoise, the frame time) and a device
 * ray query cost no retrace.  rt_download(RT_ARR_SPEC_STATS) counts the launches, reuses and drops;
 * tests/test_gpu_draw_state.py walks every state-changing call against this rule. */
int rt_draw(rt_context* ctx, uint8_t* rgba8_out, float* hdr_out);

/* RayTracer::draw(SurfObj* renderTarget), kernel.cu:259-398 (CopyToOutput kernel.cu:26-59 writes
 * the caller's surface): one frame whose screen-size RGBA8 image is written straight into
 * caller-owned DEVICE memory (row pitch in bytes, 0 = width * 4; 4-byte aligned).  flags 0: returns
 * when the frame is complete, as the reference's draw does (it ends with a device sync).
 * RT_DRAW_ASYNC: returns once the frame is enqueued; frames are pipelined (the denoise/post of
 * frame f overlaps the trace of f+1 on an internal stream (low priority under [tuning] streams = "prio") unless rt_set_post_stream
 * named one) and each frame's target must stay valid until rt_sync (or a later synchronous
 * call) has returned.  rt_download(RT_ARR_RGBA8) reads the last frame's target. */
#define RT_DRAW_ASYNC 1
int rt_draw_device(rt_context* ctx, void* rgba8_device, size_t pitch_bytes, int flags);

/* RayTracer::cleanup + ~RayTracer, init.cu:601-663, kernel.cuh:443-446 */
void rt_destroy(rt_context* ctx);

/* last error text for this handle (NULL handle: last rt_create failure) */
const char* rt_last_error(const rt_context* ctx);

/* ---------------------------------------------------------------- parameter surface */

/* SkyParams, settingParams.h:26-47 */
typedef struct rt_sky_params {
    int32_t needRegenerate;
    float timeOfDay, sunAxisAngle, skyScalar, sunScalar, sunAngle;
} rt_sky_params;

/* SampleParams, settingParams.h:49-66 */
typedef struct rt_sample_params {
    int32_t sampleSurfaceVsLightUseMisWeight, sampleSkyVsSunUseFluxWeight;
    float sampleSurfaceVsLight, sampleSkyVsSun;
} rt_sample_params;

/* RenderPassSettings, settingParams.h:68-104 */
typedef struct rt_render_pass_settings {
    int32_t enableTemporalDenoising, enableLocalSpatialFilter, enableNoiseLevelVisualize, enableWideSpatialFilter,
        enableTemporalDenoising2, enablePostProcess, enableDownScalePasses, enableHistogram, enableAutoExposure,
        enableBloomEffect, enableLensFlare, enableToneMapping, enableSharpening;
} rt_render_pass_settings;

/* PostProcessParams, settingParams.h:106-124 (toneMappingType: 0 Uncharted, 1 ACES1,
 * 2 ACES2, 3 Reinhard) */
typedef struct rt_post_process_params {
    int32_t toneMappingType;
    float exposure, gain, maxWhite, gamma;
} rt_post_process_params;

/* DenoisingParams, settingParams.h:126-157 */
typedef struct rt_denoising_params {
    float local_denoise_sigma_normal, local_denoise_sigma_depth, local_denoise_sigma_material;
    float large_denoise_sigma_normal, large_denoise_sigma_depth, large_denoise_sigma_material;
    float temporal_denoise_sigma_normal, temporal_denoise_sigma_depth, temporal_denoise_sigma_material;
    float noise_threshold_local, noise_threshold_large;
} rt_denoising_params;

/* public members skyParams .. sampleParams, kernel.cuh:465-470 */
typedef struct rt_params {
    rt_sky_params sky;
    rt_sample_params sample;
    rt_render_pass_settings pass;
    rt_post_process_params post;
    rt_denoising_params denoise;
} rt_params;

int rt_get_params(const rt_context* ctx, rt_params* out);
int rt_set_params(rt_context* ctx, const rt_params* in);

/* Camera fields the app sets (init.cu:412-439, kernel.cuh:78-121); fovX in radians */
typedef struct rt_camera {
    float pos[3];
    float yaw, pitch;
    float focal, aperture;
    float fovX;
} rt_camera;

int rt_get_camera(const rt_context* ctx, rt_camera* out); /* RayTracer::GetCamera */
int rt_set_camera(rt_context* ctx, const rt_camera* in);

/* Input (inputControl.cu:29-113): a windowing host forwards GLFW events (key, action and
 * modifier values are GLFW's).  keyboardUpdate sets the W/S/A/D/C/X movement flags and the
 * shift slow-down, or with ctrl saves (C) / loads (V) the camera at [file] cameraSaveFileName;
 * cursorPosUpdate turns the cursor delta into yaw / pitch (the first event after a cursor reset
 * only records the position); scrollUpdate and mouseButtenUpdate are no-ops as in the
 * reference.  rt_draw moves the camera by the held keys once per frame (InputControlUpdate,
 * pos += dir * deltaTime * moveSpeed).  cursorReset (kernel.cuh:465) starts set. */
int rt_keyboard_update(rt_context* ctx, int key, int scancode, int action, int mods);
int rt_cursor_pos_update(rt_context* ctx, double xpos, double ypos);
int rt_scroll_update(rt_context* ctx, double xoffset, double yoffset);
int rt_mouse_button_update(rt_context* ctx, int button, int action, int mods);
int rt_set_cursor_reset(rt_context* ctx, int reset);

/* RayTracer::SaveCameraToFile / LoadCameraFromFile (inputControl.cu:115-149): the reference's
 * 176-byte binary Camera record (kernel.cuh:78-100, derived fields included).  Loading takes
 * pos, pitch, yaw, focal, aperture and fov.x from the record; the derived fields are recomputed
 * by Camera::update every frame, as in the reference.  rt_init loads [file] inputCameraFileName
 * when loadCameraAtInit is true (init.cu:433-435). */
int rt_save_camera(const rt_context* ctx, const char* path);
int rt_load_camera(rt_context* ctx, const char* path);

/* Offscreen presentation (replaces the Vulkan swapchain blit, main.cu:1295-1310): the last
 * frame's RGBA8 output as a binary PPM (P6, screen size), or the denoised pre-tone-map HDR
 * colour as a PFM (PF, render size, bottom row first as the format prescribes). */
#define RT_IMAGE_PPM_RGBA8 0
#define RT_IMAGE_PFM_HDR 1
int rt_save_image(rt_context* ctx, const char* path, int kind);

/* Texture path, init.cu:524-580 + MipmapGen (mipgen.cu:121-182): a 16-bit texture of the atlas
 * (MipmapTextureName, texture.h:5-12) — its level 0 as stbi_load_16 returns it, rows of
 * width * channels ushorts — is copied to the device and its 11-level mip chain is generated there
 * (2x2 mean in float, min 65535, truncated to ushort).  The atlas is 1024 x 1024: 4 channels for
 * the albedo/AO and normal/roughness maps the diffuse shading samples, 1 for the height map.
 * rt_init uploads a deterministic synthetic pair (the PNGs are missing from the reference tree).
 * Synchronous. */
#define RT_TEX_SOIL_ALBEDO_AO 0
#define RT_TEX_SOIL_NORMAL_ROUGHNESS 1
#define RT_TEX_SOIL_HEIGHT 2
int rt_upload_texture(rt_context* ctx, int which, const uint16_t* texels, int width, int height, int channels);

/* Texture sets: per-material atlases.  A texture set is one pair of 1024 x 1024,
 * 11-level ushort4 mip chains (albedo/AO and normal/roughness).  [scene] textureSets = N (absent or 0:
 * 1; at most RT_TEXTURE_SETS_MAX, about 22.4 MB each) makes the context hold N of them.  An unparsable
 * or negative value: RT_ERR_IO from rt_create; N > 16: RT_ERR_ARG from rt_init, before any device call.
 * Set 0 is the soil atlas: rt_upload_texture and RT_ARR_TEX_* mean set 0.  rt_init fills sets 1..N-1
 * with a copy of set 0, so a set nobody uploaded to renders exactly like set 0.  The height map stays
 * single (shading does not read it).
 *
 * rt_upload_texture_set is rt_upload_texture for any set: synchronous, behind a wait for the renderer's
 * streams, mips built on the device; `which` is the albedo or the normal map (RT_TEX_SOIL_HEIGHT with
 * set > 0 is RT_ERR_ARG; with set 0 it is rt_upload_texture's height upload).
 *
 * rt_upload_texture_set_device is the stream-ordered counterpart, in the family of
 * rt_update_vertices_device, rt_set_mesh_device and rt_set_triangle_materials_device: the host is never
 * synchronised and no stream is drained.  `texels` is device memory, 1024 x 1024 x 4 channels of
 * `format`, read after ready_event (NULL: after everything enqueued on the context stream so far); work
 * enqueued on the context stream after the call follows that read.  The write of level 0 and the mip
 * generation run behind every path trace enqueued before the call, on whichever renderer stream: those
 * path traces, pipelined frames in flight included, keep the old texels; every path trace enqueued
 * after the call waits for the upload and sees the new chain.  What a synchronous draw traced ahead is
 * stale and the next draw traces it again.
 *
 * Both calls, checked in this order, and on an error nothing changes: RT_ERR_ARG for NULL ctx, u or
 * texels, an unknown `which` or format, a misaligned (4 B) device pointer, a wrong size or channel
 * count; RT_ERR_STATE before rt_init; RT_ERR_ARG for set >= the context's texture sets; RT_ERR_HIP for
 * a failed launch.  Never RT_ERR_DEVICE. */
#define RT_TEXTURE_SETS_MAX 16
int rt_get_texture_sets(const rt_context* ctx, uint32_t* count);
int rt_upload_texture_set(rt_context* ctx, uint32_t set, int which, const uint16_t* texels, int width, int height,
                          int channels);

#define RT_TEX_FORMAT_U16 0   /* ushort4 rows, as rt_upload_texture */
#define RT_TEX_FORMAT_U8  1   /* uchar4 rows; each channel becomes v * 257 (255 -> 65535) */
typedef struct rt_texture_upload {
    const void* texels;   /* device memory, 1024 x 1024 x 4 channels, 4-byte aligned */
    uint32_t set;
    int32_t which;        /* RT_TEX_SOIL_ALBEDO_AO or RT_TEX_SOIL_NORMAL_ROUGHNESS */
    uint32_t format;      /* RT_TEX_FORMAT_* */
    void* ready_event;    /* hipEvent_t or NULL, as in rt_update_vertices_device */
} rt_texture_upload;
int rt_upload_texture_set_device(rt_context* ctx, const rt_texture_upload* u);

/* Which texture set a material id samples: a table of its own beside the material table (rt_material is
 * unchanged), 256 bytes, all 0 by default.  A textured diffuse hit (Lambertian or microfacet, not
 * RT_MAT_FLAG_FLAT), reached by a camera ray or through bounces, samples both maps of the set bound to
 * its material id; flat entries, glass, mirrors and emitters ignore the binding; [render]
 * materialOverride chooses the id, whose binding then applies.  The binding belongs to the context: it
 * survives rt_set_mesh*, rt_set_materials and rt_reset_materials, and only rt_reset_material_textures
 * clears it; rt_get_materials is unaffected.
 *
 * A binding that is all zeros is no binding: the path trace launches exactly the kernels it launches
 * without these calls.  With any non-zero entry every frame runs the table-reading kernels of
 * rt_set_materials on the unsplit plan (without a custom table, over rt_default_material's entries,
 * under which they are the identity bit for bit).
 *
 * The setters behave like rt_set_materials: they wait for the renderer's streams, drop what a
 * synchronous draw traced ahead and take effect for every path trace enqueued afterwards; they are not
 * stream-ordered.  Every rank of a multi-GPU run calls with the same data.  On an error nothing changes.
 * Checked in this order: RT_ERR_ARG for NULL ctx, sets or out, count == 0, first_id + count > 256;
 * RT_ERR_STATE before rt_init; RT_ERR_ARG for an entry >= the context's texture sets. */
int rt_set_material_textures(rt_context* ctx, uint32_t first_id, uint32_t count, const uint8_t* sets);
int rt_get_material_textures(const rt_context* ctx, uint32_t first_id, uint32_t count, uint8_t* sets);
int rt_reset_material_textures(rt_context* ctx);

/* Sky sets and environment maps.
 *
 * A sky set is everything one sky generation writes: the 512 x 256 sky table with its pdf, CDF and
 * probe tree, the 32 x 32 sun tables likewise, and the light-selection terms (about 3.2 MB).  [scene]
 * skySets = N (absent, 0 or 1: one set; at most RT_SKY_SETS_MAX) makes the context hold N of them.  An
 * unparsable or negative value: RT_ERR_IO from rt_create; N > 8: RT_ERR_ARG from rt_init, before any
 * device call.  With one set a change of the sky parameters rewrites the tables in place, which on a
 * pipelined context (rt_set_post_stream) waits for every stream first.  With two or more it never
 * waits on the host and drains no stream: the next set in turn is generated behind its own readers,
 * which are waited for on the device, on the side stream of a pipelined context (where the LBVH builds
 * and the camera kernels run) and on the context stream otherwise; path traces enqueued earlier, the
 * pipelined frames in flight and what a synchronous draw traced ahead, keep the set they were launched
 * with, and a launch ahead made under the old sky is traced again (RT_ARR_SPEC_STATS[2] counts it).
 *
 * An environment replaces the Hosek sky table and its pdf by an image of the caller's; the sun tables
 * stay those of the sky parameters (sunScalar, sunAngle, timeOfDay, sunAxisAngle), and the CDF, the
 * probe trees and the light selection are derived as ever.  The sky has an upper hemisphere only: the
 * lookup clamps below the horizon and blends to the mist, with or without an environment.  An all-zero
 * environment is valid: every light sample then goes to the sun.  A later change of the sky parameters
 * regenerates the sun tables and keeps the environment.
 *
 * The image: width x height texels of four floats (RT_ENV_FORMAT_F32X4) or four halves
 * (RT_ENV_FORMAT_F16X4), alpha ignored.  RT_ENV_LAYOUT_TABLE is the renderer's own equal-area table,
 * 512 x 256 (what RT_BUF_SKY returns).  RT_ENV_LAYOUT_LATLONG is a latitude-longitude image, row 0 at
 * the zenith, 4 <= width <= 16384, 2 <= height <= 16384, of which the rows above the horizon (2 r + 1 <
 * height) are read; column c points along the table's own azimuth u = (c + 0.5) / width.
 * rt_environment_table is the definition of the table an image gives, compiled for the host, with no
 * context and no device; the device gives its bits.  In short: a source value x counts as
 * (x == x && x > 0) ? min(x, 65504) : 0; a LATLONG texel belongs to the table cell its centre falls
 * into (column (2 c + 1) * 256 / width; row min(255, (int)(cos(theta_r) * 256)), theta_r = pi (2 r + 1)
 * / (2 height)), a cell's value is the mean of its texels weighted by sin(theta_r), summed in fp32 in
 * ascending column, then row order, and a cell that owns no column or row takes the nearest one; the
 * result times `scale`, at most 65504; pdf = dot(rgb, (0.3, 0.6, 0.1)) as the Hosek table's.
 * table: 131072 x 4 floats (.w = 0), pdf: 131072 floats.
 *
 * rt_set_environment behaves like the other host setters: it waits for the renderer's streams, drops
 * what a synchronous draw traced ahead, copies the image into staging of its own (the caller's array
 * is free on return) and takes effect for every path trace enqueued afterwards; it works at any
 * skySets.  rt_set_environment_device is the stream-ordered counterpart, in the family of
 * rt_update_vertices_device: it needs skySets >= 2; the host is never synchronised and no stream is
 * drained; `texels` is device memory, read after ready_event (NULL: after everything enqueued on the
 * context stream so far), and work enqueued on the context stream after the call follows that read;
 * frames in flight keep their sky.  The first device set of a context, and the first one of a larger
 * LATLONG image than any before, allocates device scratch.  rt_reset_environment is a host-style setter
 * that goes back to the Hosek table.  rt_get_environment: whether an environment is active.
 *
 * Checked in this order, and on an error nothing changes: RT_ERR_ARG for NULL ctx or struct, NULL
 * texels, an unknown format or layout, a size outside the limits (TABLE: not 512 x 256), a scale that
 * is not finite or <= 0, a misaligned device pointer (16 B for F32X4, 8 B for F16X4); RT_ERR_STATE
 * before rt_init, or for the device variant with one sky set; RT_ERR_HIP for a failed launch.  Never
 * RT_ERR_DEVICE.  Every rank of a multi-GPU run calls with the same data. */
#define RT_SKY_SETS_MAX 8
int rt_get_sky_sets(const rt_context* ctx, uint32_t* count);
#define RT_ENV_FORMAT_F32X4 0
#define RT_ENV_FORMAT_F16X4 1
#define RT_ENV_LAYOUT_TABLE   0  /* 512 x 256, the renderer's own equal-area table (RT_BUF_SKY) */
#define RT_ENV_LAYOUT_LATLONG 1  /* width x height latitude-longitude image, row 0 at the zenith */
typedef struct rt_environment {
    const void* texels;
    uint32_t width, height, format, layout;
    float scale;        /* multiplies the radiance, like skyScalar; finite, > 0 */
    void* ready_event;  /* device variant: hipEvent_t or NULL, as in rt_update_vertices_device */
} rt_environment;
int rt_set_environment(rt_context* ctx, const rt_environment* host);
int rt_set_environment_device(rt_context* ctx, const rt_environment* dev);
int rt_reset_environment(rt_context* ctx);
int rt_get_environment(const rt_context* ctx, int* active);
/* the rule, compiled for the host; no context, no device */
int rt_environment_table(const rt_environment* host, float* table /*131072 x 4*/, float* pdf /*131072*/);

/* Scene input (host only, no device needed): Perlin::noise3D (perlin.h:50-78) with the reference
 * permutation, the source of the procedural terrain's voxel heights (Chunk::Generate,
 * terrain.cpp:5-45), at n points (xyz triples). */
int rt_scene_noise3d(const float* xyz, size_t n, float* out);

/* The denoiser's Gaussian weights (GetGaussian3x3 / 5x5 / 7x7, gaussian.cuh:12-43; the precomputed
 * tables, USE_PRECALCULATED_GAUSSIAN): size 3, 5 or 7, row-major size*size floats into out (count
 * >= size*size).  The same values the device kernels use.  Host only, no device needed. */
int rt_filter_kernel(int size, float* out, int count);

/* Scan(in, out, tmp, size, blockSize, postfix), scan.cuh:258-298: prefix sum of `size` floats in
 * DEVICE memory — blocks of block_size scanned in LDS (Blelloch tree order), the block totals
 * scanned in one workgroup into tmp (>= size / block_size floats; unused for one block), then added.
 * postfix 1: inclusive, 0: exclusive.  size and block_size powers of two, block_size and the block
 * count each <= 8192 (the reference's asserts).  Enqueued on `stream` (a hipStream_t; NULL = null
 * stream), asynchronous.  Errors: RT_ERR_ARG / RT_ERR_HIP with rt_last_error(NULL). */
int rt_scan_device(const float* in, float* out, float* tmp, int size, int block_size, int postfix, void* stream);

/* Determinism hooks the reference lacks: the frame counter is a function static
 * (kernel.cu:64) and AutoExposure reads wall-clock deltaTime (postprocessing.cu:46-51). */
int rt_set_frame_index(rt_context* ctx, int frame_num); /* next rt_draw renders this frameNum */
int rt_set_delta_time(rt_context* ctx, float ms);       /* <= 0: wall clock */

/* ---------------------------------------------------------------- queries */

typedef struct rt_info {
    uint32_t triCount;          /* real triangles */
    uint32_t triCountPadded;    /* RayTracer::GetTriangleCount (kernel.cuh:462) */
    uint32_t batchCount;        /* BLAS batches of 1024 */
    uint32_t vertexCount;
    int32_t renderWidth, renderHeight, screenWidth, screenHeight;
    int32_t frameNum;           /* frame index of the last rt_draw (0 before the first) */
    int32_t deviceId;
    uint32_t spp;               /* samples (reference PathTrace evaluations) per frame */
    int32_t gbufferSet;         /* G-buffer set the last rt_path_trace wrote (0..2, see rt_set_post_stream) */
    int32_t denoiseRowBegin, denoiseRowEnd; /* rows of a strip-local denoise (rt_set_collective_hook) */
    int32_t gbufferRowBegin, gbufferRowEnd; /* G-buffer rows the next denoise reads: its strip plus
                                               halo when it is strip-local, else the whole frame */
    int32_t stripLocalDenoise;  /* 1: the next denoise is strip-local (the same on every rank) */
    int32_t shadeOnSide;        /* 1: pipelined frames run the shade kernel behind the camera kernel on
                                   the side stream (rt_set_post_stream), not on the context stream */
    int32_t lastChain;          /* 1: the last rt_path_trace ran its bounce stages as the fused k_pt_chain
                                   (serial frames while the previous serial frame's queue 3 was short),
                                   0: as the four kernels trace<3> .. resume<4>; profiles differ */
} rt_info;

int rt_get_info(const rt_context* ctx, rt_info* out);

/* GetBuffer2D, kernel.cuh:459: copies a render buffer to host memory.  Names follow the
 * Buffer2DName enum (kernel.cuh:286-315); half buffers come back as uint16 bit patterns. */
enum rt_buffer_name {
    RT_BUF_RENDER_COLOR = 0,   /* half4 (rgb + ushort material mask), render res */
    RT_BUF_ACCUMULATION = 1,   /* half4 */
    RT_BUF_HISTORY_COLOR = 2,  /* half4 */
    RT_BUF_SCALED_COLOR = 3,   /* half4, screen res */
    RT_BUF_NORMAL = 10,        /* half4 */
    RT_BUF_DEPTH = 11,         /* half */
    RT_BUF_HISTORY_DEPTH = 12, /* half */
    RT_BUF_MOTION = 13,        /* half2 */
    RT_BUF_NOISE_LEVEL = 14,   /* half, 8x8-tile grid */
    RT_BUF_NOISE_LEVEL16 = 15, /* half, 16x16-tile grid */
    RT_BUF_SKY = 16,           /* float4 512x256 */
    RT_BUF_SUN = 17,           /* float4 32x32 */
    RT_BUF_ALBEDO = 18,        /* half4 */
    RT_BUF_RGBA8 = 19,         /* uint8 x4, screen res: the last frame's output (CopyToOutput) */
    RT_BUF_HISTOGRAM = 20      /* uint32[64] luminance histogram (Histogram2) */
};
int rt_get_buffer(const rt_context* ctx, int name, void* dst, size_t bytes);
size_t rt_buffer_bytes(const rt_context* ctx, int name); /* 0 for names not available */

/* ---------------------------------------------------------------- hot-path stages */

/* BuildBvhLevel1 + BuildBvhLevel2 (bvh.cu:7-97): one per-frame two-level LBVH rebuild,
 * enqueued on the context stream (asynchronous). */
int rt_build_bvh(rt_context* ctx);

/* Animated geometry (no reference counterpart: the reference uploads its mesh once, init.cu:78-130,
 * and rebuilds the same LBVH every frame): new positions for vertices [first, first + count).
 *
 * Effect: afterwards the vertices, the smooth normals (recomputed for the whole mesh) and every
 * later LBVH build equal those of a context whose rt_init had been given the new positions; for the
 * normals that is the reference's frame-1 sequence, GenerateSmoothNormals run twice into an
 * un-cleared buffer, angle-weighted, accumulated in triangle order (kernel.cu:228-257, 313-327), bit
 * for bit.  rt_download(RT_ARR_VERTICES / RT_ARR_NORMALS) return the updated arrays.
 *
 * Scope: the topology (indices, triangle and batch counts) stays as it is; rt_set_mesh below
 * replaces it.  The update takes effect for every rt_build_bvh, explicit or inside a draw, enqueued after the call; frames already enqueued,
 * pipelined ones included, keep the geometry they were built from.  Nothing rebuilds by itself:
 * rt_trace_rays and rt_trace_primary still use the BVH of the last rt_build_bvh.
 *
 * Ordering inside the renderer: the update runs after the last build enqueued on any of the
 * renderer's streams, the next build on whichever stream waits for it, and work enqueued on the
 * context stream (rt_set_stream) after the call follows the read of the caller's buffer, so a
 * framework tensor allocated on that stream can be reused at once.
 *
 * rt_update_vertices: host positions (count xyz triples), copied synchronously into a staging
 * buffer of the renderer; the caller's array is free on return.
 * rt_update_vertices_device: caller-owned device memory (4-byte aligned); asynchronous, the host is
 * not synchronised.  ready_event NULL: the source is read after everything enqueued on the context
 * stream so far — always safe for data produced on that stream, but on a pipelined context it puts
 * the next frame's build behind the current frame's trace.  ready_event a hipEvent_t: the update
 * waits for that event only; a host that animates on a stream of its own records one there and keeps
 * the frames overlapped.  The source must stay unchanged until the update has read it (work
 * enqueued on the context stream after the call is behind that point).
 *
 * Each update advances the geometry epoch (0 after rt_init).  What synchronous draws prepare ahead —
 * the next frame's LBVH, its camera rays and shading — carries its epoch and is built or traced
 * again by a draw that finds another one, so no draw shows geometry older than the last update.
 *
 * Temporal passes: by default history reprojection is camera-only, as in the reference
 * (temporalDenoising.cuh), and moving geometry ghosts as it would there.  With geometry motion
 * vectors on (rt_set_geometry_motion below) RT_BUF_MOTION follows the vertices, and the temporal
 * filters fetch their history where the surface was.  Multi-GPU: every rank calls the update with
 * the same data.
 *
 * RT_ERR_ARG: NULL context or pointer, count == 0, first + count > vertexCount (rt_get_info), a
 * misaligned device pointer; RT_ERR_STATE before rt_init.  Like the other setters they never
 * return RT_ERR_DEVICE. */
int rt_update_vertices(rt_context* ctx, const float* xyz, uint32_t first, uint32_t count);
int rt_update_vertices_device(rt_context* ctx, const float* xyz_device, uint32_t first, uint32_t count,
                              void* ready_event);
int rt_get_geometry_epoch(const rt_context* ctx, uint64_t* epoch); /* 0 after rt_init, +1 per update / mesh set */

/* Run-time mesh replacement (no reference counterpart): a live context gets a new indexed mesh,
 * vertices and topology, stream-ordered like rt_update_vertices_device.
 *
 * Capacity: every mesh-sized buffer is allocated once, by rt_init, for [scene] maxTriangles /
 * maxVertices (absent or 0: the init mesh's counts, and then every allocation is what it was without
 * the keys).  maxTriangles <= 1024 * 1024 and its batch count ceil(maxTriangles / 1024) stays below
 * 1024.  Unparsable or negative values: RT_ERR_IO from rt_create; a capacity below the init mesh or
 * over the limits: RT_ERR_ARG from rt_init, before any device call.
 *
 * Effect: afterwards the vertices, the indices (padded to (n + 3) & ~3 triangles with index 0, as a
 * meshFile's are), the vertex -> corner adjacency (rt_mesh_adjacency), the smooth normals and every
 * LBVH build enqueued after the call, with every frame traced on those builds, equal those of a
 * context whose rt_init had been given this mesh, bit for bit.  rt_get_info (triCount,
 * triCountPadded, batchCount, vertexCount) and the mesh-level arrays (RT_ARR_VERTICES, INDICES,
 * NORMALS, TRI_MATERIALS, ADJ_OFFSETS, CORNER_SLOTS) follow the new mesh at once; the BVH arrays
 * (TRI_POS, TRI_NRM, AABBS, MORTON, REORDER, NODES, TLAS_*, BATCH_SCENE_AABBS, BVH_ARENA) keep the sizes
 * and contents of the last build until the next one, and rt_array_bytes answers accordingly.
 * Nothing rebuilds by itself, exactly as for vertex updates.
 *
 * Ordering: as for rt_update_vertices_device, for the index and adjacency arrays as for the
 * vertices: the set runs after the last build enqueued on any of the renderer's streams, the next
 * build waits for it, and the context stream follows the read of the caller's buffers.  Frames,
 * prebuilds and ray queries already enqueued keep the geometry and the counts of the build they
 * were issued on (each LBVH set carries its build's counts).  rt_set_mesh_device never synchronises
 * the host and drains no stream; rt_set_mesh validates the indices, copies both arrays into staging
 * buffers of the renderer (the caller's arrays are free on return) and takes the same device path.
 *
 * Interactions: the geometry epoch advances, so what a synchronous draw prepared ahead is
 * discarded.  The per-triangle material table returns to the default (3 everywhere) as after
 * rt_reset_triangle_materials, without a wait: launches already enqueued hold the old table, which is
 * not written.  With geometry motion vectors on, the first build after the call records no
 * displacement (the first-build rule).  Camera, frame number, exposure and history are untouched: a
 * host that wants no temporal reuse across the cut sets the frame index to 1.  Multi-GPU: every rank
 * calls with the same mesh.
 *
 * RT_ERR_ARG (checked in this order, NULL ctx / mesh first): a NULL or misaligned (4 B) array,
 * triangle_count < 2 or above the capacity, vertex_count == 0 or above the capacity (the capacity
 * checks need rt_init), and for rt_set_mesh an index >= vertex_count, with nothing changed.
 * RT_ERR_STATE before rt_init.  Never RT_ERR_DEVICE from the call itself: rt_set_mesh_device cannot
 * see its indices, so the kernel that copies them reads an index >= vertex_count as 0 (well defined,
 * never an out-of-bounds access) and counts them; the next checking call (rt_sync, rt_build_bvh, a
 * download) returns RT_ERR_DEVICE once, with the count in rt_last_error. */
typedef struct rt_mesh {
    const float* xyz;        /* vertex_count xyz triples */
    uint32_t vertex_count;
    const uint32_t* indices; /* 3 per triangle, each < vertex_count */
    uint32_t triangle_count;
    void* ready_event;       /* rt_set_mesh_device: hipEvent_t or NULL, as in rt_update_vertices_device */
} rt_mesh;
int rt_set_mesh(rt_context* ctx, const rt_mesh* host_mesh);
int rt_set_mesh_device(rt_context* ctx, const rt_mesh* device_mesh);
/* The vertex -> corner adjacency of an index array of padded_triangles triangles (host only, no
 * device or context needed; what rt_init builds and the device kernels of rt_set_mesh reproduce):
 * corner c (index c of the array) gets slot  adj_offsets[indices[c]] + #{c' < c : indices[c'] ==
 * indices[c]},  adj_corners is the inverse (slot -> corner: the corners in a stable sort by vertex),
 * adj_offsets[v] the first slot of vertex v and adj_offsets[vertex_count] = 3 * padded_triangles.
 * adj_corners or corner_slots may be NULL.  RT_ERR_ARG: a NULL indices / adj_offsets, vertex_count
 * == 0, or an index >= vertex_count. */
int rt_mesh_adjacency(const uint32_t* indices, uint32_t padded_triangles, uint32_t vertex_count,
                      uint32_t* adj_offsets, uint32_t* adj_corners, uint32_t* corner_slots);

/* Skinned meshes (no reference counterpart): linear-blend skinning on the device.  A skin is a bind
 * pose with up to RT_SKIN_INFLUENCES joints and weights per vertex; a pose is one 3 x 4 matrix per
 * joint (12 floats, row-major, translation in column 3: 48 bytes per joint and frame where
 * rt_update_vertices moves 12 bytes per vertex).  A rigid object is one joint with weight 1.
 *
 * The rule, in plain fp32 with one rounding per operation and nothing fused, for vertex v with rest
 * position p, joints j[0..3], weights w[0..3], and each output row r = 0, 1, 2:
 *     acc = +0
 *     for k = 0, 1, 2, 3 in this order:
 *         if w[k] == 0: continue                       (the joint's matrix is not read)
 *         t   = ((M[j[k]][r][0] * px + M[j[k]][r][1] * py) + M[j[k]][r][2] * pz) + M[j[k]][r][3]
 *         acc = acc + w[k] * t
 *     out[r] = acc
 * Weights are used as given: they are not normalised and need not sum to 1.  The skip is part of the
 * rule: a NaN matrix in a joint that no non-zero weight names reaches no vertex.  The identity pose
 * returns the rest position, except that a -0 component becomes +0.  rt_skin_vertices is the rule
 * compiled for the host (no context, no device); the kernel compiles the same text and gives its bits.
 *
 * rt_set_skin / rt_reset_skin are host-style setters like rt_set_materials: they wait for the
 * renderer's streams, drop what a synchronous draw traced ahead, and rt_set_skin copies the three
 * arrays into device buffers of the context (the caller's arrays are free on return).  The first set
 * allocates, by the vertex capacity ([scene] maxVertices): 48 bytes per vertex (rest 12, joints 8,
 * weights 16, skinned positions 12) and RT_SKIN_JOINTS_MAX * 48 bytes of matrix staging.  Setting a
 * skin moves no vertex and does not advance the geometry epoch.  A skin covers the whole mesh.
 * Checked in this order, and on an error nothing changes: RT_ERR_ARG for a NULL ctx or struct;
 * RT_ERR_ARG for a NULL array, vertex_count == 0 or joint_count outside 1..RT_SKIN_JOINTS_MAX;
 * RT_ERR_STATE before rt_init; RT_ERR_ARG for vertex_count != rt_get_info().vertexCount; RT_ERR_ARG
 * for a joint index >= joint_count (slots of weight 0 included) or a weight that is negative or not
 * finite; RT_ERR_HIP for a failed allocation or copy (a failed copy leaves the context without a skin
 * rather than with a mixed one).  Never RT_ERR_DEVICE.
 *
 * rt_pose_skin_device belongs to the family of rt_update_vertices_device: the host is never
 * synchronised and no stream is drained.  The skinning kernel runs on the update stream (the side
 * stream of a pipelined context, else the context stream) behind ready_event — or, with NULL, behind
 * everything enqueued on the context stream so far — and behind the builds and the update a vertex
 * update waits for; the whole-mesh vertex update follows it on the same stream, fed the rule's
 * positions.  From there on everything is as after rt_update_vertices_device(all vertices): normals,
 * epoch + 1, geometry motion, the context stream following the read of `matrices`, frames in flight
 * keeping their geometry, a draw's work ahead built and traced again.  `matrices` is caller-owned
 * device memory, 16-byte aligned, unchanged until read.  Matrices are not inspected: non-finite
 * results behave as non-finite positions given to rt_update_vertices_device do.
 * RT_ERR_ARG for a NULL ctx or struct, NULL or misaligned matrices; RT_ERR_STATE before rt_init or
 * without a skin; RT_ERR_ARG for joint_count != the skin's; RT_ERR_HIP for a failed launch.  Never
 * RT_ERR_DEVICE.
 * rt_pose_skin: host matrices, copied synchronously into the staging buffer once the previous update
 * has ended (rt_update_vertices' staging rule), then the device path; ready_event is ignored.
 *
 * Interactions: rt_set_mesh* drops the skin, which belonged to the old vertices: a pose is
 * RT_ERR_STATE until a new rt_set_skin.  rt_update_vertices* with a skin set simply override
 * positions until the next pose, which starts from the rest pose again.  Every rank of a multi-GPU
 * run calls with the same data.  A context that never calls rt_set_skin allocates and launches
 * exactly what it did without the feature. */
#define RT_SKIN_INFLUENCES 4
#define RT_SKIN_JOINTS_MAX 4096
typedef struct rt_skin {
    const float*    rest_xyz;     /* vertex_count xyz triples: the bind pose */
    const uint16_t* joints;       /* vertex_count x 4 */
    const float*    weights;      /* vertex_count x 4 */
    uint32_t vertex_count;        /* == rt_get_info().vertexCount: a skin covers the whole mesh */
    uint32_t joint_count;         /* 1 .. RT_SKIN_JOINTS_MAX */
} rt_skin;
typedef struct rt_pose {
    const float* matrices;        /* joint_count x 12 floats, row-major 3 x 4 */
    uint32_t joint_count;         /* == the skin's */
    void* ready_event;            /* device variant: hipEvent_t or NULL, as in rt_update_vertices_device */
} rt_pose;
int rt_set_skin(rt_context* ctx, const rt_skin* host);
int rt_reset_skin(rt_context* ctx);
int rt_get_skin(const rt_context* ctx, uint32_t* vertex_count, uint32_t* joint_count); /* 0, 0 without a skin */
int rt_pose_skin(rt_context* ctx, const rt_pose* host);
int rt_pose_skin_device(rt_context* ctx, const rt_pose* dev);
/* The rule on the host: xyz_out receives vertex_count xyz triples; `matrices` holds joint_count
 * matrices.  RT_ERR_ARG, with xyz_out untouched: a NULL pointer, vertex_count == 0, joint_count outside
 * 1..RT_SKIN_JOINTS_MAX, a joint index >= joint_count, a weight that is negative or not finite. */
int rt_skin_vertices(const rt_skin* host, const float* matrices, float* xyz_out);

/* Geometry motion vectors (no reference counterpart): off by default, and off nothing changes.  On,
 * the RT_BUF_MOTION G-buffer of a frame accounts for the vertices' displacement between the LBVH
 * build the frame is traced on and the build before it: a pixel whose sample 0 hit a triangle at
 * barycentrics (u, v) was at  pos - (d3 (1 - u - v) + d1 u + d2 v)  in the previous frame, d1..d3
 * the displacement of the triangle's corners between the two builds, and its motion vector is the
 * history camera's projection of that point less the sample's screen position (the camera-only
 * formula with the previous position in place of pos; NaN handling, bias and half packing as
 * before).  A pixel whose sample 0 missed keeps (0.5, 0.5).  A triangle whose corners did not move
 * gets the camera-only value bit for bit.
 *
 * Which builds record a displacement: one at another geometry epoch than the build before it, when
 * the feature was on at the first update between the two.  The first build of a context, a build at
 * the previous build's epoch (a synchronous draw's prebuild included) and the builds of a context
 * that never updates record none, and the path trace on them launches the kernels it launches with
 * the feature off.  Several updates between two builds are one displacement, from the previous
 * build's positions to the last update's.  Only the first rt_path_trace enqueued on a build applies
 * it: a host that builds once and traces several frames sees geometry that did not move between
 * them.  What a synchronous draw traces ahead for the next frame never carries one; when a draw
 * discards that and traces again, the repeat is the frame's one path trace.
 *
 * rt_set_geometry_motion waits for the streams like the other setters, allocates its buffers on the
 * first enable (one position array, one displacement record per triangle and LBVH set) and takes
 * effect from the next build.  [render] geometryMotion = true | false sets the initial state.
 * RT_ERR_ARG: NULL argument; RT_ERR_STATE: rt_set_geometry_motion before rt_init; RT_ERR_HIP: the
 * buffers cannot be allocated.  Never RT_ERR_DEVICE. */
int rt_set_geometry_motion(rt_context* ctx, int on);
int rt_get_geometry_motion(const rt_context* ctx, int* on);

/* Emitter sampling: next-event estimation of the emissive triangles of a custom material table
 * (DESIGN.md §4.1.6).  Off by default, and then nothing changes.  The path tracer takes one light sample
 * per diffuse interaction; with emitter sampling on, that sample goes with probability `probability`
 * (q) to an emitting triangle and otherwise to the sun or sky as before, whose pdf is scaled by 1 - q.
 * q is the emitters' counterpart of the reference's sky-against-sun choice; it counts as 0 while the
 * list is empty.
 *
 * The emitter list is built on the device behind every LBVH build while the feature is on and a custom
 * material table (rt_set_materials) holds an EMISSIVE entry with non-zero emission; otherwise a frame
 * launches exactly the kernels it launches without the feature.  Triangle t of the build is an emitter
 * when the id the path tracer reads for it ([render] materialOverride, else its rt_set_triangle_materials*
 * entry, else 3) has type EMISSIVE and its weight, area x (0.2126 r + 0.7152 g + 0.0722 b) of the entry's
 * emission, is > 0.  An emitter is selected in proportion to its weight and a point on it uniformly by
 * area; emitters are two-sided, as a camera ray sees them.  A shadow ray towards an emitter lights its
 * sample only when its closest hit is exactly that triangle.
 *
 * The list belongs to the build: it follows rt_update_vertices* and rt_set_mesh* (areas) and the
 * triangle ids set on the device, and frames in flight keep the list of the build they trace.  A change
 * of the material table or of the triangle ids shows in the list at the next build, which draws do every
 * frame; until then a listed triangle that stopped emitting reads as occluded, and a new emitter is
 * reached by bounce rays only.
 *
 * rt_set_emitter_sampling waits for the streams like the other setters (what a synchronous draw traced
 * ahead is dropped), allocates the list buffers on the first enable, by the triangle capacity, and takes
 * effect from the next LBVH build.  Meshes of more than 2^20 triangles get no list.
 * Errors, in this order, with nothing changed: RT_ERR_ARG: NULL argument; RT_ERR_ARG: probability not
 * finite or outside [0, 1]; RT_ERR_STATE: rt_set_emitter_sampling before rt_init; RT_ERR_HIP: the
 * allocation failed. */
int rt_set_emitter_sampling(rt_context* ctx, int on, float probability);
int rt_get_emitter_sampling(const rt_context* ctx, int* on, float* probability);
/* The device kernels' own statement of the two rules, compiled for the host (no context).
 * rt_emitter_weight: the weight of the triangle xyz = v0 | v1 | v2 under `emission`, in fp32:
 * 0.5 |(v1 - v0) x (v2 - v0)| x luminance.  rt_emitter_select: the slot that r in [0, 1) selects from
 * the inclusive CDF of `count` >= 1 weights, the first whose CDF value is >= r * cdf[count - 1], and the
 * probability the CDF gives it, (cdf[slot] - cdf[slot - 1]) / cdf[count - 1].  RT_ERR_ARG: NULL
 * argument, or count 0. */
int rt_emitter_weight(const float xyz[9], const float emission[3], float* weight);
int rt_emitter_select(const float* cdf, uint32_t count, float r, uint32_t* slot, float* prob);

/* Per-triangle materials: SceneMaterial::materialsIdx (kernel.cuh:198-203, init.cu:261-269), the
 * material id the path tracer looks up at every hit (traverse.cuh:29-32).  ids[k] is the material of
 * triangle first + k, the objectIdx a hit reports; [first, first + count) lies within triCount
 * (rt_get_info) of the current mesh (rt_set_mesh resets the table).  Ids 0..9 index the reference's
 * material table (0, 2: emissive; 1: glass; 3, 6..9: Lambertian; 4: microfacet; 5: mirror); an id
 * >= 10 is the reference's out-of-range default, a mirror whose material mask is the id.  The mask
 * of RT_BUF_COLOR is the id of sample 0's triangle, which the denoiser's *_sigma_material weights
 * compare.
 *
 * Before the first set, and after rt_reset_triangle_materials, the table is the reference's: 3 for
 * every triangle, and the path trace launches exactly the kernels it launched before this call
 * existed.  The first set allocates one device byte per triangle (initialised to 3) and a host copy,
 * from which the census of ids, and with it the kernel variants a frame needs
 * (rt_material_classes), is taken without a device read.  A table of Lambertian and emissive ids
 * keeps the default kernels; one mirror or glass triangle puts the frame on the glossy ones.
 *
 * Both calls wait for the renderer's streams like the other setters, drop what a synchronous draw
 * traced ahead, and take effect for every path trace enqueued after them; they are not
 * stream-ordered.  [render] materialOverride >= 0 still wins over the table.
 * RT_ERR_ARG: NULL ctx or ids, count == 0, first + count > triCount; RT_ERR_STATE before rt_init;
 * RT_ERR_HIP: the allocation or the copy failed.  Never RT_ERR_DEVICE. */
int rt_set_triangle_materials(rt_context* ctx, const uint8_t* ids, uint32_t first, uint32_t count);
int rt_reset_triangle_materials(rt_context* ctx);
#define RT_MAT_CLASS_GLOSSY 1u      /* an id whose type is mirror or glass: 1, 5, and every id >= 10 */
#define RT_MAT_CLASS_MICROFACET 2u  /* id 4 */
/* The kernel classes of a set of ids (the OR over ids[0..n)); host only, no device or context
 * needed.  RT_ERR_ARG: classes NULL, or ids NULL with n > 0. */
int rt_material_classes(const uint8_t* ids, size_t n, uint32_t* classes);

/* The same set from device memory, stream-ordered: the counterpart of rt_update_vertices_device and
 * rt_set_mesh_device for the material table.  The host is never synchronised and no stream is
 * drained.  ids is read after ready_event (a hipEvent_t), or after everything enqueued on the
 * context stream so far when it is NULL; work enqueued on the context stream after the call follows
 * that read.  The new table (the previous one, or 3 everywhere after rt_set_mesh* or a reset, with
 * [first, first + count) replaced) holds for every rt_path_trace enqueued after the call, explicit
 * or inside a draw; path traces enqueued before it, pipelined frames in flight and what a
 * synchronous draw traced ahead included, keep the table they were launched with, and the next draw
 * traces again what was traced ahead.  The intended streaming sequence is rt_set_mesh_device,
 * rt_set_triangle_materials_device, rt_build_bvh, a draw, with no wait in it.
 *
 * classes: the host cannot see the ids, and the path tracer picks its kernel variants from their
 * classes, so the caller declares them: RT_MAT_CLASS_* bits (rt_material_classes is the rule) that
 * bound the classes of EVERY id the table holds after the update, the carried-over ones included.
 * Later frames launch exactly the kernels of the declared bits.  Declaring too much costs speed only
 * and changes no pixel.  Declaring too little is a caller error handled like an index past the
 * vertex count in rt_set_mesh_device: the kernel stores id 3 in place of every id of an undeclared
 * class, carried-over ones too, and counts them; the next checking call (rt_sync, rt_build_bvh, a
 * draw, a download) returns RT_ERR_DEVICE once, with the count in rt_last_error.
 *
 * Afterwards the host setter's copy is stale: rt_set_triangle_materials reads the table back before
 * it applies its range (it waits for the streams anyway), and its census is exact again.
 * RT_ARR_TRI_MATERIALS returns the current table and RT_ARR_TRI_MATERIAL_CENSUS its triangle count
 * per id.  Every rank of a multi-GPU run calls with the same data.  The first call of a context
 * allocates the table buffers (four of one byte per triangle of the capacity) and may block in the
 * allocator; later calls only enqueue work.
 * Checked in this order: RT_ERR_ARG for NULL ctx or u, NULL ids, count == 0, unknown bits in classes;
 * RT_ERR_STATE before rt_init; RT_ERR_ARG for first + count > triCount of the current mesh;
 * RT_ERR_HIP for a failed allocation or launch.  On an error nothing is changed.  Never
 * RT_ERR_DEVICE from the call itself. */
#define RT_MAT_CLASS_ALL (RT_MAT_CLASS_GLOSSY | RT_MAT_CLASS_MICROFACET)
typedef struct rt_material_update {
    const uint8_t* ids;    /* device memory, count bytes, no alignment demanded */
    uint32_t first, count; /* triangles [first, first + count) of the current mesh */
    uint32_t classes;      /* RT_MAT_CLASS_* bits: the caller's bound on the WHOLE table after this update */
    void* ready_event;     /* hipEvent_t or NULL, as in rt_update_vertices_device */
} rt_material_update;
int rt_set_triangle_materials_device(rt_context* ctx, const rt_material_update* u);
/* The class of one id (its low 8 bits) as the device kernel of rt_set_triangle_materials_device
 * computes it: the kernel's own statement of the rule, compiled for the host, so that a test can pin
 * it to rt_material_classes.  No context needed. */
uint32_t rt_material_class_rule(uint32_t id);

/* The material table: what a material id means.  Ids are 0..255 (the range of the per-triangle
 * table's uint8).  rt_default_material(id) is the reference's meaning of the id (init.cu:215-251 over
 * the SurfaceMaterial defaults): the type of ids 0..9 as listed above and RT_MAT_MIRROR for 10..255,
 * flags 0, color 1, emission 0, ior 1.33f, alpha 0.05f, f0 (0.56f, 0.57f, 0.58f); host only, no
 * context.  Before the first rt_set_materials and after rt_reset_materials the context has no custom
 * table: rt_get_materials returns the defaults and the path trace launches exactly the kernels it
 * launched before these calls existed.  rt_set_materials replaces entries [first_id, first_id + count)
 * and leaves the others as they were (the defaults, on the first call).
 *
 * Shading, each rule the identity at the default values, bit for bit:
 *   diffuse types (Lambertian, microfacet), flags 0: albedo = (triplanar soil albedo) * color,
 *     component-wise, once, behind the three-plane sum and ahead of every use of the albedo;
 *   RT_MAT_FLAG_FLAT: no texture at all: albedo = color and the shading normal stays the hit's
 *     interpolated smooth normal; light sampling, MIS and the throughput are unchanged code;
 *   microfacet: f0 and alpha are the entry's; glass: etaT = ior; mirror: no parameter;
 *   emissive: a path that ends on the hit (a camera or bounce ray, not an occluded shadow ray) carries
 *     `emission` where a sky hit carries the environment, ahead of the path tracer's clamp at 10.
 *     By default emitters are not sampled as lights: shadow rays towards the sun or sky that hit an
 *     emitter stay occluded, and an emitter lights the scene only through the bounce rays that land on
 *     it.  rt_set_emitter_sampling (below) adds next-event estimation of the emissive triangles.
 * The mask of RT_BUF_RENDER_COLOR stays the id, and [render] materialOverride still chooses the id,
 * whose entry then supplies the parameters (its low 8 bits index the table).
 *
 * Kernels: while a custom table is active every frame runs one table-reading variant of the shading
 * kernels, instantiated on the all-classes (glossy and microfacet) kernels only, on the unsplit
 * four-kernel bounce plan; the class of an id follows its entry's type, so rt_material_classes no
 * longer selects anything and rt_set_triangle_materials_device records RT_MAT_CLASS_ALL as the
 * declared classes (its kernel replaces and counts nothing).  This is deliberate: one new
 * instantiation per kernel instead of one per class combination.  It costs a Lambertian-only custom
 * table some speed and no pixel.  After a later rt_reset_materials a device-set triangle table keeps
 * the all-classes kernels until ids are set again.
 *
 * rt_set_materials and rt_reset_materials behave like rt_set_triangle_materials: they wait for the
 * renderer's streams, drop what a synchronous draw traced ahead and take effect for every path trace
 * enqueued afterwards; they are not stream-ordered.  The table belongs to the context, not the mesh:
 * rt_set_mesh* resets the per-triangle ids to 3 and leaves it alone.  Every rank of a multi-GPU run
 * calls with the same data.  The first rt_set_materials allocates the device table (256 records of
 * 64 bytes).
 * On any error nothing changes.  Checked in this order: RT_ERR_ARG for NULL ctx, m or out, count == 0,
 * first_id + count > 256, an entry with type outside 0..4, unknown flag bits, a non-finite or negative
 * color or emission component, ior not finite or <= 0, alpha not in (0, 1], an f0 component not in
 * [0, 1]; RT_ERR_STATE before rt_init; RT_ERR_HIP for a failed allocation or copy.  Never
 * RT_ERR_DEVICE. */
#define RT_MAT_LAMBERTIAN 0
#define RT_MAT_MIRROR     1
#define RT_MAT_GLASS      2
#define RT_MAT_MICROFACET 3
#define RT_MAT_EMISSIVE   4
#define RT_MAT_FLAG_FLAT  1u   /* diffuse types: no soil texture */
typedef struct rt_material {
    int32_t  type;      /* RT_MAT_* */
    uint32_t flags;     /* RT_MAT_FLAG_* */
    float color[3];     /* diffuse types: multiplies the albedo (textured) or is the albedo (flat) */
    float emission[3];  /* EMISSIVE: radiance of a hit, before the path tracer's clamp at 10 */
    float ior;          /* GLASS: etaT (the reference's 1.33f) */
    float alpha;        /* MICROFACET: GGX alpha (0.05f) */
    float f0[3];        /* MICROFACET: (0.56f, 0.57f, 0.58f) */
} rt_material;
int rt_default_material(uint32_t id, rt_material* out);
int rt_set_materials(rt_context* ctx, uint32_t first_id, uint32_t count, const rt_material* m);
int rt_get_materials(const rt_context* ctx, uint32_t first_id, uint32_t count, rt_material* out);
int rt_reset_materials(rt_context* ctx);

/* BASELINE config 2: GenerateRay + RaySceneIntersect for every render pixel with the
 * blue-noise sample of frame_num (pathtrace.cuh:116-130), enqueued asynchronously.
 * with_detail != 0 also stores normals / shading normals / traversal counters. */
int rt_trace_primary(rt_context* ctx, int frame_num, int with_detail);

/* PathTrace (pathtrace.cuh:11-128) for frame_num into the G-buffers (RT_BUF_RENDER_COLOR,
 * NORMAL, ALBEDO, DEPTH, MOTION), after UpdateFrame's sky/sun regeneration when the sky
 * parameters changed (kernel.cu:286-307).  spp > 1 ([render] spp) averages spp reference
 * samples (frame indices spp*(frame_num-1)+1 ...).  with_detail != 0 also stores the per-pixel
 * traced-ray count (RT_ARR_RAYS).  Asynchronous; the history camera advances (kernel.cu:357). */
int rt_path_trace(rt_context* ctx, int frame_num, int with_detail);

/* TemporalSpatialDenoising + PostProcessing + CopyToOutput (denoising.cu:5-189,
 * postprocessing.cu:5-161, kernel.cu:376-381) on the G-buffers of the last rt_path_trace, for
 * frame_num (frame 1 skips the temporal passes).  Afterwards RT_BUF_RENDER_COLOR holds the
 * denoised HDR colour and RT_BUF_SCALED_COLOR the tone-mapped screen image; the RGBA8 image and
 * (with_hdr) a float4 HDR copy are kept on the device for rt_draw.  Asynchronous. */
int rt_denoise_post(rt_context* ctx, int frame_num, int with_hdr);

/* Traced rays (RaySceneIntersect calls that ran a traversal) accumulated since the last reset. */
int rt_get_ray_count(rt_context* ctx, uint64_t* rays, int reset);

/* Enqueue every later stage on `stream` (a hipStream_t, e.g. the caller's framework stream so
 * its collectives order with the renderer).  NULL is the device's null stream (a framework's
 * default stream, e.g. torch's, is that stream); RT_OWN_STREAM restores the context's own. */
#define RT_OWN_STREAM ((void*)(intptr_t)-1)
#define RT_STREAM_OFF ((void*)(intptr_t)-2) /* rt_set_gather_stream: no gather stream */
int rt_set_stream(rt_context* ctx, void* stream);

/* Frame pipelining (no reference counterpart; the reference draws frames strictly one after
 * another): with a post stream set, rt_denoise_post runs the denoiser and post chain on that
 * stream, after everything enqueued on the context stream so far (path trace, G-buffer
 * gathers), and the path tracer alternates between two G-buffer sets, so the trace of frame
 * f+1 overlaps the denoise of frame f; the LBVH build and camera rays of the next frame run on
 * an internal third stream beside the current frame's trace kernels (two LBVH sets,
 * RT_GBUFFER_SETS G-buffer sets).  Results are identical to the serial order.  Host reads
 * (rt_get_buffer, rt_download, rt_sync, rt_draw's copies) wait for all streams.  NULL turns it off.
 * rt_info.gbufferSet names the set the last path trace wrote; bind the other sets' buffers
 * with name | RT_BUF_SET1 / RT_BUF_SET2 / RT_BUF_SET3. */
#define RT_GBUFFER_SETS 4
#define RT_BUF_SET1 0x100
#define RT_BUF_SET2 0x200
#define RT_BUF_SET3 0x300
int rt_set_post_stream(rt_context* ctx, void* stream);

/* Multi-GPU gathers off the trace chain (no reference counterpart): each later rt_denoise_post
 * also waits for the work enqueued on `stream` up to that call, so a host that gathers a
 * frame's G-buffer rows on its own stream (after the path trace; rtx/dist.py) keeps the next
 * frame's path trace free of the collective.  The gathers must not write a G-buffer set the
 * renderer is still using: gather the set rt_info.gbufferSet names, right after its path trace.
 * NULL is the null stream (as in rt_set_stream); RT_STREAM_OFF (the default) turns it off. */
int rt_set_gather_stream(rt_context* ctx, void* stream);

/* Multi-GPU strip-local denoise (no reference counterpart, the reference runs on one
 * GPU).  With stripCount > 1 and a hook set, each rank runs the denoise/post chain only for its own
 * contiguous rows [rowBegin, rowEnd) — the frame's 64-row blocks split evenly over the ranks — plus
 * the halo rows its passes read (the summed stencil radius, ~64 rows each side), instead of the
 * whole frame.  Two exchanges per frame make the result identical to one GPU; the renderer asks the
 * host to enqueue them on `stream` (the stream the denoise runs on) through the hook:
 *   RT_HOOK_HISTOGRAM  sum the ranks' 64-bin histograms (RT_BUF_HISTOGRAM) in place (all-reduce)
 *                      before AutoExposure reads them;
 *   RT_HOOK_ROWS       give every rank every rank's rows [rowBegin, rowEnd) of the accumulation
 *                      buffer, of history buffer `historySet` (the final HDR of the frame) and of the
 *                      RGBA8 output (all-gather), before the next frame's temporal passes read them.
 * The host binds those buffers to its own device memory (rt_bind_buffer: RT_BUF_ACCUMULATION,
 * RT_BUF_HISTORY_COLOR sets 0 and 1, RT_BUF_HISTOGRAM, RT_BUF_RGBA8) so its collectives move them
 * in place (rtx/dist.py StripDenoise).  The hook returns 0 on success.  Without a hook (or with the
 * noise visualisation, bloom or lens flare on) every rank denoises the whole frame. */
typedef struct rt_strip_exchange {
    int32_t frameNum;
    int32_t rowBegin, rowEnd;   /* this rank's rows */
    int32_t historySet;         /* history buffer (0 / 1) TemporalFilter2 wrote this frame */
    int32_t gbufferSet;         /* G-buffer set the frame was traced into (RT_HOOK_GBUFFERS) */
    int32_t stripLocal;         /* 1: the denoise is strip-local (rt_info.stripLocalDenoise) */
} rt_strip_exchange;
#define RT_HOOK_HISTOGRAM 0
#define RT_HOOK_ROWS 1
/* Optional third stage (rt_set_hook_stages): before the denoise, give every rank the G-buffer rows its
 * denoise reads (rt_info.gbufferRowBegin/End of each rank; the whole frame when stripLocal is 0) from
 * the ranks that traced them, in G-buffer set gbufferSet — what rtx/dist.py's StripGather does outside
 * the renderer.  With it, rt_draw and rt_draw_device run a multi-GPU frame by themselves
 * (include/rtx_dist.h implements all three stages). */
#define RT_HOOK_GBUFFERS 2
typedef int (*rt_collective_fn)(void* arg, int stage, void* stream, const rt_strip_exchange* x);
int rt_set_collective_hook(rt_context* ctx, rt_collective_fn fn, void* arg);
/* which stages the hook is called for: bit (1 << RT_HOOK_*); default HISTOGRAM | ROWS.  HISTOGRAM and
 * ROWS are mandatory whenever a strip-local denoise runs (a mask without either is refused with
 * RT_ERR_ARG); the mask only opts into RT_HOOK_GBUFFERS. */
int rt_set_hook_stages(rt_context* ctx, uint32_t stage_mask);

/* Use caller-owned device memory (>= the buffer's size at the largest render size, i.e.
 * maxWidth x maxHeight with dynamic resolution, else rt_buffer_bytes; 16-B aligned) as one of the path-trace
 * G-buffers (RT_BUF_RENDER_COLOR / NORMAL / ALBEDO / DEPTH / MOTION), e.g. so a multi-GPU host
 * can all-gather screen strips in place; and the strip-local denoise's exchanged buffers
 * (RT_BUF_ACCUMULATION, RT_BUF_HISTORY_COLOR | RT_BUF_SET1 for the second of the pair,
 * RT_BUF_HISTOGRAM, RT_BUF_RGBA8), whose current contents are copied over.  The memory must
 * outlive the context's use of it.
 * A G-buffer name carries its set (RT_BUF_SET1..3; none: set 0).  Pipelined frames cycle through all
 * RT_GBUFFER_SETS sets, so such a host binds every set.  A synchronous context (no post stream) with a
 * bound G-buffer launches nothing ahead and traces every later frame into set 0, whichever set its
 * draws had alternated into before the bind: binding set 0 is enough there, and rt_get_info's
 * gbufferSet reads 0 from the bind on. */
int rt_bind_buffer(rt_context* ctx, int name, void* device_ptr, size_t bytes);

/* wait for all work on the context stream */
int rt_sync(rt_context* ctx);

/* HIP-event timing on the context stream: runs `iters` back-to-back launches of a stage
 * (0 = BVH build, 1 = primary rays, 2 = path trace, 3 = full frame: BVH + path trace + denoise
 * + post, 4 = denoise + post, 5 = a whole-mesh vertex update with its smooth normals, fed the
 * current positions from a copy: arrays and epoch stay as they are, 6 = a whole-mesh set (rt_set_mesh_device)
 * fed the current mesh from a copy, arrays and epoch likewise left as they are, 7 = one sky-set
 * generation into a spare set, under the environment when one is active, the current set and its serial
 * left as they are, 8 = one whole-mesh pose of the skin (RT_ERR_STATE without one): the skinning kernel
 * under the matrices of the last rt_pose_skin (identity if there was none since rt_set_skin) and the
 * whole-mesh vertex update behind it, which like stage 5 is fed the current positions from a copy, so
 * arrays and epoch stay as they are) and returns the total milliseconds between the first launch and the end of the last. */
int rt_time_stage(rt_context* ctx, int stage, int iters, float* total_ms);

/* Stage 6 split by HIP events between its launches: `iters` whole-mesh sets one after the other,
 * parts_ms[0..2] = the summed milliseconds of the index ingest, of the adjacency kernels and of the
 * whole-mesh normals update.  Measurement aid (tools/mesh_probe.py); waits for the streams. */
int rt_time_mesh_set(rt_context* ctx, int iters, float* parts_ms);

/* Test entry (no reference counterpart): the denoiser's packed-pair transcendentals (rtmath_pk.h)
 * beside their scalar rtmath.h forms, over a caller-owned device array x of n floats (element i
 * is paired with i ^ 1).  fn 0: pow(x, y) (x finite >= 0, y finite > 0), 1: expf(x), 2: x / y
 * through c = RN(1 / y) (rt_div_rcp).  out_pk / out_scalar (device, n floats each) receive the two
 * results, which must agree bit for bit.  Null stream, synchronising; RT_ERR_ARG on bad arguments. */
int rt_debug_pk_math(int fn, const float* x, float y, float c, float* out_pk, float* out_scalar, size_t n);

/* HIP-event split of the path-trace stage (stage 2 above): runs `iters` path traces with an
 * event recorded between consecutive kernels and writes the average milliseconds of each kernel
 * (n >= 7: camera, shade, trace bounce queue, resume, trace shadow queue, resume, resolve).
 * Measurement aid for the roofline in bench.py; no reference counterpart. */
int rt_time_path_trace_kernels(rt_context* ctx, int iters, float* kernel_ms, int n);

/* The same split over `iters` whole frames (LBVH build + path trace + denoise/post of frames
 * first_frame, first_frame + 1, ...) run exactly as a caller runs them: on a pipelined context
 * (rt_set_post_stream) each kernel is timed on the stream it runs on, beside the other streams'
 * work.  With n >= 15 entries 7..14 are the denoise / post chain's kernels (TemporalFilter,
 * SpatialFilter7x7, the three a-trous passes, TemporalFilter2, the DownScale4 / histogram /
 * AutoExposure chain, the scale / sharpen / tone map / dither pass), each averaged over the frames
 * that launched it.  Waits for the frames.  Measurement aid for bench.py's per-kernel roofline. */
int rt_time_frame_kernels(rt_context* ctx, int first_frame, int iters, float* kernel_ms, int n);

/* The same split recorded inside the caller's own frames: the next `frames` frames (each a path
 * trace and the rt_denoise_post that follows it) bracket the kernels whose bit is set in
 * kernel_mask (bit k = kernel k, the 15 kernels above) with HIP events on the stream each runs on
 * (two events per kernel, no synchronisation); rt_frame_marks_read waits, writes the per-kernel
 * average milliseconds over the frames recorded (n >= 7 entries, up to 15; -1 for kernels not
 * marked) and stops recording.  bench.py's warm-up and timed frames use it. */
int rt_frame_marks_begin(rt_context* ctx, int frames, uint32_t kernel_mask);
int rt_frame_marks_read(rt_context* ctx, float* kernel_ms, int n, int* frames_recorded);

/* Copies device arrays to host (debug dumps of bvh.cu:15-96, traversal outputs). */
enum rt_array_name {
    RT_ARR_VERTICES = 0,         /* float[nv][3] */
    RT_ARR_INDICES = 1,          /* uint32[triCountPadded][3] */
    RT_ARR_NORMALS = 2,          /* float[nv][3] (smooth normals) */
    RT_ARR_TRI_POS = 3,          /* float4[triCountPadded][3] */
    RT_ARR_AABBS = 4,            /* float[triCountPadded][6] min xyz max xyz */
    RT_ARR_MORTON = 5,           /* uint32[B*1024] sorted codes (morton2.csv) */
    RT_ARR_REORDER = 6,          /* uint32[B*1024] (reorderIdx.csv) */
    RT_ARR_NODES = 7,            /* 64-B nodes [triCountPadded]: lmin lmax rmin rmax (12 f32), idxL idxR leafL leafR */
    RT_ARR_TLAS_AABBS = 8,       /* float[B][6] */
    RT_ARR_TLAS_MORTON = 9,      /* uint32[1024] sorted */
    RT_ARR_TLAS_REORDER = 10,    /* uint32[1024] */
    RT_ARR_TLAS_NODES = 11,      /* 64-B nodes [B] */
    RT_ARR_TLAS_SCENE_AABB = 12, /* float[6] */
    RT_ARR_BATCH_SCENE_AABBS = 13, /* float[B][6] */
    RT_ARR_HITS = 14,            /* float4[W*H]: t, objectIdx (int bits), u, v */
    RT_ARR_HIT_NORMALS = 15,     /* float4[W*H]: geometric normal, hit flag */
    RT_ARR_HIT_FAKE_NORMALS = 16,/* float4[W*H]: shading normal, ray offset */
    RT_ARR_HIT_STATS = 17,       /* uint32[W*H][4]: node visits, tri tests, dropped pushes, iterations */
    RT_ARR_TRI_NRM = 18,         /* float4[triCountPadded][3] */
    RT_ARR_RAYS = 19,            /* uint32[W*H] traced rays per pixel (rt_path_trace with_detail) */
    RT_ARR_SKY_PDF = 20,         /* float[131072] sky luminance (Sky kernel, sky.cuh:296-297) */
    RT_ARR_SKY_CDF = 21,         /* float[131072] inclusive scan of the sky pdf */
    RT_ARR_SUN_PDF = 22,         /* float[1024] */
    RT_ARR_SUN_CDF = 23,         /* float[1024] */
    RT_ARR_SUN_DIR = 24,         /* float[4]: sunDir xyz, cos(sun half-angle) (host values) */
    RT_ARR_HISTOGRAM = 25,       /* uint32[64] luminance histogram (Histogram2) */
    RT_ARR_EXPOSURE = 26,        /* float[4] exposure, adapted lum, bright lum, bright bin lum */
    RT_ARR_COLOR4 = 27,          /* half4 [ceil(W/4) * ceil(H/4)] DownScale4 chain */
    RT_ARR_COLOR16 = 28,         /* half4 [ceil(W/16) * ceil(H/16)] */
    RT_ARR_COLOR64 = 29,         /* half4 [ceil(W/64) * ceil(H/64)] */
    RT_ARR_RGBA8 = 30,           /* uint8[Ws*Hs][4] final output of the last rt_draw / rt_denoise_post */
    RT_ARR_PT_QUEUE = 32,        /* uint32[64] path-trace wavefront counters of the last launch: [0] rays
                                    deferred at step 3, [1] at step 4, [4] pixels resolved late,
                                    [8]/[9] longest traversal (iterations) of the step-3/4 queues
                                    (detail launches only), [10] internal errors (must be 0),
                                    [11] pixels with a sample that hit geometry; detail launches
                                    also: node visits / triangle tests of [12,13] the camera
                                    kernel, [14,15] the shade kernel (inline glossy traces),
                                    [16,17] the step-3 and [18,19] the step-4 queue tracers,
                                    diffuse events of [20] the shade and [21] the resume<3> kernel,
                                    [22] camera rays settled by the scene cull (no traversal);
                                    [23] entries of the step-3 queue's shading list (bounce rays that
                                    hit a triangle; 0 when resume<3> runs unsplit or as the fused chain) */
    RT_ARR_PT_Q3_ORIGINS = 33,   /* float4[cap] step-3 queue rays of the last launch: origin xyz, pixel bits */
    RT_ARR_PT_Q3_DIRS = 34,      /* float4[cap] direction xyz, flags bits ([0] of RT_ARR_PT_QUEUE are valid).
                                    Flags: bit 0 the entry is a shadow ray, bits 1..6 its sample index; bit 7
                                    (emitter sampling only) the shadow ray samples an emitter, and then bits
                                    8..31 are that light's triangle index; without bit 7, bits 16..31 are the
                                    light id: 7777 none (a bounce ray), 9999 the environment */
    RT_ARR_PT_Q4_ORIGINS = 35,   /* float4[cap] step-4 queue, same layout ([1] valid) */
    RT_ARR_PT_Q4_DIRS = 36,
    RT_ARR_PT_STATS = 31,        /* uint32[W*H][4] rays, node visits, triangle tests, diffuse events
                                    (rt_path_trace with_detail) */
    RT_ARR_TEX_ALBEDO_AO = 37,   /* ushort4, 11-level mip chain of 1024^2 (levels concatenated, 1024 -> 1) */
    RT_ARR_TEX_NORMAL_ROUGHNESS = 38, /* ushort4, same layout */
    RT_ARR_TEX_HEIGHT = 39,      /* ushort, same layout (zero unless uploaded) */
    RT_ARR_HDR = 40,             /* float4[W*H] pre-tone-map HDR of the last rt_draw / rt_denoise_post with_hdr */
    RT_ARR_BVH_ARENA = 41,       /* the traversal's record arena as the device holds it (64-B records: B*1024 BLAS
                                    nodes, B TLAS nodes, triCountPadded triangle records); the
                                    NODES / TLAS_NODES / TRI_POS arrays are views of it in the reference layout */
    RT_ARR_TRI_MATERIALS = 42,   /* uint8[triCount] material id per triangle (rt_set_triangle_materials); all 3
                                    before the first set and after a reset */
    RT_ARR_ADJ_OFFSETS = 43,     /* uint32[nv + 1] first slot of each vertex in the vertex -> corner adjacency
                                    (rt_mesh_adjacency) */
    RT_ARR_CORNER_SLOTS = 44,    /* uint32[3 * triCountPadded] each corner's slot in it */
    RT_ARR_TRI_MATERIAL_CENSUS = 45, /* uint32[256] triangles per material id of the current table over [0, triCount):
                                    the device census after rt_set_triangle_materials_device, the host's after
                                    rt_set_triangle_materials, triCount at id 3 without a table */
    /* the emitter list of the last LBVH build (rt_set_emitter_sampling); all three have size 0 while
       emitter sampling is off or that build wrote no list */
    RT_ARR_EMITTER_TRIS = 46,    /* uint32[count] the emitting triangles, ascending */
    RT_ARR_EMITTER_WEIGHTS = 47, /* float[count] their weights (rt_emitter_weight) */
    RT_ARR_EMITTER_CDF = 48,     /* float[P] the reference Scan (inclusive, block 256) of the weights zero-padded
                                    to P, the power of two >= max(triCount, 256); P from rt_array_bytes */
    RT_ARR_PT_Q3_BETA = 49,      /* float4[cap] step-3 queue: the first diffuse interaction's throughput beta1 xyz,
                                    ray-cone spread ([0] of RT_ARR_PT_QUEUE are valid) */
    RT_ARR_SPEC_STATS = 50,      /* uint32[4] the synchronous draws' launches ahead (rt_draw), counted on the host
                                    since rt_init: [0] launched, [1] reused by the next draw, [2] dropped unused
                                    (the next draw's launch parameters differed, the sky tables were regenerated,
                                    or a call waited for the streams), [3] 1 while one awaits the next draw;
                                    [0] == [1] + [2] + [3].  Host state: the read waits for nothing and drops
                                    nothing.  All zero with [tuning] syncSpec off; pipelined frames add nothing */
    RT_ARR_PSEUDO_NORMALS = 51   /* float4[triCount][6] the pseudo-normal table of the last LBVH build
                                    (rt_set_signed_distance): per triangle vertex 1 2 3, edge 12 23 31, .w = 0;
                                    size 0 while that build wrote none */
};
/* RT_ARR_TEX_ALBEDO_AO and RT_ARR_TEX_NORMAL_ROUGHNESS OR-ed with RT_ARR_TEX_SET(k) name the chain of
 * texture set k (k = 0 is the plain name); a k past the context's sets is RT_ERR_ARG (rt_array_bytes: 0). */
#define RT_ARR_TEX_SET(k) ((k) << 8)
int rt_download(const rt_context* ctx, int what, void* dst, size_t bytes);

/* Batch ray query: the reference's RaySceneIntersect traversal (traverse.cuh:107-253, the
 * closest hit of TraverseBvh with its 16-entry stack and 1024-iteration cap) for n caller rays,
 * run by the persistent queue tracer on the BVH of the last rt_build_bvh.
 *   rays  n x 8 floats: origin xyz, (unused), direction xyz, (unused)
 *   hits  n x 4 floats: t (RayMax on a miss), triangle index as int32 bits (-1 on a miss), u, v
 *   iters optional n x uint32: TraverseBvh loop iterations per ray
 *   kernel_ms optional: HIP-event time of the tracer kernel alone
 * n must not exceed width x strip rows x spp (the queue capacity).  Host buffers; synchronous. */
int rt_trace_rays(rt_context* ctx, const float* rays, uint32_t n, float* hits, uint32_t* iters, float* kernel_ms);

/* Device ray queries (no reference counterpart): the same traversal for rays and results that live
 * in caller-owned device memory, stream-ordered like rt_update_vertices_device.  For hosts that keep
 * their data on the stream given to rt_set_stream: visibility, line of sight, picking, collision,
 * ray-cast sensors against the geometry they just animated, between pipelined frames.
 *
 * Records: flags 0 gives the closest hit, equal to rt_trace_rays' record (and iteration count) for
 * the same ray bit for bit.  RT_QUERY_ANY_HIT ends each ray at the iteration in which the traversal
 * first records a hit, and the record is that hit: same hit / miss answer as the closest-hit query,
 * t >= the closest t, fewer iterations.  There is no tmin / tmax: every ray starts at t = RayMax (a
 * shorter initial t changes which pushes the traversal's 16-entry stack drops, and with them the
 * record, so it would be another traversal than the reference's).  n is not limited by the queue
 * capacity, only by RT_QUERY_MAX_RAYS.  n == 0 is RT_OK and enqueues nothing but done_event.
 *
 * Ordering: asynchronous, the host is never synchronised; no stream is drained, what a synchronous
 * draw traced ahead is kept, and the path tracer's workspace, RT_ARR_PT_QUEUE and rt_get_ray_count
 * are left as they were.  The kernel runs on the context stream (rt_set_stream), after ready_event
 * if one is given (a hipEvent_t; NULL: the inputs are read after everything enqueued on the context
 * stream so far).  It traces the BVH of the last rt_build_bvh, explicit or inside a draw, enqueued
 * before the call, waits for that build wherever it ran, and holds that LBVH set against every
 * later build that would overwrite it.  The results are visible to work enqueued on the context
 * stream after the call and to whatever waits for done_event (a hipEvent_t the call records behind
 * the kernel, or NULL).  All buffers must stay valid, and the inputs unchanged, until then.
 *
 * RT_ERR_ARG: NULL ctx or q (checked first); then, before the init state: a stride below 3,
 * n > RT_QUERY_MAX_RAYS, unknown flag bits, and with n > 0 a NULL org, dir or hits, hits not 16-byte
 * aligned, org, dir or iters not 4-byte aligned.  RT_ERR_STATE before rt_init; RT_ERR_HIP for a
 * failed launch.  Like the setters it never returns RT_ERR_DEVICE. */
#define RT_QUERY_ANY_HIT 1u            /* stop each ray at the first hit the traversal accepts */
#define RT_QUERY_MAX_RAYS (1u << 30)   /* keeps the kernel's fetch arithmetic inside 32 bits */
typedef struct rt_ray_query {
    const float* org;  uint32_t org_stride;   /* device; stride in floats, >= 3 (3: packed xyz, 8: rt_trace_rays' layout) */
    const float* dir;  uint32_t dir_stride;   /* device; same rules; need not be normalised (as rt_trace_rays) */
    uint32_t n;
    float* hits;        /* device, 16-B aligned, n x 4: t (RayMax on a miss), triangle index as int32 bits (-1), u, v */
    uint32_t* iters;    /* device, optional: TraverseBvh iterations per ray */
    uint32_t flags;     /* 0 or RT_QUERY_ANY_HIT */
    void* ready_event;  /* hipEvent_t or NULL, as in rt_update_vertices_device */
    void* done_event;   /* hipEvent_t or NULL: recorded on the context stream behind the kernel */
} rt_ray_query;
int rt_trace_rays_device(rt_context* ctx, const rt_ray_query* q);

/* Surface queries (no reference counterpart): a device ray query that also answers what its hits hit,
 * for collision response (the normal), semantic sensors (the material id), secondary rays (the
 * re-projected hit point and the reference's ray offset) and Doppler / optical-flow sensors (how the
 * hit point moved since the last build).  The tracer of rt_trace_rays_device runs on q->rays and
 * writes the same records to rays.hits; behind it on the context stream a dense pass writes one
 * surface record per ray, RT_SURFACE_FLOATS(flags) floats, as 16-byte quads:
 *
 *   quad  .x .y .z                                                     .w
 *   0     pos: the hit point re-projected onto the triangle            offset: the reference's ray offset
 *         (miss: RayMax x 3)                                            (errorT + errorP; miss: 1e-7f)
 *   1     normal: geometric, facing the ray (miss: 0, -1, 0)           normalDotRayDir after the flip (miss: -0.0f)
 *   2     fakeNormal: the interpolated vertex normal, flipped to       uint32 bits: 0..15 the material id the path
 *         the geometric one's side (miss: 0, -1, 0)                    tracer reads for the triangle, 16 front face
 *                                                                      (isRayIntoSurface), 17 hit; a miss: 0
 *   3     RT_SURFACE_MOTION only: the hit point's displacement since   0
 *         the build before, d3 (1 - u - v) + d1 u + d2 v of the
 *         corners' (rt_set_geometry_motion; zeros when the build
 *         recorded none, or geometry motion is off, and on a miss)
 *
 * The rule is RaySceneIntersect's tail (traverse.cuh:192-217) on the record's (t, triangle, u, v): the
 * renderer's finalize_hit, the function its path tracer shades with, so the values are the reference's
 * bit for bit (errorT = gamma(16) |t|, as RayTriangleWatertight leaves it).  The material id is
 * materialsIdx[triangle] as the path tracer reads it at the call: [render] materialOverride if set, the
 * table of rt_set_triangle_materials(_device) current at the call, 3 without one.  A secondary ray
 * starts at pos + offset * normal (pos - offset * normal to go through the surface), not at
 * org + t * dir, which hits the triangle it left.  A record whose triangle index is not one of the
 * traced build's, -1 included, is finished as a miss and reads nothing.  Not provided: tmin / tmax (as
 * for the ray query), UV coordinates or other vertex attributes, a host-buffer variant.
 *
 * RT_SURFACE_FROM_HITS: no traversal; rays.hits is read, the records of an earlier query on the same
 * rays and the same build (the caller's responsibility: the pass reads the build current at this call).
 *
 * Ordering: everything rt_trace_rays_device documents.  The host is never synchronised, no stream is
 * drained, what a synchronous draw traced ahead is kept, the path tracer's workspace, RT_ARR_PT_QUEUE,
 * rt_get_ray_count and the pending geometry motion of the next frame are left as they were.
 * rays.ready_event is waited for ahead of the tracer, rays.done_event is recorded behind the surface
 * pass, and the LBVH set and the material table are held until that pass has read them: a later build
 * or rt_set_triangle_materials_device waits on the device.  n == 0 is RT_OK and enqueues nothing but
 * done_event.
 *
 * RT_ERR_ARG: NULL ctx or q (checked first); then, before the init state: every argument error of
 * rt_trace_rays_device on q->rays, unknown bits in flags, with n > 0 a NULL or not 16-byte aligned
 * surface, and with RT_SURFACE_FROM_HITS a rays.iters that is not NULL or RT_QUERY_ANY_HIT in
 * rays.flags.  RT_ERR_STATE before rt_init; RT_ERR_HIP for a failed launch.  It never returns
 * RT_ERR_DEVICE. */
#define RT_SURFACE_FROM_HITS 1u  /* rays.hits is input: no traversal, only the surface pass */
#define RT_SURFACE_MOTION    2u  /* four quads per ray instead of three */
#define RT_SURFACE_FLOATS(flags) (((flags) & RT_SURFACE_MOTION) ? 16u : 12u)
typedef struct rt_surface_query {
    rt_ray_query rays;   /* as rt_trace_rays_device; rays.flags may hold RT_QUERY_ANY_HIT */
    float* surface;      /* device, 16-B aligned, n x RT_SURFACE_FLOATS(flags) floats */
    uint32_t flags;
} rt_surface_query;
int rt_trace_surfaces_device(rt_context* ctx, const rt_surface_query* q);

/* Closest-point queries (no reference counterpart): for points in caller-owned device memory, the
 * nearest triangle of the current build and the nearest point on it, for sphere and capsule colliders,
 * penetration depth, distance-field sampling, foot and hand placement on skinned meshes and proximity
 * sensors: the proximity question no ray answers.  A best-first descent of the two-level LBVH by box
 * distance (csrc/closest_points.hip), not a variant of the ray traversal.
 *
 * The rule (csrc/closest_kernels.h is the definition, compiled for host and device alike): plain fp32,
 * one rounding per operation, nothing fused.  The closest point of triangle (v1, v2, v3) to p by
 * Ericson's Voronoi-region walk in its branch order: vertex 1, vertex 2, edge 12, vertex 3, edge 31,
 * edge 23, face.  With ab = v2 - v1, ac = v3 - v1, dot(a, b) = (ax bx + ay by) + az bz, d1 = dot(ab, p - v1),
 * d2 = dot(ac, p - v1), d3 = dot(ab, p - v2), d4 = dot(ac, p - v2), d5 = dot(ab, p - v3), d6 = dot(ac, p - v3),
 * vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, the weights (wa, wb, wc) of (v1, v2, v3) are
 *   d1 <= 0 and d2 <= 0                           vertex 1   (1, 0, 0)
 *   d3 >= 0 and d4 <= d3                          vertex 2   (0, 1, 0)
 *   vc <= 0, d1 >= 0, d3 <= 0                     edge 12    t = d1 / (d1 - d3): (1 - t, t, 0)
 *   d6 >= 0 and d5 <= d6                          vertex 3   (0, 0, 1)
 *   vb <= 0, d2 >= 0, d6 <= 0                     edge 31    t = d2 / (d2 - d6): (1 - t, 0, t)
 *   va <= 0, d4 - d3 >= 0, d5 - d6 >= 0           edge 23    t = (d4 - d3) / ((d4 - d3) + (d5 - d6)): (0, 1 - t, t)
 *   otherwise                                     face       r = 1 / ((va + vb) + vc); wb = vb r clamped to
 *                                                            [0, 1]; wc = vc r clamped to [0, 1 - wb];
 *                                                            wa = (1 - wb) - wc
 * (the clamps change nothing while va, vb, vc > 0; they keep the point on the triangle when a sliver's
 * rounding reaches the face otherwise, and let a NaN through).  The point is, per component,
 * c = (v1 wa + v2 wb) + v3 wc; d = p - c; d2 = (dx dx + dy dy) + dz dz; u = wa, v = wb: the hit records'
 * barycentrics, so a per-vertex quantity is q1 u + q2 v + q3 (1 - u - v) as for a surface record.  The
 * front bit is dot(n, p - v1) > 0 with n = (aby acz - abz acy, abz acx - abx acz, abx acy - aby acx).  A
 * triangle whose d2 is a NaN is no candidate: one with a vertex that is not finite, or one of zero area
 * that reaches the face's 1 / 0.
 *
 * The answer: the candidates are the triangles that are leaves of the build's tree (what a ray can hit:
 * per 1024-triangle batch the first `count` entries of RT_ARR_REORDER) with an index below the build's
 * triangle count.  The up to three padding triangles that sort into the last batch are no candidates,
 * and the real triangles they displace from the tree are absent, as they are for rays.  (A last batch
 * of one leaf stores its first triangle as that leaf whatever sorted first; the list is the definition,
 * so that triangle is a candidate only when the list names it.)  The answer is
 * the candidate with the lexicographically smallest (d2, triangle index) among those with
 * d2 <= max_distance * max_distance (the product in fp32; +inf stays +inf).  It does not depend on the
 * traversal: rt_closest_points_host over those triangles gives the same bits.  A point with a coordinate
 * that is not finite, no candidate, or none within max_distance gives the miss record.
 *
 * The record, RT_CLOSEST_FLOATS floats per point, as two 16-byte quads:
 *   quad  .x .y .z                                              .w
 *   0     the closest point (miss: RayMax x 3)                   d2 (miss: +inf)
 *   1     triangle index as int32 bits (miss: -1), u, v          uint32 bits: 0..2 the feature (0 face, 1 2 3
 *         (miss: 0, 0)                                           vertex 1 2 3, 4 edge 12, 5 edge 23, 6 edge 31),
 *                                                                16 front, 17 found; a miss: 0
 *
 * Ordering: everything rt_trace_rays_device documents.  The kernel runs on the context stream behind
 * ready_event, on the build current at the call, whose LBVH set it holds against later builds; the host
 * is never synchronised, no stream is drained, what a synchronous draw traced ahead is kept, and the
 * path tracer's workspace, RT_ARR_PT_QUEUE and rt_get_ray_count are left as they were.  n == 0 is
 * RT_OK and enqueues nothing but done_event.  A context that never calls it allocates and launches
 * nothing for it.
 *
 * RT_ERR_ARG: NULL ctx or q (checked first); then, before the init state: a stride below 3,
 * n > RT_QUERY_MAX_RAYS, a max_distance that is negative or a NaN, and with n > 0 a NULL points or out,
 * points not 4-byte or out not 16-byte aligned.  RT_ERR_STATE before rt_init (and before the first
 * build); RT_ERR_HIP for a failed launch.  It never returns RT_ERR_DEVICE.
 *
 * The distance is unsigned, and the front bit is its sign only where the feature is the face: a
 * signed distance is rt_signed_distance_device's (below).  Not provided: per-point radii (one max_distance per
 * call), the k nearest triangles, a host-buffer variant of the device query.
 *
 * [debug] closestStack = N (2..32, default 32) lowers the per-point stack of the descent.  A push onto a
 * full stack makes that point's answer come from a scan of the build's leaf list instead: the same
 * answer, slowly; trees deeper than the stack (chains of equal Morton keys) take that path too. */
#define RT_CLOSEST_FLOATS 8u
#define RT_CLOSEST_FRONT (1u << 16)
#define RT_CLOSEST_FOUND (1u << 17)
typedef struct rt_closest_query {
    const float* points; uint32_t stride;  /* device; stride in floats, >= 3; 4-byte aligned */
    uint32_t n;                            /* <= RT_QUERY_MAX_RAYS; 0 is RT_OK, only done_event */
    float max_distance;                    /* >= 0 or +inf; NaN or negative: RT_ERR_ARG */
    float* out;                            /* device, 16-byte aligned, n x 8 floats */
    void* ready_event; void* done_event;   /* as rt_ray_query */
} rt_closest_query;
int rt_closest_points_device(rt_context* ctx, const rt_closest_query* q);
/* The rule and the definition on the host: no context, no device.  rt_point_triangle: the record of p
 * against the one triangle xyz (v1, v2, v3), with index 0.  rt_closest_points_host: exhaustive; the rule
 * for every triangle of tris (ntri x 9 floats) and every point (n x 3), triangle t under the index ids[t]
 * (NULL: t; 0xFFFFFFFF is RT_ERR_ARG), the lower index winning a tie; out is n x 8 floats.  RT_ERR_ARG:
 * a NULL array that is read or written, a negative or NaN max_distance. */
int rt_point_triangle(const float p[3], const float xyz[9], float out8[8]);
int rt_closest_points_host(const float* tris, const uint32_t* ids, uint32_t ntri, const float* points, uint32_t n,
                           float max_distance, float* out);

/* Signed distance queries (no reference counterpart): the closest-point query with "inside or outside",
 * for penetration depth, distance-field sampling and inside tests against closed meshes that are
 * animated, skinned or streamed, without a host wait.  The closest record's front bit is the sign only
 * where the nearest feature is a face; at an edge or a vertex the lowest-index triangle wins the tie and
 * the point may lie behind its plane while outside the solid.  The sign here comes from angle-weighted
 * pseudo-normals (Baerentzen and Aanaes 2005): the sign of dot(N, p - c) with N the pseudo-normal of the
 * nearest feature is the inside / outside answer of a closed, consistently wound, welded mesh.
 *
 * The rule (csrc/sdf_kernels.h is the definition, compiled for host and device alike): plain fp32, one
 * rounding per operation, nothing fused, dot(a, b) = (ax bx + ay by) + az bz.
 *   unit normal of (v1, v2, v3): n = ab x ac as the closest rule's front bit computes it;
 *     l2 = dot(n, n); if l2 > 0 is false or l2 is not finite the triangle is degenerate: it contributes
 *     nothing anywhere and its own unit normal is (0, 0, 0); otherwise n / sqrtf(l2) per component.
 *   corner angle: rt_acosf(clamp(dot(ea, eb) / sqrtf(dot(ea, ea) dot(eb, eb)), -1, 1)); a NaN stays a NaN,
 *     and such a corner contributes nothing to its vertex.  Corner 1: ea = v2 - v1, eb = v3 - v1;
 *     corner 2: v3 - v2, v1 - v2; corner 3: v1 - v3, v2 - v3.
 *   vertex pseudo-normal of vertex id a: acc = +0; over the slots of a in rt_mesh_adjacency's order
 *     (ascending corner index c, t' = c / 3), skipping t' >= triCount, degenerate triangles and NaN angles:
 *     acc = acc + angle * unit(t') per component, the product rounded first.
 *   edge pseudo-normal of the edge (a, b): the same walk over the slots of a; for a counted t' that
 *     carries b at another of its corners, acc = acc + unit(t').  The walk meets the triangles in ascending
 *     index from either end, so the triangles that share an edge hold the same bits for it.  A boundary
 *     edge gets its own triangle's unit normal, an edge of three or more triangles the sum of them all.
 * The table of a build holds, per triangle t < triCount, six float4 (.w = 0) in the order of the closest
 * record's feature codes 1..6: vertex 1, 2, 3, edge 12 (a = i1, b = i2), edge 23 (i2, i3), edge 31
 * (i3, i1).  All triangles below triCount contribute, whether or not padding displaced them from the
 * tree; the padding triangles have all indices 0, are degenerate and drop out.  Positions are the
 * vertices the build gathered.  Vertex identity is the index: a mesh that repeats positions under
 * several indices (unwelded) or winds neighbours inconsistently gets per-index pseudo-normals that mean
 * little.  Welding is the caller's job.
 *
 * The sign record, one 16-byte quad per point, from the point p and its closest record: N is the table
 * entry of (triangle, feature), for the face (feature 0) the triangle's unit normal from the set's
 * triangle record; d = p - c per component, c the record's closest point; s = dot(N, d);
 *   .xyz = N (not normalised; all zero: no incident triangle counted)
 *   .w   = sqrtf(d2), negated when s < 0 (a zero or NaN s reads as outside); d2 is the record's
 * A miss record gives (0, 0, 0, +inf).
 *
 * rt_set_signed_distance(ctx, on) is a host-style setter like rt_set_emitter_sampling: it waits for the
 * streams, drops what a synchronous draw built or traced ahead, and takes effect from the next LBVH
 * build.  The first enable allocates 96 B per triangle of the capacity (the table) and 72 B per padded
 * triangle (the table build's scratch) on each LBVH set that exists; sets created later get theirs when
 * they are created.  While on, every build writes its set's table behind it on the build's stream
 * (csrc/sdf.hip: a triangle pass into the vertex -> corner adjacency's slots and a gather pass; no float
 * atomics), so frames in flight and held query sets keep the table of their build, and a later vertex
 * update or mesh set is ordered behind the read.  rt_download(RT_ARR_PSEUDO_NORMALS) reads the table of
 * the last build.  RT_ERR_ARG: NULL ctx (or NULL on); RT_ERR_STATE: before rt_init.
 *
 * rt_signed_distance_device runs rt_closest_points_device's descent unchanged, which writes the closest
 * records to closest.out, and behind it on the context stream a dense sign pass (one lane per point)
 * that writes the quads to signed_out.  With RT_DISTANCE_FROM_RECORDS nothing descends: closest.out is
 * read as the records of an earlier query on the same points and the same build (that it is the same
 * build is the caller's responsibility); a record whose triangle index is not below the build's triangle
 * count, -1 included, or whose feature code is past 6, is finished as a miss.  Ordering is the closest
 * query's: closest.ready_event is waited for ahead of the descent, closest.done_event is recorded behind
 * the sign pass, the LBVH set is held until the pass has read it, and the host is never synchronised.
 *
 * Errors, in this order: RT_ERR_ARG for a NULL ctx or q; RT_ERR_ARG for every argument error of
 * rt_closest_points_device on q->closest, unknown flag bits, and with n > 0 a NULL or not 16-byte aligned
 * signed_out; RT_ERR_STATE before rt_init, or when the current build wrote no table (the feature is off,
 * or it was enabled after that build), n == 0 included; RT_ERR_HIP for a failed launch.  Never
 * RT_ERR_DEVICE.  With a table, n == 0 is RT_OK and enqueues nothing but done_event.
 *
 * Not provided: per-point radii, the k nearest triangles, a host-buffer variant of the device query, a
 * generalised winding number for open or unoriented meshes (there the sign follows the nearest
 * feature's pseudo-normal, which means what the winding does). */
int rt_set_signed_distance(rt_context* ctx, int on);
int rt_get_signed_distance(const rt_context* ctx, int* on);
#define RT_DISTANCE_FROM_RECORDS 1u   /* closest.out is input: no descent, only the sign pass */
typedef struct rt_distance_query {
    rt_closest_query closest;  /* as rt_closest_points_device; its records are written to closest.out */
    float* signed_out;         /* device, 16-B aligned, n x 4 floats */
    uint32_t flags;
} rt_distance_query;
int rt_signed_distance_device(rt_context* ctx, const rt_distance_query* q);
/* The rule on the host: no context, no device.  rt_pseudo_normals: the table of a mesh (xyz:
 * vertex_count x 3, indices: triangle_count x 3) into out (triangle_count x 24 floats), with the adjacency
 * of rt_mesh_adjacency over the given triangles; RT_ERR_ARG for a NULL pointer, a zero count or an index
 * >= vertex_count.  rt_signed_distance_rule: the sign record of p from its closest record rec8, the named
 * triangle's positions xyz9 (v1, v2, v3) and its six table entries pn24; a miss record (the found bit
 * clear, index -1 or a feature code past 6) gives (0, 0, 0, +inf); RT_ERR_ARG for a NULL pointer. */
int rt_pseudo_normals(const float* xyz, uint32_t vertex_count, const uint32_t* indices, uint32_t triangle_count,
                      float* out /* triangle_count x 24 */);
int rt_signed_distance_rule(const float p[3], const float rec8[8], const float xyz9[9], const float pn24[24],
                            float out4[4]);
size_t rt_array_bytes(const rt_context* ctx, int what);

#ifdef __cplusplus
}
#endif

#endif /* RTX_AMD_H */
