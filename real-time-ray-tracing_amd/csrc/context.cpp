// context.cpp — RayTracer lifecycle, scene setup and hot-path stage dispatch behind the C-ABI.
//
//   rt_create  <- RayTracer::RayTracer + LoadConfig   (kernel.cuh:435-441, configLoader.cpp:5-27)
//   rt_init    <- RayTracer::init                    (init.cu:53-410)
//   rt_destroy <- RayTracer::cleanup                 (init.cu:601-663)
//   rt_build_bvh / rt_trace_primary <- BuildBvhLevel1/2 (bvh.cu:7-97) / PathTrace's first hit
#include "context.h"

#include <dlfcn.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <fstream>
#include <sstream>

#include "emitter_kernels.h"
#include "gaussian_tables.h"
#include "mat_kernels.h"
#include "rtmath.h"
#include "skin_kernels.h"
#include "toml_lite.h"

namespace {

thread_local std::string g_createError;

void default_params(rt_params& p) {
    // settingParams.h defaults
    p.sky.needRegenerate = 1;
    p.sky.timeOfDay = 0.25f;
    p.sky.sunAxisAngle = 45.0f;
    p.sky.skyScalar = 0.01f;
    p.sky.sunScalar = 0.01f;
    p.sky.sunAngle = 0.6f;
    p.sample.sampleSurfaceVsLightUseMisWeight = 1;
    p.sample.sampleSkyVsSunUseFluxWeight = 1;
    p.sample.sampleSurfaceVsLight = 0.5f;
    p.sample.sampleSkyVsSun = 0.5f;
    p.pass.enableTemporalDenoising = 1;
    p.pass.enableLocalSpatialFilter = 1;
    p.pass.enableNoiseLevelVisualize = 0;
    p.pass.enableWideSpatialFilter = 1;
    p.pass.enableTemporalDenoising2 = 1;
    p.pass.enablePostProcess = 1;
    p.pass.enableDownScalePasses = 1;
    p.pass.enableHistogram = 1;
    p.pass.enableAutoExposure = 1;
    p.pass.enableBloomEffect = 0;
    p.pass.enableLensFlare = 0;
    p.pass.enableToneMapping = 1;
    p.pass.enableSharpening = 1;
    p.post.toneMappingType = 3;
    p.post.exposure = 1.0f;
    p.post.gain = 40.0f;
    p.post.maxWhite = 7.0f;
    p.post.gamma = 2.2f;
    p.denoise.local_denoise_sigma_normal = 100.0f;
    p.denoise.local_denoise_sigma_depth = 0.1f;
    p.denoise.local_denoise_sigma_material = 100.0f;
    p.denoise.large_denoise_sigma_normal = 100.0f;
    p.denoise.large_denoise_sigma_depth = 0.01f;
    p.denoise.large_denoise_sigma_material = 100.0f;
    p.denoise.temporal_denoise_sigma_normal = 100.0f;
    p.denoise.temporal_denoise_sigma_depth = 0.1f;
    p.denoise.temporal_denoise_sigma_material = 100.0f;
    p.denoise.noise_threshold_local = 0.001f;
    p.denoise.noise_threshold_large = 0.001f;
}

bool read_file(const std::string& path, std::string& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::stringstream ss;
    ss << f.rdbuf();
    out = ss.str();
    return true;
}

// meshProcessor .bin (u32 count + Triangle[count], 128 B each: init.cu:28-50,
// tool/meshProcessor.cpp:204-209) -> unshared vertex/index buffers
bool load_triangle_bin(const std::string& path, rtscene::SceneMesh& m, std::string& err) {
    std::string blob;
    if (!read_file(path, blob) || blob.size() < 4) { err = "cannot read mesh file " + path; return false; }
    uint32_t n = 0;
    memcpy(&n, blob.data(), 4);
    // exactly u32 count + count Triangle records of 128 B: the reference reads count * 128 bytes
    // into an uninitialised buffer without checking the read (init.cu:33-43), so a short file
    // (e.g. resources/models/test.bin: 32,768 records of 64 B, the older 4-vertex Triangle) would
    // render uninitialised memory there; it is refused here
    if (n < 2 || blob.size() < 4 + (size_t)n * 128) {
        err = "malformed mesh file " + path + " (" + std::to_string(blob.size()) + " bytes for " + std::to_string(n) +
              " triangles of 128 B)";
        return false;
    }
    m.vertices.resize((size_t)n * 9);
    m.indices.resize((size_t)n * 3);
    for (uint32_t t = 0; t < n; ++t) {
        const char* rec = blob.data() + 4 + (size_t)t * 128;
        for (int k = 0; k < 3; ++k) {
            memcpy(&m.vertices[((size_t)t * 3 + k) * 3], rec + 16 * k, 12);  // v1 w1 v2 w2 v3 w3
            m.indices[(size_t)t * 3 + k] = t * 3 + k;
        }
    }
    m.triCount = n;
    m.triCountPadded = (n + 3u) & ~3u;
    m.indices.resize((size_t)m.triCountPadded * 3, 0u);
    m.cornerCount = n * 3;
    return true;
}

}  // namespace

namespace {
constexpr size_t kArenaChunk = 256ull << 20, kArenaMaxBuffer = 64ull << 20, kArenaAlign = 2ull << 20;
int raw_alloc(rt_context* ctx, void** p, size_t bytes) {
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
        ctx->err = std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e);
        return RT_ERR_HIP;
    }
    ctx->allocations.push_back(q);
    *p = q;
    return RT_OK;
}
}  // namespace

// A renderer stream.  The frame pipeline needs its streams to run concurrently, but HIP maps
// ordinary streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4) shared round-robin with every
// stream created before in the process — a framework's stream pool, say.  Measured: after torch
// had created its pools, rt_draw_device(RT_DRAW_ASYNC) ran 1.42 ms/frame instead of 1.10, two of
// its streams having landed on one queue.  A stream created with a CU mask gets a hardware queue
// of its own, so the renderer's streams use a full mask; they then carry no priority, which
// measured no difference.  [tuning] streams = "prio": plain streams with priorities.
// hipExtStreamCreateWithCUMask makes blocking streams (hipStreamDefault): work on the null stream
// (a framework's default-stream kernels, synchronous hipMemcpy / hipMemset) and the renderer's
// streams wait for each other.  The renderer itself issues synchronous copies only outside
// frames (rt_init, rt_bind_buffer, host reads, the ray-counter reset); a host that keeps default-
// stream work in flight beside pipelined frames should set [tuning] streams = "prio" (non-blocking
// streams).
int rt_create_stream(rt_context* ctx, hipStream_t* s, bool high) {
    if (!ctx->tune.prioStreams) {
        uint32_t mask[32];  // 1024 CUs' worth of bits; bits past the device's CU count are ignored
        for (uint32_t& m : mask) m = 0xFFFFFFFFu;
        HIP_TRY(ctx, hipExtStreamCreateWithCUMask(s, 32, mask));
        return RT_OK;
    }
    int least = 0, greatest = 0;
    HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(ctx, hipStreamCreateWithPriority(s, hipStreamNonBlocking, high ? greatest : least));
    return RT_OK;
}

// Device buffers of a context.  Buffers up to 64 MiB (the BVH, triangles, textures, sky tables,
// G-buffers, counters) are carved from 256-MiB chunks, each buffer starting on a 2-MiB boundary,
// so the data a frame reads lies in a few large, contiguous allocations rather than in dozens of
// separate ones wherever a fragmented device heap puts them; the large, sparsely
// used queue planes get allocations of their own.
int rt_dalloc_bytes(rt_context* ctx, void** p, size_t bytes) {
    if (bytes < 16) bytes = 16;
    if (!ctx->tune.arena || bytes > kArenaMaxBuffer) return raw_alloc(ctx, p, bytes);
    size_t at = (ctx->arenaUsed + kArenaAlign - 1) / kArenaAlign * kArenaAlign;
    if (!ctx->arenaPtr || at + bytes > ctx->arenaCap) {
        void* chunk = nullptr;
        const int rc = raw_alloc(ctx, &chunk, kArenaChunk);
        if (rc != RT_OK) return rc;
        ctx->arenaPtr = (char*)chunk;
        ctx->arenaCap = kArenaChunk;
        at = 0;
    }
    *p = ctx->arenaPtr + at;
    ctx->arenaUsed = at + bytes;
    return RT_OK;
}

std::string rt_data_dir() {
    Dl_info info;
    if (dladdr((void*)&rt_data_dir, &info) && info.dli_fname) {
        std::string so = info.dli_fname;
        size_t s = so.rfind('/');
        std::string dir = s == std::string::npos ? std::string(".") : so.substr(0, s);
        return dir + "/../data";
    }
    return "real-time-ray-tracing_amd/data";
}

// Camera::update (kernel.cuh:103-121), evaluated with the deterministic rtmath functions
void rt_camera_update(const rt_camera& in, int renderW, int renderH, HostCamera& c) {
    memcpy(c.pos, in.pos, sizeof(c.pos));
    c.yaw = in.yaw;
    c.pitch = in.pitch;
    c.focal = in.focal;
    c.aperture = in.aperture;
    c.res[0] = (float)renderW;
    c.res[1] = (float)renderH;
    c.fov[0] = in.fovX;
    const float sy = rt_sinf(c.yaw), cy = rt_cosf(c.yaw), sp = rt_sinf(c.pitch), cp = rt_cosf(c.pitch);
    float dir[3] = {sy * cp, sp, cy * cp};
    c.invRes[0] = 1.0f / c.res[0];
    c.invRes[1] = 1.0f / c.res[1];
    c.fov[1] = c.fov[0] / c.res[0] * c.res[1];
    c.tanHalfFov[0] = rt_tanf(c.fov[0] / 2);
    c.tanHalfFov[1] = rt_tanf(c.fov[1] / 2);
    auto dopf = [](float a, float b, float cc, float d) {
        float cd = cc * d;
        float e = fmaf(-cc, d, cd);
        float dp = fmaf(a, b, -cd);
        return dp + e;
    };
    auto crossf = [&](const float* a, const float* b, float* r) {
        r[0] = dopf(a[1], b[2], a[2], b[1]);
        r[1] = dopf(a[2], b[0], a[0], b[2]);
        r[2] = dopf(a[0], b[1], a[1], b[0]);
    };
    auto normf = [](float* v) {
        float n = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        v[0] = v[0] / n; v[1] = v[1] / n; v[2] = v[2] / n;
    };
    float up0[3] = {0.0f, 1.0f, 0.0f}, left[3], up[3];
    crossf(up0, dir, left);
    normf(left);
    crossf(dir, left, up);
    normf(up);
    for (int k = 0; k < 3; ++k) {
        c.dir[k] = dir[k];
        c.left[k] = left[k];
        c.up[k] = up[k];
        c.adjustedFront[k] = dir[k] * c.focal;
        c.adjustedLeft[k] = left[k] * c.tanHalfFov[0] * c.focal;
        c.adjustedUp[k] = up[k] * c.tanHalfFov[1] * c.focal;
        c.apertureLeft[k] = left[k] * c.aperture;
        c.apertureUp[k] = up[k] * c.aperture;
    }
}

TraceCamera rt_trace_camera(const HostCamera& c) {
    TraceCamera t;
    memcpy(t.pos, c.pos, 12);
    memcpy(t.adjustedFront, c.adjustedFront, 12);
    memcpy(t.adjustedLeft, c.adjustedLeft, 12);
    memcpy(t.adjustedUp, c.adjustedUp, 12);
    memcpy(t.apertureLeft, c.apertureLeft, 12);
    memcpy(t.apertureUp, c.apertureUp, 12);
    memcpy(t.invRes, c.invRes, 8);
    return t;
}

// An LBVH set takes the current mesh's counts, and its arena the layout the build kernel's traversal
// words assume for that batch count (traverse.h): TLAS nodes at B * 1024, triangle records behind
// them.  The allocation is the capacity's, which holds the layout of every mesh within it.
static void arena_place(rt_context* ctx, BvhBufs& b) {
    b.meshSerial = ctx->meshSerial;
    b.triCount = ctx->mesh.triCount;
    b.triCountPadded = ctx->mesh.triCountPadded;
    b.B = ctx->B;
    b.tlasNodes = (char*)b.nodes + (size_t)b.B * 1024 * 64;
    b.triPos = (float4*)((char*)b.nodes + ((size_t)b.B * 1024 + b.B) * 64);
}

// An event of the context: created where first needed, without timing unless asked for, and destroyed
// by rt_destroy
int rt_event(rt_context* ctx, hipEvent_t& e, bool timing) {
    if (e) return RT_OK;
    HIP_TRY(ctx, hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming));
    ctx->events.push_back(e);
    return RT_OK;
}

// The buffers of one LBVH set, by the capacity (rt_set_mesh), which without the config keys is the init
// mesh: the record arena (traverse.h: BLAS nodes, TLAS nodes, triangle records, 64 B each) cleared and
// laid out for the current mesh, the build's scratch and its zeroed launch counter.  The displacement,
// emitter-list and pseudo-normal buffers are their features' (ensure_geometry_motion,
// ensure_emitter_lists, ensure_sdf_tables).
int alloc_bvh_set(rt_context* ctx, BvhBufs& b) {
    if (b.counter) return RT_OK;  // allocated last: the set is complete
    const size_t NP = ctx->capNP, B = ctx->capB;
    RT_TRY(dalloc_once(ctx, b.nodes, arena_bytes(B, NP)));
    RT_TRY(dalloc_once(ctx, b.triNrm, NP * 48));
    RT_TRY(dalloc_once(ctx, b.aabbs, NP * 24));
    RT_TRY(dalloc_once(ctx, b.batchScene, B * 24));
    RT_TRY(dalloc_once(ctx, b.morton, B * 4096));
    RT_TRY(dalloc_once(ctx, b.reorder, B * 4096));
    RT_TRY(dalloc_once(ctx, b.tlasAabbs, B * 24));
    RT_TRY(dalloc_once(ctx, b.tlasScene, 24));
    RT_TRY(dalloc_once(ctx, b.tlasMorton, 4096));
    RT_TRY(dalloc_once(ctx, b.tlasReorder, 4096));
    HIP_TRY(ctx, hipMemset(b.nodes, 0, arena_bytes(B, NP)));
    arena_place(ctx, b);
    uint32_t* counter = nullptr;
    RT_TRY(dalloc(ctx, &counter, 64));
    HIP_TRY(ctx, hipMemset(counter, 0, 64));
    b.counter = counter;
    return RT_OK;
}

extern "C" {

const char* rt_last_error(const rt_context* ctx) { return ctx ? ctx->err.c_str() : g_createError.c_str(); }

int rt_scene_noise3d(const float* xyz, size_t n, float* out) {
    if (n > 0 && (!xyz || !out)) return RT_ERR_ARG;
    for (size_t k = 0; k < n; ++k) out[k] = rtscene::noise3d(xyz[3 * k], xyz[3 * k + 1], xyz[3 * k + 2]);
    return RT_OK;
}

int rt_filter_kernel(int size, float* out, int count) {
    static const float g3[9] = RT_GAUSS3_INIT, g5[25] = RT_GAUSS5_INIT, g7[49] = RT_GAUSS7_INIT;
    const float* g = size == 3 ? g3 : size == 5 ? g5 : size == 7 ? g7 : nullptr;
    if (!g || !out || count < size * size) return RT_ERR_ARG;
    memcpy(out, g, sizeof(float) * size * size);
    return RT_OK;
}

int rt_scan_device(const float* in, float* out, float* tmp, int size, int block_size, int postfix, void* stream) {
    if (!in || !out || size <= 0) {
        g_createError = "rt_scan_device: null buffer or empty size";
        return RT_ERR_ARG;
    }
    const hipError_t e = rtk_launch_scan_ex(in, out, tmp, size, block_size, postfix ? 1 : 0, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) {
        g_createError = "rt_scan_device: size / block_size must be powers of two with block_size and the block "
                        "count <= 8192, and tmp non-null when there is more than one block";
        return RT_ERR_ARG;
    }
    if (e != hipSuccess) {
        g_createError = std::string("rt_scan_device: ") + hipGetErrorString(e);
        return RT_ERR_HIP;
    }
    return RT_OK;
}

int rt_create(int screen_width, int screen_height, const char* config_toml, rt_context** out) {
    if (!out) return RT_ERR_ARG;
    *out = nullptr;
    rt_context* ctx = new rt_context();
    default_params(ctx->params);
    // CameraSetup defaults (init.cu:412-439)
    ctx->camera.pos[0] = -2.0f; ctx->camera.pos[1] = 2.0f; ctx->camera.pos[2] = -2.0f;
    ctx->camera.yaw = 0.0f; ctx->camera.pitch = 0.0f;
    ctx->camera.focal = 5.0f; ctx->camera.aperture = 0.001f;
    ctx->camera.fovX = 90.0f * 0.01745329251f;
    rttoml::Doc doc;
    if (config_toml && config_toml[0]) {
        std::string text, err;
        if (!read_file(config_toml, text)) { g_createError = std::string("cannot read config ") + config_toml; delete ctx; return RT_ERR_IO; }
        if (!rttoml::parse(text, doc, err)) { g_createError = "config parse error: " + err; delete ctx; return RT_ERR_IO; }
    }
    // LoadConfig (configLoader.cpp:15-26); the screen size passed in wins, as in main.cu:260
    int w = rttoml::find_or_int(doc, "resolution", "width", 1920);
    int h = rttoml::find_or_int(doc, "resolution", "height", 1080);
    ctx->screenW = screen_width > 0 ? screen_width : w;
    ctx->screenH = screen_height > 0 ? screen_height : h;
    ctx->inputMeshFileName = rttoml::find_or_string(doc, "file", "inputMeshFileName", "");
    ctx->inputTextureFileNames = rttoml::find_or_strings(doc, "file", "inputTextureFileNames");
    ctx->inputCameraFileName = rttoml::find_or_string(doc, "file", "inputCameraFileName", "");
    ctx->cameraSaveFileName = rttoml::find_or_string(doc, "file", "cameraSaveFileName", "");
    ctx->loadCameraAtInit = rttoml::find_or_bool(doc, "file", "loadCameraAtInit", false);
    ctx->useDynamicResolution = rttoml::find_or_bool(doc, "optimziation", "useDynamicResolution", true);
    ctx->targetFps = rttoml::find_or_float(doc, "optimziation", "targetFps", 60.0f);
    ctx->maxWidth = rttoml::find_or_int(doc, "optimziation", "maxWidth", 3840);
    ctx->maxHeight = rttoml::find_or_int(doc, "optimziation", "maxHeight", 2160);
    ctx->minWidth = rttoml::find_or_int(doc, "optimziation", "minWidth", 640);
    ctx->minHeight = rttoml::find_or_int(doc, "optimziation", "minHeight", 480);
    ctx->chunkDim = rttoml::find_or_int(doc, "scene", "chunkDim", 1);
    ctx->meshFile = rttoml::find_or_string(doc, "scene", "meshFile", "");
    for (const char* key : {"maxTriangles", "maxVertices"}) {  // rt_set_mesh's capacity: a count, 0 = the init mesh's
        const rttoml::Value* v = rttoml::find(doc, "scene", key);
        if (!v) continue;
        char* end = nullptr;
        const long long n = v->isArray || v->isString || v->raw.empty() ? -1 : strtoll(v->raw.c_str(), &end, 10);
        if (n < 0 || n > 0xFFFFFFFFll || !end || *end != '\0') {
            g_createError = std::string("config parse error: [scene] ") + key + " must be a count";
            delete ctx;
            return RT_ERR_IO;
        }
        (key[3] == 'T' ? ctx->maxTriangles : ctx->maxVertices) = (uint32_t)n;
    }
    if (const rttoml::Value* v = rttoml::find(doc, "scene", "textureSets")) {  // a count, 0 = 1; the limit is rt_init's
        char* end = nullptr;
        const long long n = v->isArray || v->isString || v->raw.empty() ? -1 : strtoll(v->raw.c_str(), &end, 10);
        if (n < 0 || n > 0x7FFFFFFFll || !end || *end != '\0') {
            g_createError = "config parse error: [scene] textureSets must be a count";
            delete ctx;
            return RT_ERR_IO;
        }
        ctx->textureSets = (int)n;
    }
    if (const rttoml::Value* v = rttoml::find(doc, "scene", "skySets")) {  // a count, 0 = 1; the limit is rt_init's
        char* end = nullptr;
        const long long n = v->isArray || v->isString || v->raw.empty() ? -1 : strtoll(v->raw.c_str(), &end, 10);
        if (n < 0 || n > 0x7FFFFFFFll || !end || *end != '\0') {
            g_createError = "config parse error: [scene] skySets must be a count";
            delete ctx;
            return RT_ERR_IO;
        }
        ctx->skySetsCfg = (int)n;
    }
    ctx->spp = rttoml::find_or_int(doc, "render", "spp", 1);
    ctx->bvhThreads = rttoml::find_or_int(doc, "render", "bvhThreads", 0);  // LBVH workgroup shape (A/B, tests)
    ctx->device = rttoml::find_or_int(doc, "render", "device", -1);
    ctx->stripY0 = rttoml::find_or_int(doc, "render", "stripY0", 0);
    ctx->stripRows = rttoml::find_or_int(doc, "render", "stripRows", -1);
    ctx->stripCount = rttoml::find_or_int(doc, "render", "stripCount", 1);
    ctx->stripIndex = rttoml::find_or_int(doc, "render", "stripIndex", 0);
    ctx->materialOverride = rttoml::find_or_int(doc, "render", "materialOverride", -1);
    if (const rttoml::Value* v = rttoml::find(doc, "render", "geometryMotion")) {
        if (v->isArray || v->isString || (v->raw != "true" && v->raw != "false")) {
            g_createError = "config parse error: [render] geometryMotion must be true or false";
            delete ctx;
            return RT_ERR_IO;
        }
        ctx->geomMotion = v->raw == "true";
    }
    if (const rttoml::Value* v = rttoml::find(doc, "render", "emitterSampling")) {
        if (v->isArray || v->isString || (v->raw != "true" && v->raw != "false")) {
            g_createError = "config parse error: [render] emitterSampling must be true or false";
            delete ctx;
            return RT_ERR_IO;
        }
        ctx->emitterOn = v->raw == "true";
    }
    if (const rttoml::Value* v = rttoml::find(doc, "render", "signedDistance")) {
        if (v->isArray || v->isString || (v->raw != "true" && v->raw != "false")) {
            g_createError = "config parse error: [render] signedDistance must be true or false";
            delete ctx;
            return RT_ERR_IO;
        }
        ctx->sdfOn = v->raw == "true";
    }
    if (const rttoml::Value* v = rttoml::find(doc, "render", "emitterProbability")) {
        char* end = nullptr;
        const float q = v->isArray || v->isString || v->raw.empty() ? -1.0f : strtof(v->raw.c_str(), &end);
        if (!end || *end != '\0' || !std::isfinite(q) || q < 0.0f || q > 1.0f) {
            g_createError = "config parse error: [render] emitterProbability must be a number in [0, 1]";
            delete ctx;
            return RT_ERR_IO;
        }
        ctx->emitterQ = q;
    }
    ctx->bvhSkipPublish = (uint32_t)rttoml::find_or_int(doc, "debug", "bvhSkipPublish", -1);
    ctx->bvhSkipBuilds = rttoml::find_or_int(doc, "debug", "bvhSkipPublishBuilds", -1);
    ctx->bvhWaitMs = rttoml::find_or_float(doc, "debug", "bvhWaitMs", 1000.0f);
    if (const rttoml::Value* v = rttoml::find(doc, "debug", "closestStack")) {
        char* end = nullptr;
        const long cap = v->isArray || v->isString || v->raw.empty() ? -1 : strtol(v->raw.c_str(), &end, 10);
        if (!end || *end != '\0') {
            g_createError = "config parse error: [debug] closestStack must be an integer";
            delete ctx;
            return RT_ERR_IO;
        }
        if (cap < 2 || cap > 32) {  // kClosestStackMax (frame_kernels.h)
            g_createError = "[debug] closestStack must be 2..32";
            delete ctx;
            return RT_ERR_ARG;
        }
        ctx->closestStack = (int)cap;
    }
    {
        rt_context::Tuning& t = ctx->tune;
        t.arena = rttoml::find_or_bool(doc, "tuning", "arena", true);
        t.prioStreams = rttoml::find_or_string(doc, "tuning", "streams", "cumask") == "prio";
        t.tracePerCu = rttoml::find_or_int(doc, "tuning", "tracePerCu", 0);
        t.trace4PerCu = rttoml::find_or_int(doc, "tuning", "trace4PerCu", 0);
        t.trace3ShortPerCu = rttoml::find_or_int(doc, "tuning", "trace3ShortPerCu", 2);
        const std::string chain = rttoml::find_or_string(doc, "tuning", "chain", "serial");
        t.chain = chain == "off" ? 0 : chain == "always" ? 2 : 1;
        t.shadeOnSide = rttoml::find_or_bool(doc, "tuning", "shadeOnSide", true);
        t.shadeBlocksPerCu = rttoml::find_or_int(doc, "tuning", "shadeBlocksPerCu", 0);
        t.overlapAfter = rttoml::find_or_int(doc, "tuning", "overlapAfter", -1);
        t.cameraAfter = rttoml::find_or_int(doc, "tuning", "cameraAfter", -1);
        t.syncSpec = rttoml::find_or_bool(doc, "tuning", "syncSpec", true);
        t.specChain = rttoml::find_or_int(doc, "tuning", "specChain", -1);
        t.specAfter = rttoml::find_or_int(doc, "tuning", "specAfter", 1);
        t.specShade = rttoml::find_or_int(doc, "tuning", "specShade", 2);
        t.specShadePerCu = rttoml::find_or_int(doc, "tuning", "specShadePerCu", 2);
        t.specTracePerCu = rttoml::find_or_int(doc, "tuning", "specTracePerCu", 2);
        t.dnSplit = rttoml::find_or_int(doc, "tuning", "dnSplit", 0);
        t.dnFold = rttoml::find_or_int(doc, "tuning", "dnFold", 0) != 0;
        t.resumeSplit = rttoml::find_or_int(doc, "tuning", "resumeSplit", t.resumeSplit);
        t.resumeSplit = t.resumeSplit < 0 ? 0 : t.resumeSplit > 2 ? 2 : t.resumeSplit;
    }
    if (ctx->screenW <= 0 || ctx->screenH <= 0 || ctx->screenW > 16384 || ctx->screenH > 16384 || ctx->spp < 1 ||
        ctx->spp > 64 || ctx->chunkDim < 1 || ctx->chunkDim > 8 ||
        (ctx->bvhThreads != 0 && ctx->bvhThreads != 512 && ctx->bvhThreads != 1024)) {
        g_createError = "invalid resolution / spp / chunkDim / bvhThreads";
        delete ctx;
        return RT_ERR_ARG;
    }
    // init.cu:58-67: dynamic resolution renders at the max size
    if (ctx->useDynamicResolution) { ctx->renderW = ctx->maxWidth; ctx->renderH = ctx->maxHeight; }
    else { ctx->renderW = ctx->screenW; ctx->renderH = ctx->screenH; }
    if (ctx->stripCount > 1) {  // interleaved row blocks (row_of): stripY0 / stripRows do not apply
        if (ctx->stripIndex < 0 || ctx->stripIndex >= ctx->stripCount || ctx->stripY0 != 0 || ctx->stripRows >= 0) {
            g_createError = "stripCount > 1 needs 0 <= stripIndex < stripCount and no stripY0 / stripRows";
            delete ctx;
            return RT_ERR_ARG;
        }
        ctx->stripRows = (int)strip_row_count((uint32_t)ctx->renderH, (uint32_t)ctx->stripCount, (uint32_t)ctx->stripIndex);
    }
    if (ctx->stripRows < 0) ctx->stripRows = ctx->renderH - ctx->stripY0;
    ctx->fullFrame = ctx->stripCount == 1 && ctx->stripY0 == 0 && ctx->stripRows == ctx->renderH;
    ctx->histW = ctx->renderW;
    ctx->histH = ctx->renderH;
    ctx->allocW = ctx->renderW;  // the largest frame: dynamic resolution only shrinks from here
    ctx->allocH = ctx->renderH;
    ctx->allocStripRows = ctx->stripRows;
    if (ctx->stripCount < 1 || ctx->stripY0 < 0 || ctx->stripRows < 1 || ctx->stripY0 + ctx->stripRows > ctx->renderH) {
        g_createError = "invalid strip rows";
        delete ctx;
        return RT_ERR_ARG;
    }
    *out = ctx;
    return RT_OK;
}

int rt_init(rt_context* ctx) {
    if (!ctx) return RT_ERR_ARG;
    if (ctx->inited) { ctx->err = "rt_init called twice"; return RT_ERR_STATE; }
    if (ctx->textureSets > RT_TEXTURE_SETS_MAX) {
        ctx->err = "[scene] textureSets out of range: at most " + std::to_string(RT_TEXTURE_SETS_MAX);
        return RT_ERR_ARG;
    }
    ctx->texSets = ctx->textureSets > 0 ? (uint32_t)ctx->textureSets : 1u;
    if (ctx->skySetsCfg > RT_SKY_SETS_MAX) {
        ctx->err = "[scene] skySets out of range: at most " + std::to_string(RT_SKY_SETS_MAX);
        return RT_ERR_ARG;
    }
    ctx->skySets = ctx->skySetsCfg > 0 ? ctx->skySetsCfg : 1;
    // ---- scene (init.cu:78-130), built and checked on the host before any device call, so a bad
    // input is reported as such on any machine
    std::string err;
    const std::string dataDir = rt_data_dir();
    if (!ctx->meshFile.empty()) {
        if (!load_triangle_bin(ctx->meshFile, ctx->mesh, err)) { ctx->err = err; return RT_ERR_IO; }
    } else {
        std::vector<std::vector<float>> tiles;
        if (!rtscene::load_tiles(dataDir + "/roundcubes_l2.bin", tiles, err) ||
            !rtscene::generate(ctx->chunkDim, tiles, ctx->mesh, err)) {
            ctx->err = err;
            return RT_ERR_IO;
        }
    }
    const uint32_t N = ctx->mesh.triCount, NP = ctx->mesh.triCountPadded;
    // MIN_TRIANGLE_COUNT_ALLOWED 2 / MAX_TRIANGLE_COUNT_ALLOWED 1024 * 1024 (kernel.cuh:54-55), which
    // init.cu:89-90 asserts; the reference's LBVH needs two triangles for a BLAS (buildBVH.cuh:30)
    if (N < 2 || N > 1024u * 1024u) { ctx->err = "triangle count out of range [2, 1048576] (kernel.cuh:54-55)"; return RT_ERR_ARG; }
    ctx->B = (N + 1023) / 1024;
    if (ctx->B >= 1024) { ctx->err = "batch count must stay below 1024 (init.cu:126)"; return RT_ERR_ARG; }
    ctx->nv = (uint32_t)(ctx->mesh.vertices.size() / 3);
    // rt_set_mesh's capacity ([scene] maxTriangles / maxVertices; 0: this mesh), under the same limits
    ctx->capTri = ctx->maxTriangles ? ctx->maxTriangles : N;
    ctx->capNV = ctx->maxVertices ? ctx->maxVertices : ctx->nv;
    if (ctx->capTri < N || ctx->capNV < ctx->nv) { ctx->err = "[scene] maxTriangles / maxVertices below the init mesh"; return RT_ERR_ARG; }
    if (ctx->capTri > 1024u * 1024u || (ctx->capTri + 1023) / 1024 >= 1024) {
        ctx->err = "[scene] maxTriangles out of range: at most 1048576 triangles in fewer than 1024 batches";
        return RT_ERR_ARG;
    }
    ctx->capNP = (ctx->capTri + 3u) & ~3u;
    ctx->capB = (ctx->capTri + 1023) / 1024;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { ctx->err = "no HIP device visible"; return RT_ERR_NO_DEVICE; }
    if (ctx->device >= 0) HIP_TRY(ctx, hipSetDevice(ctx->device));
    int dev = 0;
    HIP_TRY(ctx, hipGetDevice(&dev));
    ctx->device = dev;
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        ctx->err = std::string("librtx is built for gfx950, device is ") + prop.gcnArchName;
        return RT_ERR_NO_DEVICE;
    }
    ctx->cuCount = prop.multiProcessorCount;
    int wallKhz = 0;
    if (hipDeviceGetAttribute(&wallKhz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && wallKhz > 0)
        ctx->wallTicksPerMs = (uint64_t)wallKhz;
    HIP_TRY(ctx, hipHostMalloc((void**)&ctx->status, 64, hipHostMallocDefault));
    memset(ctx->status, 0, 64);

    // the context stream (the trace chain, a frame's critical path); with [tuning] streams = "prio" it is
    // created at the highest priority and the side / internal post streams at the lowest, otherwise
    // all are CU-masked streams without priority (rt_create_stream)
    if (int rc = rt_create_stream(ctx, &ctx->ownStream, true)) return rc;
    ctx->stream = ctx->ownStream;
    RT_TRY(rt_event(ctx, ctx->ev0, true));
    RT_TRY(rt_event(ctx, ctx->ev1, true));

    // every mesh-sized buffer by the capacity (rt_set_mesh), which without the config keys is this mesh
    const size_t capNV = ctx->capNV, capNP = ctx->capNP;
    RT_TRY(dalloc_once(ctx, ctx->dVerts, capNV * 12));
    RT_TRY(dalloc_once(ctx, ctx->dNormals, capNV * 12));
    RT_TRY(dalloc_once(ctx, ctx->dIdx, capNP * 12));
    RT_TRY(alloc_bvh_set(ctx, ctx->bvh[0]));
    RT_TRY(dalloc_once(ctx, ctx->dBlueNoise, 327680));
    const size_t P = (size_t)ctx->renderW * ctx->renderH;
    RT_TRY(dalloc_once(ctx, ctx->dHits, P * 16));
    RT_TRY(dalloc_once(ctx, ctx->dHitNrm, P * 16));
    RT_TRY(dalloc_once(ctx, ctx->dHitFake, P * 16));
    RT_TRY(dalloc_once(ctx, ctx->dHitStats, P * 16));

    HIP_TRY(ctx, hipMemcpy(ctx->dVerts, ctx->mesh.vertices.data(), (size_t)ctx->nv * 12, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->dIdx, ctx->mesh.indices.data(), (size_t)NP * 12, hipMemcpyHostToDevice));

    std::string bn;
    if (!read_file(dataDir + "/bluenoise_4spp.bin", bn) || bn.size() != 327680) {
        ctx->err = "cannot read " + dataDir + "/bluenoise_4spp.bin";
        return RT_ERR_IO;
    }
    HIP_TRY(ctx, hipMemcpy(ctx->dBlueNoise, bn.data(), bn.size(), hipMemcpyHostToDevice));

    // ---- frame-1 smooth normals (kernel.cu:313-327): vertex -> corner CSR in triangle order
    std::vector<uint32_t> slots((size_t)NP * 3);  // the CSR's inverse, corner -> slot (vertex updates)
    {
        std::vector<uint32_t> off(ctx->nv + 1, 0), corners((size_t)NP * 3);
        if (rt_mesh_adjacency(ctx->mesh.indices.data(), NP, ctx->nv, off.data(), corners.data(), slots.data()) != RT_OK) {
            ctx->err = "the mesh has an index past its vertices";
            return RT_ERR_ARG;
        }
        RT_TRY(dalloc_once(ctx, ctx->dAdjOff, (capNV + 1) * 4));
        RT_TRY(dalloc_once(ctx, ctx->dAdjCorner, capNP * 12));
        HIP_TRY(ctx, hipMemcpy(ctx->dAdjOff, off.data(), off.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(ctx->dAdjCorner, corners.data(), corners.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(ctx, rtk_launch_smooth_normals(ctx->dVerts, ctx->dAdjOff, ctx->dAdjCorner, ctx->dIdx, ctx->nv,
                                               ctx->dNormals, ctx->stream));
    }
    RT_TRY(rt_frame_init(ctx));
    // vertex updates (rt_update_vertices*, geometry.hip): their scratch and events exist from here on,
    // so that an update only enqueues work
    RT_TRY(dalloc_once(ctx, ctx->dCornerSlot, capNP * 12));
    RT_TRY(dalloc_once(ctx, ctx->dContrib, capNP * 36));
    HIP_TRY(ctx, hipMemcpy(ctx->dCornerSlot, slots.data(), slots.size() * 4, hipMemcpyHostToDevice));
    RT_TRY(rt_event(ctx, ctx->geomSrc));
    RT_TRY(rt_event(ctx, ctx->geomDone));
    // device ray queries (rt_trace_rays_device): their fetch counters and events, so that a query only enqueues work
    RT_TRY(dalloc_once(ctx, ctx->queryFetch, 512));
    for (BvhBufs& b : ctx->bvh) RT_TRY(rt_event(ctx, b.queryDone));
    if (ctx->geomMotion) RT_TRY(ensure_geometry_motion(ctx));  // [render] geometryMotion
    if (ctx->emitterOn) RT_TRY(ensure_emitter_lists(ctx));     // [render] emitterSampling
    if (ctx->sdfOn) RT_TRY(ensure_sdf_tables(ctx));            // [render] signedDistance
    // mesh sets (rt_set_mesh*, mesh.hip): the staging buffers of the host variants and the adjacency
    // sort's scratch, behind every other buffer of rt_init, so that a set only enqueues work
    RT_TRY(dalloc_once(ctx, ctx->dVertStage, capNV * 12));
    RT_TRY(dalloc_once(ctx, ctx->dIdxStage, capNP * 12));
    for (int k = 0; k < 2; ++k) {
        RT_TRY(dalloc_once(ctx, ctx->dSortKeys[k], capNP * 12));
        RT_TRY(dalloc_once(ctx, ctx->dSortVals[k], capNP * 12));
    }
    RT_TRY(dalloc_once(ctx, ctx->dSortTable, ((size_t)256 * kMeshTilesMax + 256) * 4));
    RT_TRY(dalloc_once(ctx, ctx->dMeshBad, 64));
    HIP_TRY(ctx, hipMemset(ctx->dMeshBad, 0, 64));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->mesh.vertices = std::vector<float>();   // the device holds the mesh from here on
    ctx->mesh.indices = std::vector<uint32_t>();
    ctx->inited = true;
    // CameraSetup (init.cu:433-435): a missing or short file leaves the default camera, and the
    // reference only prints its error, so this is not an rt_init failure either
    if (ctx->loadCameraAtInit && rt_load_camera(ctx, ctx->inputCameraFileName.c_str()) != RT_OK)
        fprintf(stderr, "librtx: %s (default camera kept)\n", ctx->err.c_str());
    return RT_OK;
}

void rt_destroy(rt_context* ctx) {
    if (!ctx) return;
    if (ctx->inited) (void)sync_streams(ctx, false);  // also when the context stream is the null stream
    for (hipEvent_t e : ctx->events) (void)hipEventDestroy(e);
    if (ctx->sideStream) (void)hipStreamDestroy(ctx->sideStream);
    if (ctx->leanStream) (void)hipStreamDestroy(ctx->leanStream);
    if (ctx->ownPostStream) (void)hipStreamDestroy(ctx->ownPostStream);
    for (void* p : ctx->allocations) (void)hipFree(p);
    if (ctx->envStage) (void)hipFree(ctx->envStage);  // rt_set_environment's staging, regrown outside the list
    if (ctx->fr.q3Host) (void)hipHostFree(ctx->fr.q3Host);
    if (ctx->status) (void)hipHostFree(ctx->status);
    if (ctx->ownStream) {
        (void)hipStreamSynchronize(ctx->ownStream);
        (void)hipStreamDestroy(ctx->ownStream);
    }
    delete ctx;
}

int rt_get_params(const rt_context* ctx, rt_params* out) {
    if (!ctx || !out) return RT_ERR_ARG;
    *out = ctx->params;
    return RT_OK;
}

int rt_set_params(rt_context* ctx, const rt_params* in) {
    if (!ctx || !in) return RT_ERR_ARG;
    ctx->params = *in;
    return RT_OK;
}

int rt_get_camera(const rt_context* ctx, rt_camera* out) {
    if (!ctx || !out) return RT_ERR_ARG;
    *out = ctx->camera;
    return RT_OK;
}

int rt_set_camera(rt_context* ctx, const rt_camera* in) {
    if (!ctx || !in) return RT_ERR_ARG;
    ctx->camera = *in;
    return RT_OK;
}

int rt_set_frame_index(rt_context* ctx, int frame_num) {
    if (!ctx || frame_num < 1) return RT_ERR_ARG;
    ctx->nextFrame = frame_num;
    return RT_OK;
}

int rt_set_delta_time(rt_context* ctx, float ms) {
    if (!ctx) return RT_ERR_ARG;
    ctx->deltaMs = ms;
    return RT_OK;
}

int rt_get_info(const rt_context* ctx, rt_info* out) {
    if (!ctx || !out) return RT_ERR_ARG;
    out->triCount = ctx->mesh.triCount;
    out->triCountPadded = ctx->mesh.triCountPadded;
    out->batchCount = ctx->B;
    out->vertexCount = ctx->nv;
    out->renderWidth = ctx->renderW;
    out->renderHeight = ctx->renderH;
    out->screenWidth = ctx->screenW;
    out->screenHeight = ctx->screenH;
    out->frameNum = ctx->lastFrame;
    out->deviceId = ctx->device;
    out->spp = (uint32_t)ctx->spp;
    out->gbufferSet = ctx->fr.gbSet;
    uint32_t a = 0, b = (uint32_t)ctx->renderH;
    if (ctx->stripCount > 1) denoise_rows((uint32_t)ctx->renderH, (uint32_t)ctx->stripCount, (uint32_t)ctx->stripIndex, a, b);
    out->denoiseRowBegin = (int32_t)a;
    out->denoiseRowEnd = (int32_t)b;
    uint32_t sa = 0, sb = 0, lo = 0, hi = (uint32_t)ctx->renderH;
    out->stripLocalDenoise = 0;
    out->shadeOnSide = ctx->postStream && ctx->shadeOnSide ? 1 : 0;
    out->lastChain = ctx->fr.lastChain ? 1 : 0;
    if (ctx->inited && strip_local_denoise(ctx, sa, sb)) {
        gbuffer_rows((uint32_t)ctx->renderH, sa, sb, lo, hi);
        out->stripLocalDenoise = 1;
    }
    out->gbufferRowBegin = (int32_t)lo;
    out->gbufferRowEnd = (int32_t)hi;
    return RT_OK;
}

// The explicit build (BuildBvhLevel1/2), which a draw issues too: into the current set on the context
// stream, or with frame pipelining into the other set on the side stream, behind that set's last readers.
int rt_build_bvh(rt_context* ctx) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_build_bvh before rt_init"; return RT_ERR_STATE; }
    if (int rc = check_device_status(ctx)) return rc;  // a previous build's failure, once it is known
    ctx->bvhPrebuilt = false;  // an explicit build supersedes a synchronous draw's prebuild
    if (!ctx->postStream) return build_bvh(ctx, ctx->bvhSet, ctx->stream);
    const int k = ctx->bvhSet ^ 1;
    if (ctx->bvh[k].readInFlight) HIP_TRY(ctx, hipStreamWaitEvent(ctx->sideStream, ctx->bvh[k].readDone, 0));
    ctx->bvhSet = k;
    return build_bvh(ctx, k, ctx->sideStream);
}

}  // extern "C"

// The LBVH of the current geometry into bvh[set] on `stream`, with what follows a build on its stream:
// the displacement records, the emitter list and, off the context stream, the set's buildDone.
int build_bvh(rt_context* ctx, int set, hipStream_t stream) {
    BvhBufs& b = ctx->bvh[set];
    // camera rays a synchronous draw traced ahead read this set (frame.cpp launch_spec_camera): the
    // rebuild overwrites it only after them.  It writes the same values while the geometry epoch is
    // theirs; after a vertex update it does not, and the next path trace drops them (spec_matches)
    if (ctx->fr.spec.valid) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->specDone, 0));
    if (!ctx->postStream) b.buildOnSide = false;
    // the build gathers the vertices and normals of the last update, whichever stream that ran on
    if (ctx->geomDoneValid && stream != ctx->geomStream) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->geomDone, 0));
    // the set's first build on another mesh (rt_set_mesh): its counts and arena layout, over a cleared arena,
    // so that what the build does not write reads zero as in a context initialised with this mesh
    if (b.meshSerial != ctx->meshSerial) {
        arena_place(ctx, b);
        HIP_TRY(ctx, hipMemsetAsync(b.nodes, 0, arena_bytes(ctx->capB, ctx->capNP), stream));
    }
    BvhBuildParams p;
    p.vertices = ctx->dVerts;
    p.normals = ctx->dNormals;
    p.indices = ctx->dIdx;
    p.triCount = ctx->mesh.triCount;
    p.triCountPadded = ctx->mesh.triCountPadded;
    p.batchCount = ctx->B;
    p.triPos = b.triPos;
    p.triNrm = b.triNrm;
    p.aabbs = b.aabbs;
    p.batchSceneAabbs = b.batchScene;
    p.morton = b.morton;
    p.reorder = b.reorder;
    p.nodes = b.nodes;
    p.tlasAabbs = b.tlasAabbs;
    p.tlasSceneAabb = b.tlasScene;
    p.tlasMorton = b.tlasMorton;
    p.tlasReorder = b.tlasReorder;
    p.tlasNodes = b.tlasNodes;
    p.counter = b.counter;
    p.threads = (uint32_t)ctx->bvhThreads;
    p.cus = (uint32_t)ctx->cuCount;
    p.status = ctx->status;
    p.waitTicks = (uint64_t)((double)ctx->bvhWaitMs * (double)ctx->wallTicksPerMs);
    p.skipPublish = ctx->bvhSkipBuilds != 0 ? ctx->bvhSkipPublish : 0xFFFFFFFFu;
    if (ctx->bvhSkipBuilds > 0) --ctx->bvhSkipBuilds;
    p.buildSeq = ++ctx->buildSeq;
    HIP_TRY(ctx, rtk_launch_build_bvh(&p, stream));
    // geometry motion vectors: a build at another epoch than the previous build's records the
    // vertices' step between the two, right behind the build and ahead of buildDone, so that the
    // next update (which overwrites dVerts / dPrevVerts) is behind this read as it is behind the
    // gather.  The first build, a build at the previous one's epoch and a build whose predecessor's
    // positions were not kept (the feature was off) record none.
    b.dispValid = false;
    if (ctx->geomMotion && ctx->built && ctx->geomEpoch != ctx->builtEpoch && ctx->prevVertsValid &&
        ctx->prevVertsEpoch == ctx->builtEpoch) {
        GeomDispParams d;
        d.vertices = ctx->dVerts;
        d.prevVerts = ctx->dPrevVerts;
        d.indices = ctx->dIdx;
        d.triDisp = b.triDisp;
        d.triCountPadded = b.triCountPadded;
        HIP_TRY(ctx, rtk_launch_geometry_displacement(&d, stream));
        b.dispValid = true;
        b.dispTraced = false;
    }
    ctx->built = true;
    ctx->builtEpoch = ctx->geomEpoch;
    // emitter sampling: the set's emitter list from the records this build has just written, behind it on
    // its stream and ahead of buildDone, so whatever traces the set reads the list of its build.  The
    // material table is written in place behind a wait for every stream; the triangle ids may come from a
    // device set on another stream (matDone), and a later device set into the buffer read here waits for
    // listRead as it waits for the path traces that read it.
    b.emBuilt = false;
    if (emitter_active(ctx) && b.emHeader && ctx->mesh.triCount <= kEmMaxTris) {
        const bool ids = ctx->materialOverride < 0 && ctx->dTriMat;
        if (ids && ctx->matDevice && ctx->matDone) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->matDone, 0));
        EmitterListParams e;
        e.triPos = b.triPos;
        e.triMat = ids ? ctx->dTriMat : nullptr;
        e.matTable = reinterpret_cast<const float4*>(ctx->dMatTable);
        e.materialOverride = ctx->materialOverride;
        e.triCount = ctx->mesh.triCount;
        e.cdfLen = emitter_cdf_len(ctx->mesh.triCount);
        e.triWeight = b.emTriWeight;
        e.blockCount = b.emBlockCount;
        e.tris = b.emTris;
        e.weights = b.emWeights;
        e.cdf = b.emCdf;
        e.scanSums = b.emScanSums;
        e.header = b.emHeader;
        HIP_TRY(ctx, rtk_launch_emitter_list(&e, stream));
        if (ids && ctx->matPoolReady) {
            rt_context::MatTable& tab = ctx->matPool[ctx->matCur];
            HIP_TRY(ctx, hipEventRecord(tab.listRead, stream));
            tab.listValid = true;
        }
        b.emBuilt = true;
        b.emCdfLen = e.cdfLen;
    }
    // signed distance queries: the set's pseudo-normal table from the vertices this build has just gathered,
    // behind it on its stream and ahead of buildDone.  The vertices, indices and adjacency are read where
    // the build's gather and the displacement kernel read them, so a later vertex update or mesh set is
    // behind this read as it is behind theirs, and whatever queries the set reads the table of its build.
    b.sdfBuilt = false;
    if (ctx->sdfOn && b.sdfSlotOthers && ctx->mesh.triCount > 0u) {
        SdfTableParams t;
        t.vertices = ctx->dVerts;
        t.indices = ctx->dIdx;
        t.cornerSlot = ctx->dCornerSlot;
        t.adjOffsets = ctx->dAdjOff;
        t.nverts = ctx->nv;
        t.triCount = ctx->mesh.triCount;
        t.triCountPadded = ctx->mesh.triCountPadded;
        t.slotNormal = b.sdfSlotNormal;
        t.slotOthers = b.sdfSlotOthers;
        t.table = b.sdfTable;
        HIP_TRY(ctx, rtk_launch_sdf_table(&t, stream));
        b.sdfBuilt = true;
    }
    if (stream != ctx->stream) {  // the side stream: a pipelined frame's build, a synchronous draw's prebuild
        HIP_TRY(ctx, hipEventRecord(b.buildDone, stream));
        b.buildOnSide = b.sideBuilt = true;
    }
    return RT_OK;
}

extern "C" {

// ---------------------------------------------------------------- animated geometry
//
// One update on stream U: the side stream on a pipelined context (where every build runs, so the
// update is behind the last one and ahead of the next without an event, and beside the current
// frame's trace chain), else the context stream.  `srcReady`: the source needs no ordering (the
// renderer's staging copy); otherwise U waits for `ready`, or without one for the context stream.
//
// A mesh set (rt_set_mesh*) is the same update with `mesh` given: the index ingest and the adjacency
// kernels (mesh.hip) run first on U, behind the same waits, since the builds' gather, the normals
// kernels and the displacement kernel are the only readers of the index and adjacency arrays as they
// are of the vertices; then the whole-mesh update with the new counts.
struct MeshChange {
    const uint32_t* indices;  // device memory, [triCount * 3]
    uint32_t triCount, nverts;
};
static hipStream_t update_stream(const rt_context* ctx) { return ctx->postStream ? ctx->sideStream : ctx->stream; }

// what an update on U waits for: its source, and the builds and the update still using what it writes
static int order_vertex_update(rt_context* ctx, hipStream_t u, hipEvent_t ready, bool srcReady) {
    if (!srcReady) {
        if (ready) {
            HIP_TRY(ctx, hipStreamWaitEvent(u, ready, 0));
        } else if (u != ctx->stream) {
            HIP_TRY(ctx, hipEventRecord(ctx->geomSrc, ctx->stream));
            HIP_TRY(ctx, hipStreamWaitEvent(u, ctx->geomSrc, 0));
        }
    }
    // the builds that still gather the old positions: a synchronous draw's prebuild on the side stream
    // (the context stream's own builds are ahead of the update there), an earlier update elsewhere
    if (u != ctx->sideStream)
        for (const BvhBufs& b : ctx->bvh)
            if (b.sideBuilt) HIP_TRY(ctx, hipStreamWaitEvent(u, b.buildDone, 0));
    if (ctx->geomDoneValid && ctx->geomStream != u) HIP_TRY(ctx, hipStreamWaitEvent(u, ctx->geomDone, 0));
    return RT_OK;
}

// `ordered`: the caller has made U wait already (order_vertex_update) and enqueued the source's producer
// on it (a pose's skinning kernel)
static int enqueue_vertex_update(rt_context* ctx, const float* src, uint32_t first, uint32_t count, hipEvent_t ready,
                                 bool srcReady, bool bump, const MeshChange* mesh = nullptr, bool ordered = false) {
    hipStream_t u = update_stream(ctx);
    if (!ordered)
        if (int rc = order_vertex_update(ctx, u, ready, srcReady)) return rc;
    hipEvent_t* marks = ctx->meshMarks;  // rt_time_mesh_set only
    if (mesh) {
        MeshSetParams m;
        m.srcIndices = mesh->indices;
        m.triCount = mesh->triCount;
        m.triCountPadded = (mesh->triCount + 3u) & ~3u;
        m.nverts = mesh->nverts;
        m.indices = ctx->dIdx;
        m.adjOffsets = ctx->dAdjOff;
        m.adjCorner = ctx->dAdjCorner;
        m.cornerSlot = ctx->dCornerSlot;
        for (int k = 0; k < 2; ++k) {
            m.keys[k] = ctx->dSortKeys[k];
            m.vals[k] = ctx->dSortVals[k];
        }
        m.table = ctx->dSortTable;
        m.badCount = ctx->dMeshBad;
        m.status = ctx->status;
        if (marks) HIP_TRY(ctx, hipEventRecord(marks[0], u));
        HIP_TRY(ctx, rtk_launch_mesh_set(&m, u, marks ? marks[1] : nullptr));
        if (marks) HIP_TRY(ctx, hipEventRecord(marks[2], u));
        if (bump) {  // the context follows the new mesh from here; each LBVH set keeps its build's counts
            ctx->mesh.triCount = m.triCount;
            ctx->mesh.triCountPadded = m.triCountPadded;
            ctx->mesh.cornerCount = m.triCount * 3;
            ctx->B = (m.triCount + 1023) / 1024;
            ctx->nv = m.nverts;
            ++ctx->meshSerial;
            // the material table back to the default, as rt_reset_triangle_materials leaves it but without
            // a wait: launches in flight hold the old table by value, and the store is not written
            ctx->dTriMat = nullptr;
            ctx->triMatClasses = 0;
            ctx->matDevice = false;
            ++ctx->matSerial;
            ctx->prevVertsValid = false;  // geometry motion: the next build is a first build
            ctx->skinSet = false;         // a skin belongs to the vertices it was set for (rt_set_skin)
        }
    }
    GeomUpdateParams p;
    p.src = src;
    p.first = first;
    p.count = count;
    p.vertices = ctx->dVerts;
    p.normals = ctx->dNormals;
    p.indices = ctx->dIdx;
    p.cornerSlot = ctx->dCornerSlot;
    p.adjOffsets = ctx->dAdjOff;
    p.contrib = ctx->dContrib;
    p.nverts = ctx->nv;
    p.triCountPadded = ctx->mesh.triCountPadded;
    // geometry motion vectors: the first update after a build keeps the positions that build gathered
    // (several updates before the next build count as one step); rt_time_stage(5) keeps nothing
    const bool keep = bump && !mesh && ctx->geomMotion && ctx->built && ctx->geomEpoch == ctx->builtEpoch;
    p.prevVerts = keep ? ctx->dPrevVerts : nullptr;
    HIP_TRY(ctx, rtk_launch_geometry_update(&p, u));
    if (mesh && marks) HIP_TRY(ctx, hipEventRecord(marks[3], u));
    if (keep) {
        ctx->prevVertsValid = true;
        ctx->prevVertsEpoch = ctx->geomEpoch;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->geomDone, u));
    ctx->geomStream = u;
    ctx->geomDoneValid = true;
    // what the caller enqueues on the context stream from here on follows the read of its buffer
    if (u != ctx->stream) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->geomDone, 0));
    if (bump) ++ctx->geomEpoch;
    return RT_OK;
}

static int check_vertex_range(rt_context* ctx, const void* xyz, uint32_t first, uint32_t count, const char* who) {
    if (!ctx || !xyz) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = std::string(who) + " before rt_init"; return RT_ERR_STATE; }
    if (count == 0 || (uint64_t)first + (uint64_t)count > (uint64_t)ctx->nv) {
        ctx->err = std::string(who) + ": [first, first + count) must be a non-empty range of the mesh's vertices";
        return RT_ERR_ARG;
    }
    return RT_OK;
}

int rt_update_vertices_device(rt_context* ctx, const float* xyz_device, uint32_t first, uint32_t count,
                              void* ready_event) {
    if (int rc = check_vertex_range(ctx, xyz_device, first, count, "rt_update_vertices_device")) return rc;
    if (((uintptr_t)xyz_device & 3u) != 0) { ctx->err = "rt_update_vertices_device: positions must be 4-byte aligned"; return RT_ERR_ARG; }
    return enqueue_vertex_update(ctx, xyz_device, first, count, (hipEvent_t)ready_event, false, true);
}

// the staging buffer, once no earlier update still reads it
static int vertex_stage(rt_context* ctx) {
    if (ctx->geomDoneValid) HIP_TRY(ctx, hipEventSynchronize(ctx->geomDone));
    return RT_OK;
}

int rt_update_vertices(rt_context* ctx, const float* xyz, uint32_t first, uint32_t count) {
    if (int rc = check_vertex_range(ctx, xyz, first, count, "rt_update_vertices")) return rc;
    if (int rc = vertex_stage(ctx)) return rc;
    float* stage = ctx->dVertStage + 3 * (size_t)first;
    HIP_TRY(ctx, hipMemcpy(stage, xyz, (size_t)count * 12, hipMemcpyHostToDevice));
    return enqueue_vertex_update(ctx, stage, first, count, nullptr, true, true);
}

int rt_get_geometry_epoch(const rt_context* ctx, uint64_t* epoch) {
    if (!ctx || !epoch) return RT_ERR_ARG;
    *epoch = ctx->geomEpoch;
    return RT_OK;
}

// ---------------------------------------------------------------- mesh replacement
//
// Check order: NULL ctx / mesh, the arguments that need no context state, the init state, the capacity.
static int check_mesh(rt_context* ctx, const rt_mesh* m, const char* who) {
    if (!ctx || !m) return RT_ERR_ARG;
    const char* bad = nullptr;
    if (!m->xyz || !m->indices) bad = "xyz and indices must not be NULL";
    else if ((((uintptr_t)m->xyz | (uintptr_t)m->indices) & 3u) != 0) bad = "xyz and indices must be 4-byte aligned";
    else if (m->triangle_count < 2u) bad = "a mesh has at least 2 triangles";
    else if (m->vertex_count == 0u) bad = "a mesh has at least 1 vertex";
    if (bad) { ctx->err = std::string(who) + ": " + bad; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = std::string(who) + " before rt_init"; return RT_ERR_STATE; }
    if (m->triangle_count > ctx->capTri || m->vertex_count > ctx->capNV) {
        ctx->err = std::string(who) + ": " + std::to_string(m->triangle_count) + " triangles / " +
                   std::to_string(m->vertex_count) + " vertices exceed the capacity ([scene] maxTriangles " +
                   std::to_string(ctx->capTri) + " / maxVertices " + std::to_string(ctx->capNV) + ")";
        return RT_ERR_ARG;
    }
    return RT_OK;
}

int rt_set_mesh_device(rt_context* ctx, const rt_mesh* mesh) {
    if (int rc = check_mesh(ctx, mesh, "rt_set_mesh_device")) return rc;
    const MeshChange mc{mesh->indices, mesh->triangle_count, mesh->vertex_count};
    return enqueue_vertex_update(ctx, mesh->xyz, 0, mesh->vertex_count, (hipEvent_t)mesh->ready_event, false, true, &mc);
}

int rt_set_mesh(rt_context* ctx, const rt_mesh* mesh) {
    if (int rc = check_mesh(ctx, mesh, "rt_set_mesh")) return rc;
    const size_t ni = (size_t)mesh->triangle_count * 3;
    for (size_t c = 0; c < ni; ++c)
        if (mesh->indices[c] >= mesh->vertex_count) {
            ctx->err = "rt_set_mesh: index " + std::to_string(mesh->indices[c]) + " of corner " + std::to_string(c) +
                       " is not below vertex_count";
            return RT_ERR_ARG;
        }
    if (int rc = vertex_stage(ctx)) return rc;  // the staging buffers, once no earlier update reads them
    HIP_TRY(ctx, hipMemcpy(ctx->dVertStage, mesh->xyz, (size_t)mesh->vertex_count * 12, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->dIdxStage, mesh->indices, ni * 4, hipMemcpyHostToDevice));
    const MeshChange mc{ctx->dIdxStage, mesh->triangle_count, mesh->vertex_count};
    return enqueue_vertex_update(ctx, ctx->dVertStage, 0, mesh->vertex_count, nullptr, true, true, &mc);
}

// ---------------------------------------------------------------- skinned meshes
//
// Check order of rt_set_skin: NULL ctx / skin, the arguments that need no context state, the init state,
// the vertex count, the arrays' contents.
int rt_set_skin(rt_context* ctx, const rt_skin* skin) {
    if (!ctx || !skin) return RT_ERR_ARG;
    if (const char* bad = skin_shape_fault(skin)) { ctx->err = std::string("rt_set_skin: ") + bad; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = "rt_set_skin before rt_init"; return RT_ERR_STATE; }
    if (skin->vertex_count != ctx->nv) {
        ctx->err = "rt_set_skin: vertex_count " + std::to_string(skin->vertex_count) + " is not the mesh's " +
                   std::to_string(ctx->nv) + ": a skin covers the whole mesh";
        return RT_ERR_ARG;
    }
    uint32_t at = 0;
    if (const char* bad = skin_content_fault(skin, at)) {
        ctx->err = "rt_set_skin: vertex " + std::to_string(at) + ": " + bad;
        return RT_ERR_ARG;
    }
    // a pose in flight reads the arrays; camera rays traced ahead are dropped as by every setter
    if (int rc = sync_streams(ctx, false)) return rc;
    RT_TRY(dalloc_once(ctx, ctx->dSkinRest, (size_t)ctx->capNV * 12));
    RT_TRY(dalloc_once(ctx, ctx->dSkinJoints, (size_t)ctx->capNV * 8));
    RT_TRY(dalloc_once(ctx, ctx->dSkinWeights, (size_t)ctx->capNV * 16));
    RT_TRY(dalloc_once(ctx, ctx->dSkinned, (size_t)ctx->capNV * 12));
    RT_TRY(dalloc_once(ctx, ctx->dSkinMats, (size_t)kSkinJointsMax * kSkinMatrixFloats * 4));
    const size_t nv = skin->vertex_count;
    std::vector<float> ident((size_t)skin->joint_count * kSkinMatrixFloats, 0.0f);
    for (uint32_t j = 0; j < skin->joint_count; ++j)
        ident[(size_t)j * 12] = ident[(size_t)j * 12 + 5] = ident[(size_t)j * 12 + 10] = 1.0f;
    ctx->skinSet = false;  // a failed copy leaves no skin rather than a mixed one
    HIP_TRY(ctx, hipMemcpy(ctx->dSkinRest, skin->rest_xyz, nv * 12, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->dSkinJoints, skin->joints, nv * 8, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->dSkinWeights, skin->weights, nv * 16, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->dSkinMats, ident.data(), ident.size() * 4, hipMemcpyHostToDevice));
    ctx->skinSet = true;
    ctx->skinJoints = skin->joint_count;
    return RT_OK;
}

int rt_reset_skin(rt_context* ctx) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_reset_skin before rt_init"; return RT_ERR_STATE; }
    if (int rc = sync_streams(ctx, false)) return rc;
    ctx->skinSet = false;  // the buffers stay allocated for the next set
    return RT_OK;
}

int rt_get_skin(const rt_context* ctx, uint32_t* vertex_count, uint32_t* joint_count) {
    if (!ctx || !vertex_count || !joint_count) return RT_ERR_ARG;
    *vertex_count = ctx->skinSet ? ctx->nv : 0u;
    *joint_count = ctx->skinSet ? ctx->skinJoints : 0u;
    return RT_OK;
}

// One pose on the update stream: the skinning kernel behind what a vertex update waits for, then the
// whole-mesh update reading its output (`src` null), or for rt_time_stage(8) the given copy of the
// current positions.
static int enqueue_pose(rt_context* ctx, const float* matrices, hipEvent_t ready, bool srcReady, bool bump,
                        const float* src = nullptr) {
    hipStream_t u = update_stream(ctx);
    if (int rc = order_vertex_update(ctx, u, ready, srcReady)) return rc;
    SkinParams p;
    p.rest = ctx->dSkinRest;
    p.joints = ctx->dSkinJoints;
    p.weights = ctx->dSkinWeights;
    p.matrices = matrices;
    p.out = ctx->dSkinned;
    p.nverts = ctx->nv;
    HIP_TRY(ctx, rtk_launch_skin(&p, u));
    return enqueue_vertex_update(ctx, src ? src : ctx->dSkinned, 0, ctx->nv, nullptr, true, bump, nullptr, true);
}

static int check_pose(rt_context* ctx, const rt_pose* pose, bool device, const char* who) {
    if (!ctx || !pose) return RT_ERR_ARG;
    if (!pose->matrices) { ctx->err = std::string(who) + ": matrices must not be NULL"; return RT_ERR_ARG; }
    if (device && ((uintptr_t)pose->matrices & 15u) != 0) { ctx->err = std::string(who) + ": matrices must be 16-byte aligned"; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = std::string(who) + " before rt_init"; return RT_ERR_STATE; }
    if (!ctx->skinSet) { ctx->err = std::string(who) + " without a skin (rt_set_skin; rt_set_mesh drops it)"; return RT_ERR_STATE; }
    if (pose->joint_count != ctx->skinJoints) {
        ctx->err = std::string(who) + ": joint_count " + std::to_string(pose->joint_count) + " is not the skin's " +
                   std::to_string(ctx->skinJoints);
        return RT_ERR_ARG;
    }
    return RT_OK;
}

int rt_pose_skin_device(rt_context* ctx, const rt_pose* pose) {
    if (int rc = check_pose(ctx, pose, true, "rt_pose_skin_device")) return rc;
    return enqueue_pose(ctx, pose->matrices, (hipEvent_t)pose->ready_event, false, true);
}

int rt_pose_skin(rt_context* ctx, const rt_pose* pose) {
    if (int rc = check_pose(ctx, pose, false, "rt_pose_skin")) return rc;
    if (int rc = vertex_stage(ctx)) return rc;  // the matrix staging, once no earlier pose reads it
    HIP_TRY(ctx, hipMemcpy(ctx->dSkinMats, pose->matrices, (size_t)pose->joint_count * kSkinMatrixFloats * 4, hipMemcpyHostToDevice));
    return enqueue_pose(ctx, ctx->dSkinMats, nullptr, true, true);
}

// ---------------------------------------------------------------- geometry motion vectors
//
// The previous-position array and the displacement records of the LBVH sets that exist (the second
// set's are allocated with it, ensure_bvh_pair); once allocated they stay.
int ensure_geometry_motion(rt_context* ctx) {
    if (!ctx->dPrevVerts) {
        if (int rc = dalloc(ctx, &ctx->dPrevVerts, (size_t)ctx->capNV * 12)) return rc;
    }
    for (BvhBufs& b : ctx->bvh)
        if (b.nodes && !b.triDisp) {
            if (int rc = dalloc(ctx, &b.triDisp, (size_t)ctx->capNP * 48)) return rc;
        }
    return RT_OK;
}

int rt_set_geometry_motion(rt_context* ctx, int on) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_set_geometry_motion before rt_init"; return RT_ERR_STATE; }
    int rc = sync_streams(ctx, false);
    if (rc != RT_OK) return rc;
    if (on && (rc = ensure_geometry_motion(ctx)) != RT_OK) return rc;
    if ((on != 0) != ctx->geomMotion) {  // from the next build on: what the sets hold is dropped either way
        ctx->prevVertsValid = false;
        ctx->bvh[0].dispValid = ctx->bvh[1].dispValid = false;
    }
    ctx->geomMotion = on != 0;
    return RT_OK;
}

int rt_get_geometry_motion(const rt_context* ctx, int* on) {
    if (!ctx || !on) return RT_ERR_ARG;
    *on = ctx->geomMotion ? 1 : 0;
    return RT_OK;
}

// ---------------------------------------------------------------- emitter sampling
//
// The list buffers of the LBVH sets that exist (the second set's are allocated with it,
// ensure_bvh_pair), by the triangle capacity: every triangle may be an emitter.  Once allocated they stay.
int ensure_emitter_lists(rt_context* ctx) {
    if (ctx->capTri > kEmMaxTris) return RT_OK;  // such a mesh gets no list (rt_build_bvh); nothing to hold
    const size_t len = emitter_cdf_len(ctx->capTri), blocks = len / 256;
    for (BvhBufs& b : ctx->bvh)
        if (b.nodes && !b.emHeader) {
            int rc;
            if ((rc = dalloc(ctx, &b.emTris, len * 4)) != RT_OK) return rc;
            if ((rc = dalloc(ctx, &b.emWeights, len * 4)) != RT_OK) return rc;
            if ((rc = dalloc(ctx, &b.emCdf, len * 4)) != RT_OK) return rc;
            if ((rc = dalloc(ctx, &b.emTriWeight, len * 4)) != RT_OK) return rc;
            if ((rc = dalloc(ctx, &b.emBlockCount, (blocks + 1) * 4)) != RT_OK) return rc;
            if ((rc = dalloc(ctx, &b.emScanSums, blocks * 4)) != RT_OK) return rc;
            if ((rc = dalloc(ctx, &b.emHeader, kEmHeaderWords * 4)) != RT_OK) return rc;  // last: the set is complete
        }
    return RT_OK;
}

int rt_set_emitter_sampling(rt_context* ctx, int on, float probability) {
    if (!ctx) return RT_ERR_ARG;
    if (!std::isfinite(probability) || probability < 0.0f || probability > 1.0f) {
        ctx->err = "rt_set_emitter_sampling: probability must be finite and lie in [0, 1]";
        return RT_ERR_ARG;
    }
    if (!ctx->inited) { ctx->err = "rt_set_emitter_sampling before rt_init"; return RT_ERR_STATE; }
    // the kernels in flight read the lists, and what a synchronous draw traced ahead precedes the change
    int rc = sync_streams(ctx, false);
    if (rc != RT_OK) return rc;
    if (on && (rc = ensure_emitter_lists(ctx)) != RT_OK) return rc;
    // from the next build on: a synchronous draw's prebuild was made under the old state
    ctx->bvhPrebuilt = false;
    if (!on)
        for (BvhBufs& b : ctx->bvh) b.emBuilt = false;
    ctx->emitterOn = on != 0;
    ctx->emitterQ = probability;
    return RT_OK;
}

int rt_get_emitter_sampling(const rt_context* ctx, int* on, float* probability) {
    if (!ctx || !on || !probability) return RT_ERR_ARG;
    *on = ctx->emitterOn ? 1 : 0;
    *probability = ctx->emitterQ;
    return RT_OK;
}

// ---------------------------------------------------------------- signed distance queries
//
// The pseudo-normal tables of the LBVH sets that exist (the second set's are allocated with it,
// ensure_bvh_pair): 96 B per triangle of the capacity, and the table build's scratch, 24 B per corner of
// the padded capacity.  Once allocated they stay.
int ensure_sdf_tables(rt_context* ctx) {
    for (BvhBufs& b : ctx->bvh)
        if (b.nodes && !b.sdfSlotOthers) {
            int rc;
            if (!b.sdfTable && (rc = dalloc(ctx, &b.sdfTable, (size_t)ctx->capTri * 96)) != RT_OK) return rc;
            if (!b.sdfSlotNormal && (rc = dalloc(ctx, &b.sdfSlotNormal, (size_t)ctx->capNP * 48)) != RT_OK) return rc;
            if ((rc = dalloc(ctx, &b.sdfSlotOthers, (size_t)ctx->capNP * 24)) != RT_OK) return rc;  // last: the set is complete
        }
    return RT_OK;
}

int rt_set_signed_distance(rt_context* ctx, int on) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_set_signed_distance before rt_init"; return RT_ERR_STATE; }
    // what a synchronous draw traced ahead precedes the change
    int rc = sync_streams(ctx, false);
    if (rc != RT_OK) return rc;
    if (on && (rc = ensure_sdf_tables(ctx)) != RT_OK) return rc;
    // from the next build on: a synchronous draw's prebuild was made under the old state
    ctx->bvhPrebuilt = false;
    if (!on)
        for (BvhBufs& b : ctx->bvh) b.sdfBuilt = false;
    ctx->sdfOn = on != 0;
    return RT_OK;
}

int rt_get_signed_distance(const rt_context* ctx, int* on) {
    if (!ctx || !on) return RT_ERR_ARG;
    *on = ctx->sdfOn ? 1 : 0;
    return RT_OK;
}

// the kernels' two rules (emitter_kernels.h), compiled for the host
int rt_emitter_weight(const float xyz[9], const float emission[3], float* weight) {
    if (!xyz || !emission || !weight) return RT_ERR_ARG;
    *weight = emitter_weight(xyz, emission);
    return RT_OK;
}

int rt_emitter_select(const float* cdf, uint32_t count, float r, uint32_t* slot, float* prob) {
    if (!cdf || !slot || !prob || count == 0u) return RT_ERR_ARG;
    float p;
    *slot = emitter_select(cdf, count, r, p);
    *prob = p;
    return RT_OK;
}

// ---------------------------------------------------------------- per-triangle materials
//
// SceneMaterial::materialsIdx (kernel.cuh:198-203, init.cu:261-269): one material id per triangle,
// looked up at every hit (traverse.cuh:29-32; update_material in pathtrace.hip).

// Which ids select which kernel class: mat_type (shade.h) gives mirror to id 5 and glass to id 1, and
// an id past the ten-entry table is the reference's SAFE_LOAD default, mirror; id 4 is the one
// microfacet material.  The one statement of the rule (fill_pt_params calls it too).
int rt_material_classes(const uint8_t* ids, size_t n, uint32_t* classes) {
    if (!classes || (!ids && n)) return RT_ERR_ARG;
    uint32_t c = 0;
    for (size_t k = 0; k < n; ++k) {
        const uint8_t id = ids[k];
        if (id == 1 || id == 5 || id >= 10) c |= RT_MAT_CLASS_GLOSSY;
        else if (id == 4) c |= RT_MAT_CLASS_MICROFACET;
    }
    *classes = c;
    return RT_OK;
}

// the classes of the ids that have a triangle, from the census
static void census_classes(rt_context* ctx) {
    uint8_t present[256];
    size_t n = 0;
    for (int id = 0; id < 256; ++id)
        if (ctx->triMatCount[id]) present[n++] = (uint8_t)id;
    (void)rt_material_classes(present, n, &ctx->triMatClasses);
}

int rt_set_triangle_materials(rt_context* ctx, const uint8_t* ids, uint32_t first, uint32_t count) {
    if (!ctx || !ids) return RT_ERR_ARG;
    if (count == 0) { ctx->err = "rt_set_triangle_materials: count must not be 0"; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = "rt_set_triangle_materials before rt_init"; return RT_ERR_STATE; }
    const uint32_t n = ctx->mesh.triCount;
    if ((uint64_t)first + (uint64_t)count > (uint64_t)n) {
        ctx->err = "rt_set_triangle_materials: [first, first + count) must be a non-empty range of the mesh's triangles";
        return RT_ERR_ARG;
    }
    // the kernels in flight read the table, and camera rays traced ahead precede it (spec_matches)
    if (int rc = sync_streams(ctx, false)) return rc;
    // the current buffer of the pool, in place: nothing reads it now
    rt_context::MatTable& tab = ctx->matPool[ctx->matCur];
    ctx->matBytes = ((size_t)ctx->capNP + 15u) & ~(size_t)15u;
    if (!tab.ids) {
        if (int rc = dalloc(ctx, &tab.ids, ctx->matBytes)) return rc;
    }
    if (!ctx->dTriMat) {  // the first set, or the first after a reset: the reference's table
        HIP_TRY(ctx, hipMemset(tab.ids, 3, ctx->matBytes));
        ctx->triMatHost.assign(n, (uint8_t)3);
        memset(ctx->triMatCount, 0, sizeof ctx->triMatCount);
        ctx->triMatCount[3] = n;
    } else if (ctx->matDevice) {  // a device set's table: the host copy and its census afresh
        ctx->triMatHost.assign(n, (uint8_t)3);
        HIP_TRY(ctx, hipMemcpy(ctx->triMatHost.data(), tab.ids, n, hipMemcpyDeviceToHost));
        memset(ctx->triMatCount, 0, sizeof ctx->triMatCount);
        for (uint32_t k = 0; k < n; ++k) ++ctx->triMatCount[ctx->triMatHost[k]];
    }
    HIP_TRY(ctx, hipMemcpy(tab.ids + first, ids, count, hipMemcpyHostToDevice));
    for (uint32_t k = 0; k < count; ++k) {
        uint8_t& h = ctx->triMatHost[(size_t)first + k];
        --ctx->triMatCount[h];
        h = ids[k];
        ++ctx->triMatCount[h];
    }
    census_classes(ctx);
    ctx->dTriMat = tab.ids;
    ctx->matDevice = false;
    ++ctx->matSerial;
    return RT_OK;
}

int rt_reset_triangle_materials(rt_context* ctx) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_reset_triangle_materials before rt_init"; return RT_ERR_STATE; }
    if (int rc = sync_streams(ctx, false)) return rc;
    ctx->dTriMat = nullptr;  // the null table: the launches of a context that never set one
    ctx->triMatClasses = 0;
    ctx->matDevice = false;
    ++ctx->matSerial;
    return RT_OK;
}

// ---- the stream-ordered set (materials.hip)

uint32_t rt_material_class_rule(uint32_t id) { return mat_class_of(id & 0xFFu); }

// every buffer of the pool with its census, the counter and the events: the first device set
static int ensure_mat_pool(rt_context* ctx) {
    if (ctx->matPoolReady) return RT_OK;
    ctx->matBytes = ((size_t)ctx->capNP + 15u) & ~(size_t)15u;
    size_t missing = 0;
    for (const rt_context::MatTable& t : ctx->matPool) missing += t.ids ? 0u : 1u;
    // one block: the missing tables, then a 1-KiB census per table, then the counter's 64 bytes
    const size_t bytes = missing * ctx->matBytes + (size_t)kMatPool * 1024 + 64;
    uint8_t* block = nullptr;
    if (int rc = dalloc(ctx, &block, bytes)) return rc;
    HIP_TRY(ctx, hipMemset(block, 3, missing * ctx->matBytes));
    HIP_TRY(ctx, hipMemset(block + missing * ctx->matBytes, 0, (size_t)kMatPool * 1024 + 64));
    HIP_TRY(ctx, hipStreamSynchronize(nullptr));  // this first call may block; the fills precede every stream's use
    for (hipEvent_t* e : {&ctx->matSrc, &ctx->matDone}) RT_TRY(rt_event(ctx, *e));
    for (rt_context::MatTable& t : ctx->matPool)
        for (hipEvent_t* e : {&t.read, &t.specRead, &t.listRead}) RT_TRY(rt_event(ctx, *e));
    uint8_t* at = block;
    for (rt_context::MatTable& t : ctx->matPool)
        if (!t.ids) {
            t.ids = at;
            at += ctx->matBytes;
        }
    for (rt_context::MatTable& t : ctx->matPool) {
        t.census = (uint32_t*)at;
        at += 1024;
    }
    ctx->dMatBad = (uint32_t*)at;
    // path traces enqueued so far read the current (host-set) table unmarked: everything on the
    // streams their kernels run on counts as its readers
    rt_context::MatTable& cur = ctx->matPool[ctx->matCur];
    HIP_TRY(ctx, hipEventRecord(cur.read, ctx->stream));
    cur.readValid = true;
    if (ctx->sideStream) {
        HIP_TRY(ctx, hipEventRecord(cur.specRead, ctx->sideStream));
        cur.specValid = true;
    }
    ctx->matPoolReady = true;
    return RT_OK;
}

int rt_set_triangle_materials_device(rt_context* ctx, const rt_material_update* u) {
    if (!ctx || !u) return RT_ERR_ARG;
    const char* bad = nullptr;
    if (!u->ids) bad = "ids must not be NULL";
    else if (u->count == 0) bad = "count must not be 0";
    else if ((u->classes & ~RT_MAT_CLASS_ALL) != 0u) bad = "unknown bits in classes";
    if (bad) { ctx->err = std::string("rt_set_triangle_materials_device: ") + bad; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = "rt_set_triangle_materials_device before rt_init"; return RT_ERR_STATE; }
    if ((uint64_t)u->first + (uint64_t)u->count > (uint64_t)ctx->mesh.triCount) {
        ctx->err = "rt_set_triangle_materials_device: [first, first + count) must be a non-empty range of the mesh's triangles";
        return RT_ERR_ARG;
    }
    if (int rc = ensure_mat_pool(ctx)) return rc;
    // On the stream of the vertex updates: the side stream of a pipelined context, where the next
    // frame's shade kernel follows it without an event and it runs beside the current frame's chain.
    hipStream_t s = ctx->postStream ? ctx->sideStream : ctx->stream;
    const int next = (ctx->matCur + 1) % kMatPool;
    rt_context::MatTable& dst = ctx->matPool[next];
    if (u->ready_event) {
        HIP_TRY(ctx, hipStreamWaitEvent(s, (hipEvent_t)u->ready_event, 0));
    } else if (s != ctx->stream) {
        HIP_TRY(ctx, hipEventRecord(ctx->matSrc, ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->matSrc, 0));
    }
    // the launches that still read the buffer this set writes; the previous table was written on this
    // stream (an earlier device set) or behind a wait for every stream (a host set)
    if (dst.readValid) HIP_TRY(ctx, hipStreamWaitEvent(s, dst.read, 0));
    if (dst.specValid) HIP_TRY(ctx, hipStreamWaitEvent(s, dst.specRead, 0));
    if (dst.listValid) HIP_TRY(ctx, hipStreamWaitEvent(s, dst.listRead, 0));  // an emitter-list build (rt_build_bvh)
    MatSetParams p;
    p.prev = ctx->dTriMat;  // null after rt_set_mesh* and a reset: 3 everywhere
    p.src = u->ids;
    p.dst = dst.ids;
    p.census = dst.census;
    p.badCount = ctx->dMatBad;
    p.status = ctx->status;
    p.first = u->first;
    p.count = u->count;
    p.triCount = ctx->mesh.triCount;
    p.capBytes = (uint32_t)ctx->matBytes;
    // under a custom material table (rt_set_materials) the class of an id follows its entry's type and
    // every frame runs the all-classes kernels: the set records every class, replaces and counts nothing
    const uint32_t classes = ctx->matCustom ? RT_MAT_CLASS_ALL : u->classes;
    p.classes = classes;
    HIP_TRY(ctx, rtk_launch_mat_set(&p, s));
    HIP_TRY(ctx, hipEventRecord(ctx->matDone, s));
    // the caller's later work on the context stream follows the read of its buffer, and so does every
    // later path trace: its kernels run on this stream, on the context stream or behind a fork of it
    if (s != ctx->stream) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->matDone, 0));
    dst.readValid = dst.specValid = dst.listValid = false;
    ctx->matCur = next;
    ctx->dTriMat = dst.ids;
    ctx->triMatClasses = classes;  // the plan of later frames: exactly the declared bits
    ctx->matDevice = true;
    ++ctx->matSerial;
    return RT_OK;
}

// ---------------------------------------------------------------- the material table
//
// What an id means (rt_set_materials).  The host keeps the 256 entries as the caller
// gave them; the device gets one 64-byte record each (MatRecord), written in place behind the wait for
// every stream.

int rt_default_material(uint32_t id, rt_material* out) {
    if (!out || id > 255u) return RT_ERR_ARG;
    rt_material m = {};
    // mat_type (shade.h), restated for the host: 0, 2 emissive; 1 glass; 3, 6..9 Lambertian; 4
    // microfacet; 5 and everything past the ten-entry table mirror
    m.type = (id == 0u || id == 2u) ? RT_MAT_EMISSIVE
             : id == 1u             ? RT_MAT_GLASS
             : id == 4u             ? RT_MAT_MICROFACET
             : (id == 5u || id >= 10u) ? RT_MAT_MIRROR
                                       : RT_MAT_LAMBERTIAN;
    m.flags = 0u;
    for (int k = 0; k < 3; ++k) {
        m.color[k] = 1.0f;
        m.emission[k] = 0.0f;
    }
    m.ior = 1.33f;
    m.alpha = 0.05f;
    m.f0[0] = 0.56f;
    m.f0[1] = 0.57f;
    m.f0[2] = 0.58f;
    *out = m;
    return RT_OK;
}

static const char* material_fault(const rt_material& m) {
    if (m.type < RT_MAT_LAMBERTIAN || m.type > RT_MAT_EMISSIVE) return "type must be one of RT_MAT_*";
    if ((m.flags & ~RT_MAT_FLAG_FLAT) != 0u) return "unknown flag bits";
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(m.color[k]) || m.color[k] < 0.0f) return "color must be finite and not negative";
        if (!std::isfinite(m.emission[k]) || m.emission[k] < 0.0f) return "emission must be finite and not negative";
    }
    if (!std::isfinite(m.ior) || !(m.ior > 0.0f)) return "ior must be finite and positive";
    if (!(m.alpha > 0.0f && m.alpha <= 1.0f)) return "alpha must lie in (0, 1]";
    for (int k = 0; k < 3; ++k)
        if (!(m.f0[k] >= 0.0f && m.f0[k] <= 1.0f)) return "f0 must lie in [0, 1]";
    return nullptr;
}

static MatRecord material_record(const rt_material& m) {
    MatRecord r = {};
    memcpy(r.color, m.color, 12);
    r.typeFlags = (uint32_t)m.type | (m.flags << 8);
    memcpy(r.f0, m.f0, 12);
    r.alpha = m.alpha;
    memcpy(r.emission, m.emission, 12);
    r.ior = m.ior;
    return r;
}

// The device table from the entries (null: rt_default_material's) and the texture-set binding, whose set
// index rides in bits 16..23 of typeFlags.  Behind the caller's wait for every stream, in place.
static int write_mat_table(rt_context* ctx, const std::vector<rt_material>* entries, const uint8_t* tex) {
    std::vector<MatRecord> recs(256);
    for (uint32_t id = 0; id < 256u; ++id) {
        rt_material m;
        if (entries) m = (*entries)[id];
        else (void)rt_default_material(id, &m);
        recs[id] = material_record(m);
        recs[id].typeFlags |= (uint32_t)tex[id] << 16;
    }
    if (!ctx->dMatTable) {
        if (int rc = dalloc(ctx, &ctx->dMatTable, 256 * sizeof(MatRecord))) return rc;
    }
    HIP_TRY(ctx, hipMemcpy(ctx->dMatTable, recs.data(), 256 * sizeof(MatRecord), hipMemcpyHostToDevice));
    return RT_OK;
}

int rt_set_materials(rt_context* ctx, uint32_t first_id, uint32_t count, const rt_material* m) {
    if (!ctx || !m) return RT_ERR_ARG;
    if (count == 0u || (uint64_t)first_id + (uint64_t)count > 256u) {
        ctx->err = "rt_set_materials: [first_id, first_id + count) must be a non-empty range of the ids 0..255";
        return RT_ERR_ARG;
    }
    for (uint32_t k = 0; k < count; ++k)
        if (const char* bad = material_fault(m[k])) {
            ctx->err = "rt_set_materials: entry " + std::to_string(first_id + k) + ": " + bad;
            return RT_ERR_ARG;
        }
    if (!ctx->inited) { ctx->err = "rt_set_materials before rt_init"; return RT_ERR_STATE; }
    // the kernels in flight read the table, and camera rays traced ahead precede it (spec_matches)
    if (int rc = sync_streams(ctx, false)) return rc;
    std::vector<rt_material> next = ctx->matCustom ? ctx->matHost : std::vector<rt_material>();
    if (next.empty()) {
        next.resize(256);
        for (uint32_t id = 0; id < 256u; ++id) (void)rt_default_material(id, &next[id]);
    }
    for (uint32_t k = 0; k < count; ++k) next[first_id + k] = m[k];
    bool emits = false;
    for (uint32_t id = 0; id < 256u; ++id) {
        const rt_material& e = next[id];
        emits = emits || (e.type == RT_MAT_EMISSIVE && (e.emission[0] > 0.0f || e.emission[1] > 0.0f || e.emission[2] > 0.0f));
    }
    if (int rc = write_mat_table(ctx, &next, ctx->matTex)) return rc;
    ctx->matHost.swap(next);
    ctx->matCustom = true;
    ctx->matEmits = emits;
    ++ctx->matSerial;
    return RT_OK;
}

int rt_get_materials(const rt_context* ctx, uint32_t first_id, uint32_t count, rt_material* out) {
    if (!ctx || !out) return RT_ERR_ARG;
    if (count == 0u || (uint64_t)first_id + (uint64_t)count > 256u) return RT_ERR_ARG;
    for (uint32_t k = 0; k < count; ++k) {
        if (ctx->matCustom) out[k] = ctx->matHost[first_id + k];
        else (void)rt_default_material(first_id + k, &out[k]);
    }
    return RT_OK;
}

int rt_reset_materials(rt_context* ctx) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_reset_materials before rt_init"; return RT_ERR_STATE; }
    if (int rc = sync_streams(ctx, false)) return rc;
    // a texture-set binding keeps the table-reading kernels: their table goes back to the defaults
    if (ctx->matTexBound)
        if (int rc = write_mat_table(ctx, nullptr, ctx->matTex)) return rc;
    ctx->matCustom = false;  // the buffer stays allocated for the next set
    ctx->matEmits = false;
    ++ctx->matSerial;
    return RT_OK;
}

// ---------------------------------------------------------------- texture-set binding

int rt_get_sky_sets(const rt_context* ctx, uint32_t* count) {
    if (!ctx || !count) return RT_ERR_ARG;
    *count = ctx->inited ? (uint32_t)ctx->skySets : (ctx->skySetsCfg > 0 ? (uint32_t)ctx->skySetsCfg : 1u);
    return RT_OK;
}

int rt_get_texture_sets(const rt_context* ctx, uint32_t* count) {
    if (!ctx || !count) return RT_ERR_ARG;
    *count = ctx->inited ? ctx->texSets : (ctx->textureSets > 0 ? (uint32_t)ctx->textureSets : 1u);
    return RT_OK;
}

static int bind_material_textures(rt_context* ctx, const uint8_t (&next)[256]) {
    // the kernels in flight read the table, and camera rays traced ahead precede it (spec_matches)
    if (int rc = sync_streams(ctx, false)) return rc;
    bool bound = false;
    for (uint32_t id = 0; id < 256u; ++id) bound = bound || next[id] != 0u;
    // without a binding and without a custom table no launch reads the device table
    if (bound || ctx->matCustom)
        if (int rc = write_mat_table(ctx, ctx->matCustom ? &ctx->matHost : nullptr, next)) return rc;
    memcpy(ctx->matTex, next, 256);
    ctx->matTexBound = bound;
    ++ctx->matSerial;
    return RT_OK;
}

int rt_set_material_textures(rt_context* ctx, uint32_t first_id, uint32_t count, const uint8_t* sets) {
    if (!ctx || !sets) return RT_ERR_ARG;
    if (count == 0u || (uint64_t)first_id + (uint64_t)count > 256u) {
        ctx->err = "rt_set_material_textures: [first_id, first_id + count) must be a non-empty range of the ids 0..255";
        return RT_ERR_ARG;
    }
    if (!ctx->inited) { ctx->err = "rt_set_material_textures before rt_init"; return RT_ERR_STATE; }
    for (uint32_t k = 0; k < count; ++k)
        if (sets[k] >= ctx->texSets) {
            ctx->err = "rt_set_material_textures: entry " + std::to_string(first_id + k) + ": set " + std::to_string(sets[k]) +
                       " of " + std::to_string(ctx->texSets) + " ([scene] textureSets)";
            return RT_ERR_ARG;
        }
    uint8_t next[256];
    memcpy(next, ctx->matTex, 256);
    memcpy(next + first_id, sets, count);
    return bind_material_textures(ctx, next);
}

int rt_get_material_textures(const rt_context* ctx, uint32_t first_id, uint32_t count, uint8_t* sets) {
    if (!ctx || !sets) return RT_ERR_ARG;
    if (count == 0u || (uint64_t)first_id + (uint64_t)count > 256u) return RT_ERR_ARG;
    if (!ctx->inited) return RT_ERR_STATE;
    memcpy(sets, ctx->matTex + first_id, count);
    return RT_OK;
}

int rt_reset_material_textures(rt_context* ctx) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_reset_material_textures before rt_init"; return RT_ERR_STATE; }
    const uint8_t none[256] = {};
    return bind_material_textures(ctx, none);
}

// a context-stream user of the current LBVH waits for its build on the side stream
int wait_bvh(rt_context* ctx) {
    if (ctx->lbvh().buildOnSide) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->lbvh().buildDone, 0));
    return RT_OK;
}

int rt_trace_primary(rt_context* ctx, int frame_num, int with_detail) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_trace_primary before rt_init"; return RT_ERR_STATE; }
    HostCamera hc;
    rt_camera_update(ctx->camera, ctx->renderW, ctx->renderH, hc);
    TracePrimaryParams p;
    p.cam = rt_trace_camera(hc);
    p.width = (uint32_t)ctx->renderW;
    p.height = (uint32_t)ctx->renderH;
    p.y0 = (uint32_t)ctx->stripY0;
    p.rows = (uint32_t)ctx->stripRows;
    p.nStrips = (uint32_t)ctx->stripCount;
    p.strip = (uint32_t)ctx->stripIndex;
    p.frameNum = frame_num;
    p.bluenoise = ctx->dBlueNoise;
    p.triPos = ctx->lbvh().triPos;
    p.triNrm = ctx->lbvh().triNrm;
    p.nodes = ctx->lbvh().nodes;
    p.tlasNodes = ctx->lbvh().tlasNodes;
    p.hitOut = ctx->dHits;
    p.normalOut = with_detail ? ctx->dHitNrm : nullptr;
    p.fakeNormalOut = with_detail ? ctx->dHitFake : nullptr;
    p.statsOut = with_detail ? ctx->dHitStats : nullptr;
    if (int rc = wait_bvh(ctx)) return rc;
    HIP_TRY(ctx, rtk_launch_trace_primary(&p, ctx->stream));
    return RT_OK;
}

int rt_sync(rt_context* ctx) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) return RT_OK;  // NULL is a valid stream (the null stream): test the init state
    return sync_streams(ctx);
}

int rt_draw_frame_internal(rt_context* ctx);  // frame.cpp

int rt_time_stage(rt_context* ctx, int stage, int iters, float* total_ms) {
    if (!ctx || !total_ms || iters < 1) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_time_stage before rt_init"; return RT_ERR_STATE; }
    if (ctx->postStream) {  // stages are timed serially on the context stream
        void* post = ctx->postStream;
        int rc = rt_set_post_stream(ctx, nullptr);
        if (rc == RT_OK) rc = rt_time_stage(ctx, stage, iters, total_ms);
        const int rc2 = rt_set_post_stream(ctx, post);
        return rc != RT_OK ? rc : rc2;
    }
    const MeshChange same{ctx->dIdxStage, ctx->mesh.triCount, ctx->nv};  // stage 6
    if (stage == 8 && !ctx->skinSet) { ctx->err = "rt_time_stage(8) without a skin (rt_set_skin)"; return RT_ERR_STATE; }
    if (stage == 5 || stage == 6 || stage == 8) {  // the current positions (and indices) again, from a copy: the arrays and the epoch stay as they are
        int rc = sync_streams(ctx, false);
        if (rc == RT_OK) rc = vertex_stage(ctx);
        if (rc != RT_OK) return rc;
        HIP_TRY(ctx, hipMemcpy(ctx->dVertStage, ctx->dVerts, (size_t)ctx->nv * 12, hipMemcpyDeviceToDevice));
        if (stage == 6)
            HIP_TRY(ctx, hipMemcpy(ctx->dIdxStage, ctx->dIdx, (size_t)ctx->mesh.triCount * 12, hipMemcpyDeviceToDevice));
        HIP_TRY(ctx, hipDeviceSynchronize());
    }
    if (stage == 7) {  // nothing reads the spare set: the streams idle, and the spare allocated ahead of the timing
        int rc = sync_streams(ctx, false);
        if (rc == RT_OK) rc = rt_time_sky_generation(ctx);
        if (rc != RT_OK) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (int i = 0; i < iters; ++i) {
        int rc = RT_OK;
        if (stage == 0) rc = rt_build_bvh(ctx);
        else if (stage == 7) rc = rt_time_sky_generation(ctx);
        else if (stage == 5) rc = enqueue_vertex_update(ctx, ctx->dVertStage, 0, ctx->nv, nullptr, true, false);
        else if (stage == 6) rc = enqueue_vertex_update(ctx, ctx->dVertStage, 0, ctx->nv, nullptr, true, false, &same);
        else if (stage == 8) rc = enqueue_pose(ctx, ctx->dSkinMats, nullptr, true, false, ctx->dVertStage);
        else if (stage == 1) rc = rt_trace_primary(ctx, 1 + i, 0);
        else if (stage == 2) rc = rt_path_trace(ctx, 1 + i, 0);
        else if (stage == 3) {
            const int f = ctx->nextFrame++;
            if ((rc = rt_build_bvh(ctx)) == RT_OK && (rc = rt_path_trace(ctx, f, 0)) == RT_OK)
                rc = rt_denoise_post(ctx, f, 0);
        } else if (stage == 4) rc = rt_denoise_post(ctx, 2 + i, 0);
        else { ctx->err = "unknown stage"; return RT_ERR_ARG; }
        if (rc != RT_OK) return rc;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
    HIP_TRY(ctx, hipEventElapsedTime(total_ms, ctx->ev0, ctx->ev1));
    return RT_OK;
}

// Stage 6 split by HIP events between its launches: parts_ms = the sums over `iters` sets of the index
// ingest, the adjacency kernels and the whole-mesh normals update
int rt_time_mesh_set(rt_context* ctx, int iters, float* parts_ms) {
    if (!ctx || !parts_ms || iters < 1) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_time_mesh_set before rt_init"; return RT_ERR_STATE; }
    if (ctx->postStream) {  // timed serially on the context stream, as rt_time_stage
        void* post = ctx->postStream;
        int rc = rt_set_post_stream(ctx, nullptr);
        if (rc == RT_OK) rc = rt_time_mesh_set(ctx, iters, parts_ms);
        const int rc2 = rt_set_post_stream(ctx, post);
        return rc != RT_OK ? rc : rc2;
    }
    hipEvent_t marks[4] = {};
    int rc = RT_OK;
    for (hipEvent_t& e : marks)
        if (hipEventCreate(&e) != hipSuccess) { rc = RT_ERR_HIP; ctx->err = "hipEventCreate failed"; }
    parts_ms[0] = parts_ms[1] = parts_ms[2] = 0.0f;
    ctx->meshMarks = marks;
    for (int i = 0; i < iters && rc == RT_OK; ++i) {
        float one = 0.0f;
        if ((rc = rt_time_stage(ctx, 6, 1, &one)) != RT_OK) break;  // ends with the stream idle
        for (int k = 0; k < 3; ++k) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, marks[k], marks[k + 1]) != hipSuccess) { rc = RT_ERR_HIP; ctx->err = "HIP event timing failed"; }
            parts_ms[k] += ms;
        }
    }
    ctx->meshMarks = nullptr;
    for (hipEvent_t e : marks)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

// per-kernel HIP-event split of `iters` path traces: serial ones (stage 2 of rt_time_stage) or,
// with `frames` set, whole frames (BVH + path trace + denoise/post) as the caller runs them, so
// on a pipelined context each kernel is timed beside the other streams' work (bench.py).  Kernels
// 0..6 are the path trace's, 7..14 (frames only, n >= 15) the denoise / post chain's; a denoise
// kernel's average is over the frames that launched it (its events read 0 ms otherwise).
static int time_kernels(rt_context* ctx, int first_frame, int iters, float* kernel_ms, int n, bool frames) {
    if (!ctx || !kernel_ms || iters < 1 || n < kPtKernels || first_frame < 1) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_time_*_kernels before rt_init"; return RT_ERR_STATE; }
    const int nk = frames ? (n < kFrameKernels ? n : kFrameKernels) : kPtKernels;
    std::vector<hipEvent_t> marks((size_t)iters * 2 * kFrameKernels, nullptr);
    int rc = RT_OK;
    for (size_t i = 0; i < marks.size(); ++i) {
        if ((int)(i % (2 * kFrameKernels)) / 2 >= nk) continue;  // kernels the caller does not ask for
        if (hipEventCreate(&marks[i]) != hipSuccess) { rc = RT_ERR_HIP; ctx->err = "hipEventCreate failed"; break; }
    }
    for (int k = 0; k < n; ++k) kernel_ms[k] = k < nk ? 0.0f : -1.0f;
    for (int i = 0; i < iters && rc == RT_OK; ++i) {
        const int f = first_frame + i;
        if (frames) rc = rt_build_bvh(ctx);
        ctx->ptMarks = marks.data() + (size_t)i * 2 * kFrameKernels;
        if (rc == RT_OK) rc = rt_path_trace(ctx, f, 0);
        ctx->ptMarks = nullptr;
        if (rc == RT_OK && frames) rc = rt_denoise_post(ctx, f, 0);
        ctx->dnMarks = nullptr;
        if (rc == RT_OK && !frames && hipEventSynchronize(marks[(size_t)i * 2 * kFrameKernels + 2 * kPtKernels - 1]) != hipSuccess)
            rc = RT_ERR_HIP;
    }
    if (rc == RT_OK) rc = sync_streams(ctx);
    std::vector<int> cnt(nk, 0);
    for (int i = 0; i < iters && rc == RT_OK; ++i)
        for (int k = 0; k < nk && rc == RT_OK; ++k) {
            float ms = 0.0f;
            hipEvent_t* m = marks.data() + (size_t)i * 2 * kFrameKernels;
            if (hipEventElapsedTime(&ms, m[2 * k], m[2 * k + 1]) != hipSuccess) { rc = RT_ERR_HIP; ctx->err = "HIP event timing failed"; }
            if (k < kPtKernels || ms > 0.0f) {
                kernel_ms[k] += ms;
                ++cnt[k];
            }
        }
    for (int k = 0; k < nk; ++k) kernel_ms[k] = cnt[k] ? kernel_ms[k] / (float)cnt[k] : 0.0f;
    for (auto& m : marks)
        if (m) (void)hipEventDestroy(m);
    return rc;
}

int rt_time_path_trace_kernels(rt_context* ctx, int iters, float* kernel_ms, int n) {
    if (ctx && ctx->inited && ctx->postStream) {  // kernels are timed serially on the context stream
        void* post = ctx->postStream;
        int rc = rt_set_post_stream(ctx, nullptr);
        if (rc == RT_OK) rc = rt_time_path_trace_kernels(ctx, iters, kernel_ms, n);
        const int rc2 = rt_set_post_stream(ctx, post);
        return rc != RT_OK ? rc : rc2;
    }
    return time_kernels(ctx, 1, iters, kernel_ms, n, false);
}

int rt_time_frame_kernels(rt_context* ctx, int first_frame, int iters, float* kernel_ms, int n) {
    return time_kernels(ctx, first_frame, iters, kernel_ms, n, true);
}

int rt_frame_marks_begin(rt_context* ctx, int frames, uint32_t kernel_mask) {
    if (!ctx || frames < 0 || frames > 100000 || (kernel_mask & ~((1u << kFrameKernels) - 1u)) != 0) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_frame_marks_begin before rt_init"; return RT_ERR_STATE; }
    if (int rc = sync_streams(ctx, false)) return rc;  // the events of earlier frames are complete
    ctx->dnMarks = nullptr;
    const size_t need = (size_t)frames * 2 * kFrameKernels;
    while (ctx->markPool.size() < need) {
        hipEvent_t e = nullptr;
        RT_TRY(rt_event(ctx, e, true));
        ctx->markPool.push_back(e);
    }
    ctx->markRing.assign(need, nullptr);  // unmarked kernels keep null entries (no event recorded)
    for (size_t i = 0; i < need; ++i)
        if (kernel_mask & (1u << ((i % (2 * kFrameKernels)) / 2))) ctx->markRing[i] = ctx->markPool[i];
    ctx->markMask = kernel_mask;
    ctx->markFrames = frames;
    ctx->markNext = 0;
    return RT_OK;
}

int rt_frame_marks_read(rt_context* ctx, float* kernel_ms, int n, int* frames_recorded) {
    if (!ctx || !kernel_ms || n < kPtKernels) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_frame_marks_read before rt_init"; return RT_ERR_STATE; }
    if (int rc = sync_streams(ctx)) return rc;
    const int frames = ctx->markNext, nk = n < kFrameKernels ? n : kFrameKernels;
    for (int k = 0; k < nk; ++k) {
        kernel_ms[k] = -1.0f;
        if (!(ctx->markMask & (1u << k))) continue;
        float sum = 0.0f;
        int cnt = 0;
        for (int i = 0; i < frames; ++i) {
            const hipEvent_t* m = ctx->markRing.data() + (size_t)i * 2 * kFrameKernels;
            float ms = 0.0f;
            HIP_TRY(ctx, hipEventElapsedTime(&ms, m[2 * k], m[2 * k + 1]));
            if (k < kPtKernels || ms > 0.0f) {  // a denoise kernel the frame did not launch reads 0
                sum += ms;
                ++cnt;
            }
        }
        kernel_ms[k] = cnt ? sum / (float)cnt : 0.0f;
    }
    if (frames_recorded) *frames_recorded = frames;
    ctx->markFrames = 0;
    ctx->markNext = 0;
    ctx->dnMarks = nullptr;
    return RT_OK;
}

size_t rt_array_bytes(const rt_context* ctx, int what) {
    if (!ctx) return 0;
    // the BVH arrays have the sizes of the current set's last build (before one, the init mesh's), the
    // mesh-level arrays the current mesh's (rt_set_mesh)
    const BvhBufs& set = ctx->lbvh();
    const size_t NP = set.triCountPadded, B = set.B, P = (size_t)ctx->renderW * ctx->renderH;
    if ((what & ~0xFF) != 0) {  // RT_ARR_TEX_SET(k): a colour map of texture set k
        const int base = what & 0xFF;
        const uint32_t k = (uint32_t)what >> 8;
        const bool map = base == RT_ARR_TEX_ALBEDO_AO || base == RT_ARR_TEX_NORMAL_ROUGHNESS;
        return what > 0 && map && k < ctx->texSets ? (size_t)kTexTexels * 8 : 0;
    }
    switch (what) {
        case RT_ARR_VERTICES: return (size_t)ctx->nv * 12;
        case RT_ARR_INDICES: return (size_t)ctx->mesh.triCountPadded * 12;
        case RT_ARR_NORMALS: return (size_t)ctx->nv * 12;
        case RT_ARR_ADJ_OFFSETS: return ((size_t)ctx->nv + 1) * 4;
        case RT_ARR_CORNER_SLOTS: return (size_t)ctx->mesh.triCountPadded * 12;
        case RT_ARR_TRI_POS: return NP * 48;
        case RT_ARR_TRI_NRM: return NP * 48;
        case RT_ARR_AABBS: return NP * 24;
        case RT_ARR_MORTON: return B * 4096;
        case RT_ARR_REORDER: return B * 4096;
        case RT_ARR_NODES: return B * 1024 * 64;
        case RT_ARR_TLAS_AABBS: return B * 24;
        case RT_ARR_TLAS_MORTON: return 4096;
        case RT_ARR_TLAS_REORDER: return 4096;
        case RT_ARR_TLAS_NODES: return B * 64;
        case RT_ARR_BVH_ARENA: return arena_bytes(B, NP);
        case RT_ARR_TLAS_SCENE_AABB: return 24;
        case RT_ARR_BATCH_SCENE_AABBS: return B * 24;
        case RT_ARR_HITS: return P * 16;
        case RT_ARR_HIT_NORMALS: return P * 16;
        case RT_ARR_HIT_FAKE_NORMALS: return P * 16;
        case RT_ARR_HIT_STATS: return P * 16;
        case RT_ARR_RAYS: return P * 4;
        case RT_ARR_SKY_PDF: case RT_ARR_SKY_CDF: return (size_t)kSkySize * 4;
        case RT_ARR_SUN_PDF: case RT_ARR_SUN_CDF: return (size_t)kSunSize * 4;
        case RT_ARR_SUN_DIR: return 16;
        case RT_ARR_HISTOGRAM: return 256;
        case RT_ARR_EXPOSURE: return 16;
        case RT_ARR_COLOR4: return (size_t)((ctx->renderW + 3) / 4) * ((ctx->renderH + 3) / 4) * 8;
        case RT_ARR_COLOR16: return (size_t)((((ctx->renderW + 3) / 4) + 3) / 4) * ((((ctx->renderH + 3) / 4) + 3) / 4) * 8;
        case RT_ARR_COLOR64: {
            const size_t w16 = (((size_t)ctx->renderW + 3) / 4 + 3) / 4, h16 = (((size_t)ctx->renderH + 3) / 4 + 3) / 4;
            return ((w16 + 3) / 4) * ((h16 + 3) / 4) * 8;
        }
        case RT_ARR_RGBA8: return (size_t)ctx->screenW * ctx->screenH * 4;
        case RT_ARR_HDR: return P * 16;
        case RT_ARR_PT_STATS: return P * 16;
        case RT_ARR_TEX_ALBEDO_AO: case RT_ARR_TEX_NORMAL_ROUGHNESS: return (size_t)kTexTexels * 8;
        case RT_ARR_TEX_HEIGHT: return (size_t)kTexTexels * 2;
        case RT_ARR_PT_QUEUE: return 64 * 4;
        case RT_ARR_PT_Q3_ORIGINS:
        case RT_ARR_PT_Q3_DIRS:
        case RT_ARR_PT_Q4_ORIGINS:
        case RT_ARR_PT_Q4_DIRS:
        case RT_ARR_PT_Q3_BETA: return (size_t)ctx->fr.ws.cap * 16;
        // the emitter list of the current set's last build; nothing while that build wrote none.  The
        // count is known on the device only: read behind a wait for the streams
        case RT_ARR_EMITTER_TRIS:
        case RT_ARR_EMITTER_WEIGHTS: {
            if (!set.emBuilt) return 0;
            rt_context* mctx = const_cast<rt_context*>(ctx);
            uint32_t count = 0;
            if (sync_streams(mctx, false) != RT_OK ||
                hipMemcpy(&count, set.emHeader + kEmCount, 4, hipMemcpyDeviceToHost) != hipSuccess)
                return 0;
            return (size_t)count * 4;
        }
        case RT_ARR_EMITTER_CDF: return set.emBuilt ? (size_t)set.emCdfLen * 4 : 0;
        // the pseudo-normal table of the current set's last build; nothing while that build wrote none
        case RT_ARR_PSEUDO_NORMALS: return set.sdfBuilt ? (size_t)set.triCount * 96 : 0;
        case RT_ARR_TRI_MATERIALS: return (size_t)ctx->mesh.triCount;
        case RT_ARR_TRI_MATERIAL_CENSUS: return 256 * sizeof(uint32_t);
        case RT_ARR_SPEC_STATS: return 4 * sizeof(uint32_t);
        default: return 0;
    }
}

int rt_download(const rt_context* cctx, int what, void* dst, size_t bytes) {
    rt_context* ctx = const_cast<rt_context*>(cctx);
    if (!ctx || !dst) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_download before rt_init"; return RT_ERR_STATE; }
    const void* src = nullptr;
    const BvhBufs& set = ctx->lbvh();
    const FrameSet& qs = ctx->fr.set[ctx->fr.lastSlot];  // the bounce queues of the last path trace
    if ((what & ~0xFF) != 0) {  // RT_ARR_TEX_SET(k) | RT_ARR_TEX_ALBEDO_AO / NORMAL_ROUGHNESS
        const size_t need = rt_array_bytes(ctx, what);
        if (need == 0) { ctx->err = "unknown array, or a texture set past [scene] textureSets"; return RT_ERR_ARG; }
        if (bytes < need) { ctx->err = "destination too small"; return RT_ERR_ARG; }
        if (int rc = sync_streams(ctx)) return rc;
        const uint2* chain = (what & 0xFF) == RT_ARR_TEX_ALBEDO_AO ? ctx->fr.texAlbedo : ctx->fr.texNormal;
        HIP_TRY(ctx, hipMemcpy(dst, chain + (size_t)((uint32_t)what >> 8) * kTexTexels, need, hipMemcpyDeviceToHost));
        return RT_OK;
    }
    switch (what) {
        case RT_ARR_VERTICES: src = ctx->dVerts; break;
        case RT_ARR_INDICES: src = ctx->dIdx; break;
        case RT_ARR_NORMALS: src = ctx->dNormals; break;
        case RT_ARR_ADJ_OFFSETS: src = ctx->dAdjOff; break;
        case RT_ARR_CORNER_SLOTS: src = ctx->dCornerSlot; break;
        case RT_ARR_TRI_POS: src = set.triPos; break;
        case RT_ARR_TRI_NRM: src = set.triNrm; break;
        case RT_ARR_AABBS: src = set.aabbs; break;
        case RT_ARR_MORTON: src = set.morton; break;
        case RT_ARR_REORDER: src = set.reorder; break;
        case RT_ARR_NODES: src = set.nodes; break;
        case RT_ARR_BVH_ARENA: src = set.nodes; break;
        case RT_ARR_TLAS_AABBS: src = set.tlasAabbs; break;
        case RT_ARR_TLAS_MORTON: src = set.tlasMorton; break;
        case RT_ARR_TLAS_REORDER: src = set.tlasReorder; break;
        case RT_ARR_TLAS_NODES: src = set.tlasNodes; break;
        case RT_ARR_TLAS_SCENE_AABB: src = set.tlasScene; break;
        case RT_ARR_BATCH_SCENE_AABBS: src = set.batchScene; break;
        case RT_ARR_HITS: src = ctx->dHits; break;
        case RT_ARR_HIT_NORMALS: src = ctx->dHitNrm; break;
        case RT_ARR_HIT_FAKE_NORMALS: src = ctx->dHitFake; break;
        case RT_ARR_HIT_STATS: src = ctx->dHitStats; break;
        case RT_ARR_RAYS: src = ctx->fr.rays; break;
        case RT_ARR_SKY_PDF: src = ctx->fr.sky().skyPdf; break;
        case RT_ARR_SKY_CDF: src = ctx->fr.sky().skyCdf; break;
        case RT_ARR_SUN_PDF: src = ctx->fr.sky().sunPdf; break;
        case RT_ARR_SUN_CDF: src = ctx->fr.sky().sunCdf; break;
        case RT_ARR_HISTOGRAM: src = ctx->fr.histogram; break;
        case RT_ARR_EXPOSURE: src = ctx->fr.exposure; break;
        case RT_ARR_COLOR4: src = ctx->fr.c4; break;
        case RT_ARR_COLOR16: src = ctx->fr.c16; break;
        case RT_ARR_COLOR64: src = ctx->fr.c64; break;
        case RT_ARR_RGBA8:  // the last frame's output, wherever it was drawn (rt_draw_device)
            if (bytes < rt_array_bytes(ctx, what)) { ctx->err = "destination too small"; return RT_ERR_ARG; }
            return copy_rgba_out(ctx, dst);
        case RT_ARR_HDR: src = ctx->fr.hdr; break;
        case RT_ARR_PT_STATS: src = ctx->fr.ptStats; break;
        case RT_ARR_TEX_ALBEDO_AO: src = ctx->fr.texAlbedo; break;
        case RT_ARR_TEX_NORMAL_ROUGHNESS: src = ctx->fr.texNormal; break;
        case RT_ARR_TEX_HEIGHT: src = ctx->fr.texHeight; break;
        case RT_ARR_PT_QUEUE: src = ctx->fr.lastCounters ? ctx->fr.lastCounters : ctx->fr.set[0].counters; break;
        case RT_ARR_PT_Q3_ORIGINS: src = qs.q3.rayO; break;
        case RT_ARR_PT_Q3_DIRS: src = qs.q3.rayD; break;
        case RT_ARR_PT_Q4_ORIGINS: src = qs.q4.rayO; break;
        case RT_ARR_PT_Q4_DIRS: src = qs.q4.rayD; break;
        case RT_ARR_PT_Q3_BETA: src = qs.q3.st1; break;
        case RT_ARR_EMITTER_TRIS: src = set.emTris; break;
        case RT_ARR_EMITTER_WEIGHTS: src = set.emWeights; break;
        case RT_ARR_EMITTER_CDF: src = set.emCdf; break;
        case RT_ARR_PSEUDO_NORMALS: src = set.sdfTable; break;
        case RT_ARR_SUN_DIR: {
            if (bytes < 16) { ctx->err = "destination too small"; return RT_ERR_ARG; }
            float* o = (float*)dst;
            memcpy(o, ctx->fr.sunDir, 12);
            o[3] = ctx->fr.sky().cosThetaMax;
            return RT_OK;
        }
        case RT_ARR_TRI_MATERIALS: {  // what the kernels read; without a table the reference's, 3 everywhere
            const size_t n = ctx->mesh.triCount;
            if (bytes < n) { ctx->err = "destination too small"; return RT_ERR_ARG; }
            if (!ctx->dTriMat) { memset(dst, 3, n); return RT_OK; }
            if (int rc = sync_streams(ctx)) return rc;
            HIP_TRY(ctx, hipMemcpy(dst, ctx->dTriMat, n, hipMemcpyDeviceToHost));
            return RT_OK;
        }
        case RT_ARR_TRI_MATERIAL_CENSUS: {  // triangles per id of that table: the device set's census, else the host's
            uint32_t* out = (uint32_t*)dst;
            if (bytes < 256 * sizeof(uint32_t)) { ctx->err = "destination too small"; return RT_ERR_ARG; }
            if (!ctx->dTriMat) {
                memset(out, 0, 256 * sizeof(uint32_t));
                out[3] = ctx->mesh.triCount;
            } else if (ctx->matDevice) {
                if (int rc = sync_streams(ctx)) return rc;
                HIP_TRY(ctx, hipMemcpy(out, ctx->matPool[ctx->matCur].census, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost));
            } else {
                memcpy(out, ctx->triMatCount, 256 * sizeof(uint32_t));
            }
            return RT_OK;
        }
        case RT_ARR_SPEC_STATS: {  // host counters of the synchronous draws' launches ahead: no wait, nothing dropped
            if (bytes < 4 * sizeof(uint32_t)) { ctx->err = "destination too small"; return RT_ERR_ARG; }
            const FrameResources& fr = ctx->fr;
            const uint32_t v[4] = {fr.specLaunched, fr.specReused, fr.specDropped, fr.spec.valid ? 1u : 0u};
            memcpy(dst, v, sizeof v);
            return RT_OK;
        }
        default: ctx->err = "unknown array"; return RT_ERR_ARG;
    }
    const size_t need = rt_array_bytes(ctx, what);
    if (bytes < need) { ctx->err = "destination too small"; return RT_ERR_ARG; }
    if (int rc = sync_streams(ctx)) return rc;
    if (what == RT_ARR_TRI_POS) {  // the arena's 64-B triangle records -> the reference's [N][3] float4
        HIP_TRY(ctx, hipMemcpy2D(dst, 48, src, 64, 48, set.triCountPadded, hipMemcpyDeviceToHost));
        return RT_OK;
    }
    if (need == 0) return RT_OK;  // an empty emitter list, or none; no pseudo-normal table
    HIP_TRY(ctx, hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
    if (what == RT_ARR_NODES || what == RT_ARR_TLAS_NODES) {
        // the reference's q3 (idxLeft, idxRight, isLeftLeaf, isRightLeaf) from the child references
        // the build keeps in q3.z (traverse.h, the record arena); a slot never written stays zero
        uint32_t* q = (uint32_t*)dst;
        for (size_t k = 0; k < need / 64; ++k) {
            uint32_t* q3 = q + 16 * k + 12;
            const uint32_t cl = q3[2] & 0xFFFFu, cr = q3[2] >> 16;
            q3[0] = cl & 0x7FFFu;
            q3[1] = cr & 0x7FFFu;
            q3[2] = (cl >> 15) & 1u;
            q3[3] = (cr >> 15) & 1u;
        }
    }
    return RT_OK;
}

}  // extern "C"
