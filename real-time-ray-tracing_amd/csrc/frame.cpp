// frame.cpp — the per-frame part of RayTracer::draw (kernel.cu:259-398) behind the C-ABI:
// sky/sun regeneration, the path tracer, G-buffer access.  Denoise and post-processing
// stages are dispatched from here as they land.
//
//   sun direction       UpdateFrame (kernel.cu:119-123), rotate3f (linearMath.h:650-716)
//   UpdateSkyState      sky.cuh:124-146 (host, float + rtmath, like the reference's host code)
//   sky regeneration    kernel.cu:286-307
//   PathTrace launch    kernel.cu:330-350; HistoryCamera::Setup kernel.cu:133-136, 357
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <fstream>
#include <utility>
#include <vector>

#include "context.h"
#include "rtmath.h"

namespace {

constexpr float kPi = 3.1415926535897932384626422832795028841971f;
constexpr float kTwoPi = 6.2831853071795864769252867665590057683943f;
constexpr float kPiOver180 = 0.01745329251f;

// ---- host vector helpers with the device rounding policy (one rounding per op, fma only
// where the reference's TwoProd/InnerProduct use it)
struct V3 { float x, y, z; };
V3 v3(float x, float y, float z) { return V3{x, y, z}; }
V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
V3 operator*(float s, V3 a) { return v3(a.x * s, a.y * s, a.z * s); }
V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
float dop(float a, float b, float c, float d) {
    const float cd = c * d;
    const float err = fmaf(-c, d, cd);
    const float dp = fmaf(a, b, -cd);
    return dp + err;
}
float inner3(float a, float b, float c, float d, float e, float f) {
    const float ef = e * f, efe = fmaf(e, f, -ef);
    const float cd = c * d, cde = fmaf(c, d, -cd);
    const float s2 = cd + ef, dl2 = s2 - cd, s2e = (cd - (s2 - dl2)) + (ef - dl2);
    const float tpv = s2, tpe = cde + (efe + s2e);
    const float ab = a * b, abe = fmaf(a, b, -ab);
    const float s1 = ab + tpv, dl1 = s1 - ab, s1e = (ab - (s1 - dl1)) + (tpv - dl1);
    return s1 + (abe + (tpe + s1e));
}
float dot(V3 a, V3 b) { return inner3(a.x, b.x, a.y, b.y, a.z, b.z); }
V3 cross(V3 a, V3 b) { return v3(dop(a.y, b.z, a.z, b.y), dop(a.z, b.x, a.x, b.z), dop(a.x, b.y, a.y, b.x)); }
V3 normalize(V3 v) {
    const float n = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    return v3(v.x / n, v.y / n, v.z / n);
}

struct Quat { V3 v; float w; };
Quat qmul(const Quat& p, const Quat& q) { return Quat{p.w * q.v + q.w * p.v + cross(p.v, q.v), p.w * q.w - dot(p.v, q.v)}; }

// sunDir = rotate3f(axis, angle, cross(up, axis)).normalized()
V3 sun_direction(float timeOfDay, float sunAxisAngle) {
    const V3 axis = normalize(v3(0.0f, rt_cosf(sunAxisAngle * kPiOver180), rt_sinf(sunAxisAngle * kPiOver180)));
    const float angle = fmodf(timeOfDay * kPi, kTwoPi);
    const V3 v = cross(v3(0.0f, 1.0f, 0.0f), axis);
    const Quat q{normalize(axis) * rt_sinf(angle / 2), rt_cosf(angle / 2)};
    const Quat r = qmul(qmul(q, Quat{v, 0.0f}), Quat{-q.v, q.w});
    return normalize(r.v);
}

// GetFittingData / GetFittingData2 (sky.cuh:90-111): the quintic Bernstein blend of six datasets at
// s.  The six weights depend on s alone, so a sky generation evaluates them once for its 100 blends
// instead of eleven rt_powf per blend (84 us of host time per sky change): each weight is the very
// prefix of the reference's term, in its association, so every blend has the reference's bits.
struct SkyFit { float w[6]; };
SkyFit sky_fit(float s) {
    return SkyFit{{rt_powf(1.0f - s, 5.0f), 5.0f * rt_powf(1.0f - s, 4.0f) * s,
                   10.0f * rt_powf(1.0f - s, 3.0f) * rt_powf(s, 2.0f), 10.0f * rt_powf(1.0f - s, 2.0f) * rt_powf(s, 3.0f),
                   5.0f * (1.0f - s) * rt_powf(s, 4.0f), rt_powf(s, 5.0f)}};
}
float fitting(const float* m, const SkyFit& f, int i) {  // GetFittingData (sky.cuh:90-99)
    return (f.w[0] * m[i] + f.w[1] * m[i + 9] + f.w[2] * m[i + 18] + f.w[3] * m[i + 27] + f.w[4] * m[i + 36] +
            f.w[5] * m[i + 45]);
}
float fitting2(const float* m, const SkyFit& f) {  // GetFittingData2 (sky.cuh:102-111)
    return (f.w[0] * m[0] + f.w[1] * m[1] + f.w[2] * m[2] + f.w[3] * m[3] + f.w[4] * m[4] + f.w[5] * m[5]);
}

struct SkyTablesHost {
    std::vector<float> skyDataSets, skyDataSetsRad, solar, limb, cieX, cieY, cieZ;
};
SkyTablesHost g_tables;  // immutable after the first successful load

bool load_sky_tables(const std::string& path, SkyTablesHost& t, std::string& err) {
    std::ifstream f(path, std::ios::binary);
    if (!f) { err = "cannot read " + path; return false; }
    uint32_t count = 0;
    f.read((char*)&count, 4);
    if (count != 7) { err = "bad sky table file " + path; return false; }
    uint32_t len[7];
    f.read((char*)len, sizeof(len));
    const uint32_t expect[7] = {540, 60, 1800, 60, 10, 10, 10};
    std::vector<float>* dst[7] = {&t.skyDataSets, &t.skyDataSetsRad, &t.solar, &t.limb, &t.cieX, &t.cieY, &t.cieZ};
    for (int i = 0; i < 7; ++i) {
        if (len[i] != expect[i]) { err = "bad sky table sizes in " + path; return false; }
        dst[i]->resize(len[i]);
        f.read((char*)dst[i]->data(), len[i] * 4);
    }
    if (!f) { err = "truncated " + path; return false; }
    return true;
}

bool sky_params_equal(const rt_sky_params& a, const rt_sky_params& b) {
    return a.timeOfDay == b.timeOfDay && a.sunAxisAngle == b.sunAxisAngle && a.skyScalar == b.skyScalar &&
           a.sunScalar == b.sunScalar && a.sunAngle == b.sunAngle;
}

// What a synchronous draw traced ahead will not be used: its counter block holds its counts (the next
// camera launch clears it) and so does specRayCounter (cleared ahead of the next launches).  The
// caller orders whatever it enqueues next behind specDone, or waits for the side stream.
void drop_spec(FrameResources& fr) {
    fr.spec.valid = false;
    fr.syncZeroed[fr.spec.block] = false;
    fr.specCounts = 2;
    ++fr.specDropped;
}

// One generation of the sky tables into `dst` on stream s (kernel.cu:286-307), from the clamped sky
// parameters; under an environment (rt_set_environment) the sky table and its pdf are copies of the
// context's environment table instead of k_sky's output, the sun tables and everything derived as ever
int generate_sky(rt_context* ctx, SkySet& dst, hipStream_t s) {
    FrameResources& fr = ctx->fr;
    const rt_sky_params& sp = ctx->params.sky;
    const V3 sunDir = v3(fr.sunDir[0], fr.sunDir[1], fr.sunDir[2]);
    SkyGenParams p;
    memcpy(p.sunDir, fr.sunDir, 12);
    p.skyScalar = sp.skyScalar;
    p.sunScalar = sp.sunScalar;
    p.sunAngle = sp.sunAngle;
    const float elevation = rt_acosf(sunDir.y);
    const SkyFit se = sky_fit(rt_powf(elevation / (kPi / 2.0f), (1.0f / 3.0f)));
    for (int ch = 0; ch < 10; ++ch) {
        for (int i = 0; i < 9; ++i) p.st.configs[ch * 9 + i] = fitting(g_tables.skyDataSets.data() + ch * 54, se, i);
        p.st.radiances[ch] = fitting2(g_tables.skyDataSetsRad.data() + ch * 6, se);
    }
    const float sunRadius = sp.sunAngle * kPi / 180.0f / 2.0f;
    p.cosThetaMax = rt_cosf(sunRadius);
    p.solar = fr.solar;
    p.limb = fr.limb;
    p.cie = fr.cie;
    p.skyBuffer = dst.sky;
    p.skyPdf = dst.skyPdf;
    p.skyCdf = dst.skyCdf;
    p.sunBuffer = dst.sun;
    p.sunPdf = dst.sunPdf;
    p.sunCdf = dst.sunCdf;
    p.scanSums = fr.scanSums;
    p.skyTree = dst.skyTree;
    p.sunTree = dst.sunTree;
    p.lightSel = dst.lightSel;
    if (ctx->envActive) HIP_TRY(ctx, rtk_launch_sky_env(&p, ctx->envTable, ctx->envPdf, s));
    else HIP_TRY(ctx, rtk_launch_sky(&p, s));
    dst.sunArea = rt_powf(rt_tanf(sunRadius), 2.0f) * kPi;
    dst.cosThetaMax = p.cosThetaMax;
    return RT_OK;
}

void clamp_sky_params(rt_sky_params& sp) {  // kernel.cu:291-293
    sp.sunScalar = sp.sunScalar > 0.00001f ? sp.sunScalar : 0.00001f;
    sp.skyScalar = sp.skyScalar > 0.00001f ? sp.skyScalar : 0.00001f;
    sp.sunAngle = sp.sunAngle > 0.51f ? sp.sunAngle : 0.51f;
}

// kernel.cu:286-307 — regenerate when asked to, or when the sky parameters changed
int update_sky(rt_context* ctx) {
    FrameResources& fr = ctx->fr;
    rt_sky_params& sp = ctx->params.sky;
    const V3 sunDir = sun_direction(sp.timeOfDay, sp.sunAxisAngle);
    fr.sunDir[0] = sunDir.x; fr.sunDir[1] = sunDir.y; fr.sunDir[2] = sunDir.z;
    if (fr.skyValid && !sp.needRegenerate && sky_params_equal(sp, fr.lastSky)) return RT_OK;
    if (ctx->skySets > 1) {
        // Sky sets: the next set in turn, generated on the sky stream behind that
        // set's readers, which are waited for on the device; no host wait and no stream drained.  What
        // was launched earlier keeps the set it was launched with: pipelined frames in flight, and what
        // a synchronous draw traced ahead, which the next path trace drops by the serial (spec_matches).
        hipStream_t s = sky_stream(ctx);
        const int next = (fr.skyCur + 1) % ctx->skySets;
        SkySet& dst = fr.skySet[next];
        if (dst.readValid) HIP_TRY(ctx, hipStreamWaitEvent(s, dst.read, 0));
        if (dst.specValid) HIP_TRY(ctx, hipStreamWaitEvent(s, dst.specRead, 0));
        clamp_sky_params(sp);
        RT_TRY(generate_sky(ctx, dst, s));
        dst.readValid = dst.specValid = false;
        fr.skyCur = next;
    } else {
        // The camera and shade kernels traced ahead read the tables rewritten below: the rewrite follows
        // them, and they are dropped, since the launch parameters hold only the tables' addresses, the sun
        // direction and its angle (a change of skyScalar or sunScalar alone leaves spec_matches true)
        if (fr.spec.valid) {
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->specDone, 0));
            drop_spec(fr);
        }
        if (ctx->postStream) {  // frame pipelining: nothing may read the sky while it is rewritten
            const int rc = sync_streams(ctx, false);
            if (rc != RT_OK) return rc;
        }
        clamp_sky_params(sp);
        RT_TRY(generate_sky(ctx, fr.sky(), ctx->stream));
        if (ctx->postStream) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // before the side stream's camera rays
    }
    ++fr.skySerial;
    fr.skyValid = true;
    sp.needRegenerate = 0;
    fr.lastSky = sp;
    return RT_OK;
}

// LocalizeSample(sunDir) (sampler / sky.cuh): u = cross(n, w), v = cross(n, u) with the
// reference's fma-based DiffOfProducts cross, exactly as the device evaluates it
float dop_host(float a, float b, float c, float d) {
    const float cd = c * d;
    const float err = fmaf(-c, d, cd);
    const float dp = fmaf(a, b, -cd);
    return dp + err;
}
void sun_frame(const float n[3], float t[3], float b[3]) {
    float w[3] = {1.0f, 0.0f, 0.0f};
    if (fabsf(n[0]) > 0.707f) { w[0] = 0.0f; w[1] = 1.0f; }
    auto cross = [](const float* a, const float* c, float* r) {
        r[0] = dop_host(a[1], c[2], a[2], c[1]);
        r[1] = dop_host(a[2], c[0], a[0], c[2]);
        r[2] = dop_host(a[0], c[1], a[1], c[0]);
    };
    cross(n, w, t);
    cross(n, t, b);
}

HistCamera hist_of(const HostCamera& c) {
    HistCamera h;
    memcpy(h.pos, c.pos, 12);
    memcpy(h.left, c.left, 12);
    memcpy(h.up, c.up, 12);
    memcpy(h.dir, c.dir, 12);
    return h;
}

}  // namespace

// The next path trace goes into set k; RenderColorBuffer (rt_get_buffer) follows when it is the old
// set's colour buffer, and stays when it is a denoise output.
static void use_frame_set(FrameResources& fr, int k) {
    const uint2* old = fr.cur().color;
    fr.gbSet = k;
    if (fr.renderColor == old) fr.renderColor = fr.cur().color;
}

// the denoise/post chain of one frame on stream s: phase 0, the histogram exchange, phase 1, the
// rows exchange (the exchanges only for a strip-local denoise, through the caller's hook)
// Whether this context's next denoise is strip-local (multi-GPU: a collective hook, and none of
// the passes that read the whole frame), and its rows [a, b) (the whole frame otherwise).
bool strip_local_denoise(const rt_context* ctx, uint32_t& a, uint32_t& b) {
    const rt_render_pass_settings& ps = ctx->params.pass;
    const uint32_t H = (uint32_t)ctx->renderH;
    a = 0;
    b = H;
    // TemporalFilter2 on: its output (the exchanged history buffer) is then the frame's final HDR
    const bool strip = ctx->stripCount > 1 && ctx->hook != nullptr && !ps.enableNoiseLevelVisualize &&
                       !(ps.enablePostProcess && (ps.enableBloomEffect || ps.enableLensFlare)) &&
                       ps.enableTemporalDenoising2 && ctx->screenW == ctx->renderW && ctx->screenH == ctx->renderH;
    uint32_t sa = 0, sb = H;
    if (!strip || !denoise_rows(H, (uint32_t)ctx->stripCount, (uint32_t)ctx->stripIndex, sa, sb)) return false;
    a = sa;
    b = sb;
    return true;
}

int run_denoise(rt_context* ctx, DenoisePostParams& p, hipStream_t s) {
    rt_strip_exchange x{p.frameNum, (int32_t)p.rowA, (int32_t)p.rowB, p.histOutSet, p.gbSet, p.stripLocal};
    // the G-buffer rows this rank's denoise reads, from the ranks that traced them (opt-in stage:
    // rtx/dist.py's FramePipeline moves them itself, rtx_dist.h's rtd_hook through this call)
    if (ctx->stripCount > 1 && ctx->hook && (ctx->hookStages & (1u << RT_HOOK_GBUFFERS)) &&
        ctx->hook(ctx->hookArg, RT_HOOK_GBUFFERS, (void*)s, &x) != 0) {
        ctx->err = "collective hook failed (G-buffers)";
        return RT_ERR_STATE;
    }
    if (p.marks)  // every marked pair recorded once up front: a kernel this frame does not launch reads 0 ms
        for (int k = 0; k < 2 * kDnKernels; ++k)
            if (p.marks[k]) HIP_TRY(ctx, hipEventRecord(p.marks[k], s));
    // taken when the denoise is issued (a deferred one runs after the earlier frames' swaps)
    p.tileParity = ctx->fr.tileParity;
    p.accum = ctx->fr.accum;
    p.accumAlt = ctx->fr.accumAlt;
    HIP_TRY(ctx, rtk_denoise_phase(&p, s, 0));
    if (p.listUsed) {  // the list chain wrote the other accumulation buffer; the next list frame
        ctx->fr.tileParity ^= 1;  // appends under the other counters
        if (ctx->fr.accumBound || p.stripLocal) {
            // the caller's buffer (a strip-local rank exchanges its rows of it) gets the rows this
            // chain finished — a strip-local rank's own rows, which the rows exchange gathers; the
            // halo rows the later passes read come from accumAlt (their `alt`) — once TemporalFilter,
            // the last reader of the previous frame's accumulation, is done
            const size_t r0 = p.stripLocal ? p.rowA : 0, r1 = p.stripLocal ? p.rowB : p.H;
            HIP_TRY(ctx, hipMemcpyAsync(p.accum + r0 * p.W, p.accumAlt + r0 * p.W, (r1 - r0) * p.W * 8,
                                        hipMemcpyDeviceToDevice, s));
        } else {
            std::swap(ctx->fr.accum, ctx->fr.accumAlt);
        }
    }
    // the histogram is recomputed only with the post chain on; summing a stale one again would
    // multiply it by the rank count every frame
    if (p.stripLocal && p.postProcess && ctx->hook(ctx->hookArg, RT_HOOK_HISTOGRAM, (void*)s, &x) != 0) {
        ctx->err = "collective hook failed (histogram)";
        return RT_ERR_STATE;
    }
    HIP_TRY(ctx, rtk_denoise_phase(&p, s, 1));
    if (!p.stripLocal) return RT_OK;
    if (ctx->hook(ctx->hookArg, RT_HOOK_ROWS, (void*)s, &x) != 0) {
        ctx->err = "collective hook failed (rows)";
        return RT_ERR_STATE;
    }
    // whole-frame outputs exist only after the exchange: the HDR copy of the final colour (the
    // exchanged history buffer) and the caller's draw target (k_scale_post wrote this rank's rows
    // into the exchanged RGBA8 buffer)
    const size_t W = p.W, H = p.H;
    if (p.hdrOut) HIP_TRY(ctx, rtk_hdr_out(p.finalColor, p.hdrOut, W * H, s));
    if (p.rgbaTarget)
        HIP_TRY(ctx, hipMemcpy2DAsync(p.rgbaTarget, (size_t)p.rgbaTargetPitch * 4, p.rgba, (size_t)p.Ws * 4,
                                      (size_t)p.Ws * 4, (size_t)p.Hs, hipMemcpyDeviceToDevice, s));
    return RT_OK;
}

// enqueue a deferred rt_denoise_post on the post stream (frame pipelining)
int issue_pending_post(rt_context* ctx) {
    if (!ctx->postPending) return RT_OK;
    ctx->postPending = false;
    const FrameSet& set = ctx->fr.set[ctx->postPendingSet];
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->postStream, set.ptDone, 0));
    if (ctx->postGather) HIP_TRY(ctx, hipStreamWaitEvent(ctx->postStream, set.gatherDone, 0));
    if (int rc = run_denoise(ctx, ctx->postParams, ctx->postStream)) return rc;
    HIP_TRY(ctx, hipEventRecord(set.postDone, ctx->postStream));
    ctx->fr.renderColor = ctx->postParams.finalColor;  // the launcher's buffer plan names them
    ctx->fr.scaledColor = ctx->postParams.finalScaled;
    return RT_OK;
}

namespace {
// PtLaunchHook of a pipelined frame: after kernel `overlapAfter` the previous frame's denoise
// is issued (it then runs beside the trace stages' latency-bound tails), and after kernel
// `cameraAfter` the gate event the next frame's camera rays wait for is recorded
// the previous frame's deferred denoise, behind everything enqueued so far on the context stream
hipError_t issue_overlapped_post(rt_context* ctx) {
    hipError_t e = hipEventRecord(ctx->overlapEv, ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->postStream, ctx->overlapEv, 0);
    if (e == hipSuccess && issue_pending_post(ctx) != RT_OK) e = hipErrorUnknown;
    return e;
}

hipError_t overlap_hook(void* arg, int kernel) {
    rt_context* ctx = (rt_context*)arg;
    hipError_t e = hipSuccess;
    if (kernel == ctx->overlapAfter && ctx->postPending) e = issue_overlapped_post(ctx);
    if (e == hipSuccess && kernel == ctx->cameraAfter) {
        e = hipEventRecord(ctx->cameraGate, ctx->stream);
        ctx->cameraGated = e == hipSuccess;
    }
    return e;
}
}  // namespace

// wait for the context stream and, when set, the post stream.  `report`: return a kernel's failure
// report (RT_ERR_DEVICE) — rt_sync, the draws, the reads and rt_build_bvh do; the setters that only
// need the streams idle (stream / hook / buffer / texture changes) pass false and do their work, the
// report then waiting for the next reporting call.
int sync_streams(rt_context* ctx, bool report) {
    if (ctx->postStream) {
        const int rc = issue_pending_post(ctx);
        if (rc != RT_OK) return rc;
    }
    if (ctx->sideStream) HIP_TRY(ctx, hipStreamSynchronize(ctx->sideStream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // joined into the context stream before each resolve; on its own only after a failed launch
    if (ctx->leanStream) HIP_TRY(ctx, hipStreamSynchronize(ctx->leanStream));
    if (ctx->postStream) HIP_TRY(ctx, hipStreamSynchronize(ctx->postStream));
    ctx->geomDoneValid = false;  // a vertex update ran on one of these streams: no build waits for it now
    poll_q3(ctx);
    // camera rays a synchronous draw traced ahead are kept only up to the next draw: any call that
    // waits for the streams (a read, a setter, a mode change) drops them
    FrameResources& fr = ctx->fr;
    if (fr.spec.valid) drop_spec(fr);
    if (fr.specCounts) {  // the ray counts of launches ahead: the used ones into the frame's
        HIP_TRY(ctx, rtk_fold_ray_counts(fr.specCounts == 1 ? fr.rayCounter : nullptr, fr.specRayCounter, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        fr.specCounts = 0;
    }
    return report ? check_device_status(ctx) : RT_OK;
}

// The end of a synchronous draw: its frame is complete (kernel.cu:393-397) once the context stream
// is idle; the next frame's camera rays traced ahead may still run on the side stream
static int sync_draw(rt_context* ctx) {
    if (!ctx->fr.spec.valid) return sync_streams(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    poll_q3(ctx);
    return check_device_status(ctx);
}

// The last serial frame's queue-3 length (rt_path_trace's chain choice), if k_pt_resolve has
// stored it: the pinned word pairs the length with the tag of the frame that asked for it, so a
// host that never syncs still picks it up at its next path trace, without waiting.
void poll_q3(rt_context* ctx) {
    FrameResources& fr = ctx->fr;
    if (!fr.q3Pending) return;
    const unsigned long long v = __atomic_load_n(fr.q3Host, __ATOMIC_ACQUIRE);
    if ((uint32_t)(v >> 32) != fr.q3Tag) return;
    fr.lastQ3 = (uint32_t)v;
    fr.q3Pending = false;
}

// Failures the kernels reported into the pinned status words (rt_device.h report_status): the
// LBVH's TLAS workgroup timed out waiting for a batch's publication.  The error is reported once,
// and the launch counters of both LBVH sets are re-armed (a batch that never published left its
// set's counter one short).  Called after the streams are idle (sync_streams) or before a build.
int check_device_status(rt_context* ctx) {
    // rt_set_mesh_device: indices past the vertex count, which the ingest kernel read as 0 (mesh.hip)
    if (const uint32_t badIdx = __atomic_load_n(&ctx->status[kStatusMeshBadIndices], __ATOMIC_ACQUIRE)) {
        __atomic_store_n(&ctx->status[kStatusMeshBadIndices], 0u, __ATOMIC_RELEASE);
        ctx->err = "rt_set_mesh_device: " + std::to_string(badIdx) + " index(es) not below vertex_count were read as 0";
        return RT_ERR_DEVICE;
    }
    // rt_set_triangle_materials_device: ids whose class the caller did not declare, stored as 3 (materials.hip)
    if (const uint32_t badIds = __atomic_load_n(&ctx->status[kStatusMatUndeclared], __ATOMIC_ACQUIRE)) {
        __atomic_store_n(&ctx->status[kStatusMatUndeclared], 0u, __ATOMIC_RELEASE);
        ctx->err = "rt_set_triangle_materials_device: " + std::to_string(badIds) +
                   " id(s) of a class not declared were stored as 3";
        return RT_ERR_DEVICE;
    }
    const uint32_t missing =__atomic_load_n(&ctx->status[kStatusTlasTimeout], __ATOMIC_ACQUIRE);
    if (!missing) return RT_OK;
    const uint32_t build = __atomic_load_n(&ctx->status[kStatusTlasTimeoutBuild], __ATOMIC_ACQUIRE);
    if (ctx->sideStream) HIP_TRY(ctx, hipStreamSynchronize(ctx->sideStream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (const BvhBufs& b : ctx->bvh)
        if (b.counter) HIP_TRY(ctx, hipMemset(b.counter, 0, 64));
    __atomic_store_n(&ctx->status[kStatusTlasTimeout], 0u, __ATOMIC_RELEASE);
    __atomic_store_n(&ctx->status[kStatusTlasTimeoutBuild], 0u, __ATOMIC_RELEASE);
    ctx->err = "LBVH build: the TLAS workgroup timed out waiting for " + std::to_string(missing) +
               " batch publication(s) (last in build " + std::to_string(build) +
               "); the TLAS of that build (and the frames traced on it) may be wrong";
    return RT_ERR_DEVICE;
}

// UpdateFrame's timer (kernel.cu:67-71): the frame time rt_draw already took, the fixed one
// (rt_set_delta_time) or the wall clock since the previous call.  The 75-fps limiter's busy wait
// (timer.h) is frame pacing for a window and is not reproduced.
float frame_delta(rt_context* ctx) {
    FrameResources& fr = ctx->fr;
    if (fr.drawDt >= 0.0f) {
        const float d = fr.drawDt;
        fr.drawDt = -1.0f;
        return d;
    }
    if (ctx->deltaMs > 0.0f) return ctx->deltaMs;
    const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    const float dt = fr.lastDrawTime < 0 ? 1000.0f / 60.0f : (float)((now - fr.lastDrawTime) * 1000.0);
    fr.lastDrawTime = now;
    return dt;
}

// UpdateFrame's dynamic resolution (kernel.cu:77-100): outside the targetFps +-2 band the width
// scales by sqrt(target / frame time), snaps to a multiple of 16, clamps to [minWidth, maxWidth]
// and the height follows at 16:9.  Every render-size buffer was allocated at the initial (max)
// size; a height past maxHeight (a config whose max is not 16:9) is clamped to it so it fits.
void update_dynamic_resolution(rt_context* ctx, float dt) {
    if (!(dt > 0.0f)) return;
    const float hi = 1000.0f / (ctx->targetFps - 2), lo = 1000.0f / (ctx->targetFps + 2);
    int w = ctx->renderW;
    if (hi < dt || lo > dt) {
        const float ratio = sqrtf((1000.0f / ctx->targetFps) / dt);
        w = (int)((float)w * ratio);
    }
    w = w + ((w % 16 < 8) ? (-w % 16) : (16 - w % 16));
    w = w < ctx->minWidth ? ctx->minWidth : w > ctx->maxWidth ? ctx->maxWidth : w;
    int h = (w / 16) * 9;
    if (h > ctx->maxHeight) h = ctx->maxHeight;
    ctx->renderW = w;
    ctx->renderH = h;
    ctx->stripRows = h;
}

static int upload_texture_chain(rt_context* ctx, uint32_t set, int which, const uint16_t* texels, int width, int height,
                                int channels);

// G-buffer / camera-output set k, every buffer at the allocation (largest) size: the G-buffers, the
// camera outputs with the counter block and, with `queues`, the bounce queues with their hit records
// (a set without them uses set 0's).  What exists stays, so a later call may add the queues.
static int alloc_frame_set(rt_context* ctx, int k, bool queues) {
    FrameSet& s = ctx->fr.set[k];
    const size_t P = (size_t)ctx->allocW * ctx->allocH, strip = (size_t)ctx->allocW * ctx->allocStripRows;
    const size_t cap = ctx->fr.ws.cap;
    RT_TRY(dalloc_once(ctx, s.color, P * 8));
    RT_TRY(dalloc_once(ctx, s.normal, P * 8));
    RT_TRY(dalloc_once(ctx, s.albedo, P * 8));
    RT_TRY(dalloc_once(ctx, s.depth, P * 2));
    RT_TRY(dalloc_once(ctx, s.motion, P * 4));
    RT_TRY(dalloc_once(ctx, s.hit0Rec, cap * 16));
    RT_TRY(dalloc_once(ctx, s.hit0Err, cap * 4));
    RT_TRY(dalloc_once(ctx, s.surface, strip * 4));
    RT_TRY(dalloc_once(ctx, s.counters, kWsCounterWords * 4));
    if (!queues) return RT_OK;
    for (PtQueue* q : {&s.q3, &s.q4}) {
        RT_TRY(dalloc_once(ctx, q->rayO, cap * 16));
        RT_TRY(dalloc_once(ctx, q->rayD, cap * 16));
        RT_TRY(dalloc_once(ctx, q->st0, cap * 16));
        RT_TRY(dalloc_once(ctx, q->st1, cap * 16));
        RT_TRY(dalloc_once(ctx, q->st2, cap * 16));
    }
    RT_TRY(dalloc_once(ctx, s.hitRec, cap * 16));
    RT_TRY(dalloc_once(ctx, s.hitErr, cap * 4));
    RT_TRY(dalloc_once(ctx, s.pathL, cap * 16));
    RT_TRY(dalloc_once(ctx, s.pending, strip * 4));
    if (ctx->tune.resumeSplit > 0) RT_TRY(dalloc_once(ctx, s.shade3, cap * 4));
    return RT_OK;
}

// Sky set k's tables and events (set 0's tables are rt_frame_init's)
static int alloc_sky_set(rt_context* ctx, int k) {
    SkySet& s = ctx->fr.skySet[k];
    RT_TRY(dalloc_once(ctx, s.sky, (size_t)kSkySize * 16));
    RT_TRY(dalloc_once(ctx, s.skyPdf, (size_t)kSkySize * 4));
    RT_TRY(dalloc_once(ctx, s.skyCdf, (size_t)kSkySize * 4));
    RT_TRY(dalloc_once(ctx, s.sun, (size_t)kSunSize * 16));
    RT_TRY(dalloc_once(ctx, s.sunPdf, (size_t)kSunSize * 4));
    RT_TRY(dalloc_once(ctx, s.sunCdf, (size_t)kSunSize * 4));
    RT_TRY(dalloc_once(ctx, s.skyTree, (size_t)kSkyTreeNodes * 4));
    RT_TRY(dalloc_once(ctx, s.sunTree, (size_t)kSunTreeNodes * 4));
    RT_TRY(dalloc_once(ctx, s.lightSel, 16));
    for (hipEvent_t* e : {&s.read, &s.specRead}) RT_TRY(rt_event(ctx, *e));
    return RT_OK;
}

// The sky tables again, from the current parameters and environment (the environment setters)
int rt_regenerate_sky(rt_context* ctx) {
    ctx->fr.skyValid = false;
    return update_sky(ctx);
}

// rt_time_stage(7): one sky-set generation into a spare set on the context stream; the current set and
// its serial stay as they are.  The spare is the next set in turn, whose contents nothing reads once the
// streams are idle (the caller's wait), or, on a context with one set, a set allocated here.
int rt_time_sky_generation(rt_context* ctx) {
    FrameResources& fr = ctx->fr;
    const int spare = ctx->skySets > 1 ? (fr.skyCur + 1) % ctx->skySets : 1;
    RT_TRY(alloc_sky_set(ctx, spare));
    return generate_sky(ctx, fr.skySet[spare], ctx->stream);
}

int rt_frame_init(rt_context* ctx) {
    FrameResources& fr = ctx->fr;
    std::string err;
    if (g_tables.solar.empty()) {
        SkyTablesHost t;
        if (!load_sky_tables(rt_data_dir() + "/sky_tables.bin", t, err)) { ctx->err = err; return RT_ERR_IO; }
        g_tables = std::move(t);
    }
    RT_TRY(dalloc_once(ctx, fr.solar, 1800 * 4));
    RT_TRY(dalloc_once(ctx, fr.limb, 60 * 4));
    RT_TRY(dalloc_once(ctx, fr.cie, 30 * 4));
    {  // sky set 0, in the order a context without [scene] skySets has always allocated it
        SkySet& k = fr.skySet[0];
        RT_TRY(dalloc_once(ctx, k.sky, (size_t)kSkySize * 16));
        RT_TRY(dalloc_once(ctx, k.skyPdf, (size_t)kSkySize * 4));
        RT_TRY(dalloc_once(ctx, k.skyCdf, (size_t)kSkySize * 4));
        RT_TRY(dalloc_once(ctx, k.sun, (size_t)kSunSize * 16));
        RT_TRY(dalloc_once(ctx, k.sunPdf, (size_t)kSunSize * 4));
        RT_TRY(dalloc_once(ctx, k.sunCdf, (size_t)kSunSize * 4));
        RT_TRY(dalloc_once(ctx, fr.scanSums, 512 * 4));
        RT_TRY(dalloc_once(ctx, k.skyTree, (size_t)kSkyTreeNodes * 4));
        RT_TRY(dalloc_once(ctx, k.sunTree, (size_t)kSunTreeNodes * 4));
        RT_TRY(dalloc_once(ctx, k.lightSel, 16));
    }
    // texture sets ([scene] textureSets): the sets of one map are one allocation, set k k * kTexTexels in
    RT_TRY(dalloc_once(ctx, fr.texAlbedo, (size_t)ctx->texSets * kTexTexels * 8));
    RT_TRY(dalloc_once(ctx, fr.texNormal, (size_t)ctx->texSets * kTexTexels * 8));
    RT_TRY(dalloc_once(ctx, fr.texHeight, (size_t)kTexTexels * 2));
    HIP_TRY(ctx, hipMemset(fr.texHeight, 0, (size_t)kTexTexels * 2));
    const size_t P = (size_t)ctx->renderW * ctx->renderH;
    RT_TRY(dalloc_once(ctx, fr.rays, P * 4));
    RT_TRY(dalloc_once(ctx, fr.ptStats, P * 16));
    RT_TRY(dalloc_once(ctx, fr.rayCounter, (size_t)kRayCounterSlots * kRayCounterStride * 8));
    {  // wavefront workspace: one entry per traced sample of the strip
        const size_t cap = (size_t)ctx->renderW * ctx->stripRows * ctx->spp;
        if (cap >= (1ull << 31)) { ctx->err = "strip x spp too large for the path-trace queues"; return RT_ERR_ARG; }
        PtWorkspace& ws = fr.ws;
        ws.cap = (uint32_t)cap;
        RT_TRY(alloc_frame_set(ctx, 0, true));  // set 0 has its queues from the start
        RT_TRY(dalloc_once(ctx, fr.syncCount[1], kWsCounterWords * 4));
        RT_TRY(dalloc_once(ctx, fr.syncCount[2], kWsCounterWords * 4));
        fr.syncCount[0] = fr.set[0].counters;
        int dev = 0, cus = 0;
        HIP_TRY(ctx, hipGetDevice(&dev));
        HIP_TRY(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const int perCu = rtk_trace_queue_blocks_per_cu();
        if (cus <= 0) cus = 256;
        // grid of the persistent shade / resume kernels: 5 workgroups per CU (measured)
        ws.persistBlocks = (uint32_t)(cus * 5);
        ws.cus = (uint32_t)cus;
        ws.shadeBlocksPerCu = (uint32_t)(ctx->tune.shadeBlocksPerCu > 0 ? ctx->tune.shadeBlocksPerCu : 0);
        // the queue tracers run below their residency (5 workgroups per CU at 32 KiB of LDS
        // stack each): queue 3 at 3 per CU, queue 4 at 1, so a bounce queue holds
        // more rays than lanes, lanes refill as rays finish, and the CUs keep room for the
        // denoise and next-frame waves beside the traversal tail (measured: DESIGN.md §7)
        int tracePerCu = perCu >= 3 ? 3 : (perCu > 0 ? perCu : 1), trace4PerCu = 1;
        const rt_context::Tuning& tn = ctx->tune;  // [tuning] tracePerCu / trace4PerCu (A/B aids)
        if (tn.tracePerCu > 0 && tn.tracePerCu <= perCu) tracePerCu = tn.tracePerCu;
        if (tn.trace4PerCu > 0 && tn.trace4PerCu <= perCu) trace4PerCu = tn.trace4PerCu;
        ws.traceBlocks = (uint32_t)(cus * tracePerCu);
        // one GPU: a short queue 3 (below kTrace3Short rays, the default view's 323 k) is traced by
        // 2 workgroups per CU, which leaves the next frame's camera waves more room (1.091 -> 1.081
        // ms/frame, four repeats); a long one (the terrain view) keeps all of them (2 per CU there:
        // 4.14 -> 4.44 ms); strip ranks keep 3 (at 2 ranks 0.710 vs 0.727 ms, equal at 4 and 8)
        ws.trace3ShortBlocks = ctx->stripCount == 1 && tn.trace3ShortPerCu > 0 ? (uint32_t)(cus * tn.trace3ShortPerCu) : 0u;
        ws.chain = (uint32_t)tn.chain;  // [tuning] chain = "off" | "serial" | "always" (default serial)
        ws.trace4Blocks = (uint32_t)(cus * trace4PerCu);
    }
    RT_TRY(dalloc_once(ctx, fr.colorB, P * 8));
    RT_TRY(dalloc_once(ctx, fr.accum, P * 8));
    RT_TRY(dalloc_once(ctx, fr.accumAlt, P * 8));  // the list chain's other accumulation buffer (denoise.hip active-tile lists)
    RT_TRY(dalloc_once(ctx, fr.histBuf[0], P * 8));
    RT_TRY(dalloc_once(ctx, fr.histBuf[1], P * 8));
    RT_TRY(dalloc_once(ctx, fr.histDepth, P * 2));
    const size_t W = (size_t)ctx->renderW, H = (size_t)ctx->renderH;
    const size_t W4 = (W + 3) / 4, H4 = (H + 3) / 4, W16 = (W4 + 3) / 4, H16 = (H4 + 3) / 4;
    RT_TRY(dalloc_once(ctx, fr.noise8, ((W + 7) / 8) * ((H + 7) / 8) * 2));
    RT_TRY(dalloc_once(ctx, fr.noise16, ((W + 15) / 16) * ((H + 15) / 16) * 2));
    RT_TRY(dalloc_once(ctx, fr.chainCounter, 4));
    HIP_TRY(ctx, hipMemset(fr.chainCounter, 0, 4));
    {  // active-tile lists (denoise.hip): 2 x 2 x 16 counters 128 B apart, then 2 x 16 partitions of entries
        fr.tileCap = (uint32_t)(((W + 15) / 16) * ((H + 15) / 16));
        const size_t words = 2 * 2 * 16 * 32 + 2 * 16 * (size_t)(fr.tileCap / 16 + 1);
        RT_TRY(dalloc_once(ctx, fr.tileList, words * 4));
        HIP_TRY(ctx, hipMemset(fr.tileList, 0, words * 4));
    }
    RT_TRY(dalloc_once(ctx, fr.c4, W4 * H4 * 8));
    RT_TRY(dalloc_once(ctx, fr.c16, W16 * H16 * 8));
    RT_TRY(dalloc_once(ctx, fr.c64, ((W16 + 3) / 4) * ((H16 + 3) / 4) * 8));
    RT_TRY(dalloc_once(ctx, fr.bloom4, W4 * H4 * 8));
    RT_TRY(dalloc_once(ctx, fr.bloom16, W16 * H16 * 8));
    RT_TRY(dalloc_once(ctx, fr.histogram, 256));
    RT_TRY(dalloc_once(ctx, fr.exposure, 16));
    const size_t Ps = (size_t)ctx->screenW * ctx->screenH;
    RT_TRY(dalloc_once(ctx, fr.scaledA, Ps * 8));
    RT_TRY(dalloc_once(ctx, fr.scaledB, Ps * 8));
    RT_TRY(dalloc_once(ctx, fr.rgba, Ps * 4));
    fr.outRgba = fr.rgba;
    fr.outPitch = (uint32_t)ctx->screenW;
    RT_TRY(dalloc_once(ctx, fr.hdr, P * 16));
    HIP_TRY(ctx, hipMemcpy(fr.solar, g_tables.solar.data(), 1800 * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(fr.limb, g_tables.limb.data(), 60 * 4, hipMemcpyHostToDevice));
    std::vector<float> cie(30);
    memcpy(cie.data(), g_tables.cieX.data(), 40);
    memcpy(cie.data() + 10, g_tables.cieY.data(), 40);
    memcpy(cie.data() + 20, g_tables.cieZ.data(), 40);
    HIP_TRY(ctx, hipMemcpy(fr.cie, cie.data(), 30 * 4, hipMemcpyHostToDevice));
    // soil texture pair (synthetic stand-in for the missing blobs, scene_gen.h): level 0 uploaded,
    // the mip chain built by MipmapGen on the device, as init.cu:524-580 does for the PNGs
    {
        rtscene::TexturePair t;
        rtscene::make_textures(t);
        if (t.albedoAo.size() != (size_t)kTexTexels * 4) { ctx->err = "texture chain size mismatch"; return RT_ERR_STATE; }
        int rc2;
        if ((rc2 = rt_upload_texture(ctx, RT_TEX_SOIL_ALBEDO_AO, t.albedoAo.data(), kTexSize, kTexSize, 4)) != RT_OK ||
            (rc2 = rt_upload_texture(ctx, RT_TEX_SOIL_NORMAL_ROUGHNESS, t.normalRough.data(), kTexSize, kTexSize, 4)) != RT_OK)
            return rc2;
        // sets 1..N-1 start as copies of set 0's chains: a set nobody uploaded to renders like set 0
        for (uint32_t k = 1; k < ctx->texSets; ++k)
            for (uint2* map : {fr.texAlbedo, fr.texNormal})
                HIP_TRY(ctx, hipMemcpy(map + (size_t)k * kTexTexels, map, (size_t)kTexTexels * 8, hipMemcpyDeviceToDevice));
    }
    // further sky sets ([scene] skySets), behind everything a context with one set allocates
    for (int k = 1; k < ctx->skySets; ++k) RT_TRY(alloc_sky_set(ctx, k));
    if (ctx->skySets > 1)
        for (hipEvent_t* e : {&fr.skySet[0].read, &fr.skySet[0].specRead}) RT_TRY(rt_event(ctx, *e));
    HIP_TRY(ctx, hipMemset(fr.set[0].color, 0, P * 8));
    HIP_TRY(ctx, hipMemset(fr.set[0].normal, 0, P * 8));
    HIP_TRY(ctx, hipMemset(fr.set[0].albedo, 0, P * 8));
    HIP_TRY(ctx, hipMemset(fr.set[0].depth, 0, P * 2));
    HIP_TRY(ctx, hipMemset(fr.set[0].motion, 0, P * 4));
    HIP_TRY(ctx, hipMemset(fr.rays, 0, P * 4));
    HIP_TRY(ctx, hipMemset(fr.ptStats, 0, P * 16));
    HIP_TRY(ctx, hipMemset(fr.rayCounter, 0, (size_t)kRayCounterSlots * kRayCounterStride * 8));
    HIP_TRY(ctx, hipMemset(fr.colorB, 0, P * 8));
    HIP_TRY(ctx, hipMemset(fr.accum, 0, P * 8));
    HIP_TRY(ctx, hipMemset(fr.histBuf[0], 0, P * 8));
    HIP_TRY(ctx, hipMemset(fr.histBuf[1], 0, P * 8));
    HIP_TRY(ctx, hipMemset(fr.histDepth, 0, P * 2));
    HIP_TRY(ctx, hipMemset(fr.histogram, 0, 256));
    const float exposure0[4] = {1.0f, 1.0f, 1.0f, 1.0f};  // init.cu:331-333
    HIP_TRY(ctx, hipMemcpy(fr.exposure, exposure0, 16, hipMemcpyHostToDevice));
    fr.renderColor = fr.set[0].color;
    fr.scaledColor = fr.scaledB;
    fr.ready = true;
    return RT_OK;
}

extern "C" {

// init.cu:524-580 for one texture of the atlas: its 16-bit level 0 (stbi_load_16 output, rows of
// width * channels ushorts) to the device, then GenerateMipmap (mipgen.cu:148-178) on the device
int rt_upload_texture(rt_context* ctx, int which, const uint16_t* texels, int width, int height, int channels) {
    if (!ctx || !texels) return RT_ERR_ARG;
    FrameResources& fr = ctx->fr;
    if (!fr.texAlbedo) { ctx->err = "rt_upload_texture before rt_init"; return RT_ERR_STATE; }
    return upload_texture_chain(ctx, 0u, which, texels, width, height, channels);
}

// rt_upload_texture for any texture set: the argument checks ahead of the state's
int rt_upload_texture_set(rt_context* ctx, uint32_t set, int which, const uint16_t* texels, int width, int height,
                          int channels) {
    if (!ctx || !texels) return RT_ERR_ARG;
    const bool map = which == RT_TEX_SOIL_ALBEDO_AO || which == RT_TEX_SOIL_NORMAL_ROUGHNESS;
    if (!map && !(which == RT_TEX_SOIL_HEIGHT && set == 0u)) {
        ctx->err = "rt_upload_texture_set: `which` must be the albedo/AO or the normal/roughness map (the height map is set 0's)";
        return RT_ERR_ARG;
    }
    if (width != kTexSize || height != kTexSize || channels != (map ? 4 : 1)) {
        ctx->err = "rt_upload_texture_set: the textures are 1024 x 1024, 4 channels (height: 1)";
        return RT_ERR_ARG;
    }
    if (!ctx->inited) { ctx->err = "rt_upload_texture_set before rt_init"; return RT_ERR_STATE; }
    if (set >= ctx->texSets) {
        ctx->err = "rt_upload_texture_set: set " + std::to_string(set) + " of " + std::to_string(ctx->texSets) + " ([scene] textureSets)";
        return RT_ERR_ARG;
    }
    return upload_texture_chain(ctx, set, which, texels, width, height, channels);
}

// The stream-ordered upload (texture.hip k_tex_ingest).  The set is written in place, so the write
// follows every reader enqueued so far: the context stream's by stream order, the side stream's (the
// shade kernel of pipelined frames and of synchronous draws' launches ahead) and the lean stream's by
// events recorded here.  Later path traces read it on those streams: they wait for texDone.
int rt_upload_texture_set_device(rt_context* ctx, const rt_texture_upload* u) {
    if (!ctx || !u) return RT_ERR_ARG;
    const char* bad = nullptr;
    if (!u->texels) bad = "texels must not be NULL";
    else if (u->which != RT_TEX_SOIL_ALBEDO_AO && u->which != RT_TEX_SOIL_NORMAL_ROUGHNESS)
        bad = "`which` must be the albedo/AO or the normal/roughness map";
    else if (u->format != RT_TEX_FORMAT_U16 && u->format != RT_TEX_FORMAT_U8) bad = "unknown format";
    else if (((uintptr_t)u->texels & 3u) != 0u) bad = "texels must be 4-byte aligned";
    if (bad) { ctx->err = std::string("rt_upload_texture_set_device: ") + bad; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = "rt_upload_texture_set_device before rt_init"; return RT_ERR_STATE; }
    if (u->set >= ctx->texSets) {
        ctx->err = "rt_upload_texture_set_device: set " + std::to_string(u->set) + " of " + std::to_string(ctx->texSets) +
                   " ([scene] textureSets)";
        return RT_ERR_ARG;
    }
    for (hipEvent_t* e : {&ctx->texSide, &ctx->texLean, &ctx->texDone}) RT_TRY(rt_event(ctx, *e));
    hipStream_t s = ctx->stream;
    if (u->ready_event) HIP_TRY(ctx, hipStreamWaitEvent(s, (hipEvent_t)u->ready_event, 0));
    if (ctx->sideStream) {
        HIP_TRY(ctx, hipEventRecord(ctx->texSide, ctx->sideStream));
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->texSide, 0));
    }
    if (ctx->leanStream) {
        HIP_TRY(ctx, hipEventRecord(ctx->texLean, ctx->leanStream));
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->texLean, 0));
    }
    uint2* chain = (u->which == RT_TEX_SOIL_ALBEDO_AO ? ctx->fr.texAlbedo : ctx->fr.texNormal) + (size_t)u->set * kTexTexels;
    HIP_TRY(ctx, rtk_launch_tex_ingest(u->texels, chain, (uint32_t)kTexSize * kTexSize, (int)u->format, s));
    HIP_TRY(ctx, rtk_launch_mipgen((uint16_t*)chain, kTexSize, kTexLevels, 4, s));
    HIP_TRY(ctx, hipEventRecord(ctx->texDone, s));
    if (ctx->sideStream) HIP_TRY(ctx, hipStreamWaitEvent(ctx->sideStream, ctx->texDone, 0));
    if (ctx->leanStream) HIP_TRY(ctx, hipStreamWaitEvent(ctx->leanStream, ctx->texDone, 0));
    ++ctx->matSerial;  // what a synchronous draw traced ahead sampled the old texels (spec_matches)
    return RT_OK;
}

}  // extern "C"

// level 0 of one chain of texture set `set` from host memory, then its mips; synchronous
static int upload_texture_chain(rt_context* ctx, uint32_t set, int which, const uint16_t* texels, int width, int height,
                         int channels) {
    FrameResources& fr = ctx->fr;
    uint16_t* chain = nullptr;
    int want = 4;
    switch (which) {
        case RT_TEX_SOIL_ALBEDO_AO: chain = (uint16_t*)(fr.texAlbedo + (size_t)set * kTexTexels); break;
        case RT_TEX_SOIL_NORMAL_ROUGHNESS: chain = (uint16_t*)(fr.texNormal + (size_t)set * kTexTexels); break;
        case RT_TEX_SOIL_HEIGHT: chain = fr.texHeight; want = 1; break;
        default: ctx->err = "rt_upload_texture: unknown texture"; return RT_ERR_ARG;
    }
    // the atlas is BUFFER_2D_1024x1024 with 11 levels (init.cu:526-528, texture.h:14-17), asserted there
    if (width != kTexSize || height != kTexSize || channels != want) {
        ctx->err = "rt_upload_texture: the soil textures are 1024 x 1024, 4 channels (height: 1)";
        return RT_ERR_ARG;
    }
    if (ctx->inited) {  // frames in flight may be sampling the old chain
        const int rc = sync_streams(ctx, false);
        if (rc != RT_OK) return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(chain, texels, (size_t)width * height * channels * 2, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, rtk_launch_mipgen(chain, kTexSize, kTexLevels, channels, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

extern "C" {

namespace {
// the bounce-queue slot of a path trace into set g: the set's own queues when allocated (shadeOnSide,
// a synchronous draw's launches ahead), else set 0's
int queue_slot(const FrameResources& fr, int g) { return fr.set[g].q3.rayO ? g : 0; }

// the buffers of a launch's workspace: the camera outputs and counter block of `cam`, the bounce queues of `q`
void bind_workspace(PtWorkspace& ws, const FrameSet& cam, const FrameSet& q) {
    ws.hit0Rec = cam.hit0Rec;
    ws.hit0Err = cam.hit0Err;
    ws.surface = cam.surface;
    ws.counters = cam.counters;
    ws.fetch = ws.counters + 64;
    ws.q3 = q.q3;
    ws.q4 = q.q4;
    ws.hitRec = q.hitRec;
    ws.hitErr = q.hitErr;
    ws.pathL = q.pathL;
    ws.pending = q.pending;
}

// The launch parameters of frame `frame_num`'s path trace into the G-buffers and camera outputs of set
// `cam`, with that set's counter block and the bounce queues of set `q` (the serial frames' block, the
// stream plan and the bookkeeping are rt_path_trace's).  Zero-filled first, so that two calls with the
// same state compare equal byte for byte (the synchronous draws' camera rays traced ahead,
// launch_spec_camera).
void fill_pt_params(const rt_context* ctx, int frame_num, int with_detail, const HostCamera& hc, const FrameSet& cam,
                    const FrameSet& q, PathTraceParams& p) {
    const FrameResources& fr = ctx->fr;
    const BvhBufs& bvh = ctx->lbvh();  // the build the frame is traced on (rt_set_mesh: its triangle count)
    memset(&p, 0, sizeof p);
    p.cam = rt_trace_camera(hc);
    p.tanHalfFov[0] = hc.tanHalfFov[0];
    p.tanHalfFov[1] = hc.tanHalfFov[1];
    p.res[0] = hc.res[0];
    p.res[1] = hc.res[1];
    p.halfRes[0] = hc.res[0] / 2;
    p.halfRes[1] = hc.res[1] / 2;
    p.hist = fr.hist;
    p.width = (uint32_t)ctx->renderW;
    p.height = (uint32_t)ctx->renderH;
    p.y0 = (uint32_t)ctx->stripY0;
    p.rows = (uint32_t)ctx->stripRows;
    p.nStrips = (uint32_t)ctx->stripCount;
    p.strip = (uint32_t)ctx->stripIndex;
    p.frameNum = frame_num;
    p.spp = (uint32_t)ctx->spp;
    p.invSpp = (ctx->spp & (ctx->spp - 1)) == 0 ? 1.0f / (float)ctx->spp : 0.0f;  // exact for a power of two
    p.materialOverride = ctx->materialOverride;
    p.triCount = bvh.triCount;
    p.bluenoise = ctx->dBlueNoise;
    p.triPos = bvh.triPos;
    p.triNrm = bvh.triNrm;
    // geometry motion vectors: the displacement this LBVH set's build recorded, for the first path
    // trace on it (rt_path_trace marks it traced); null: the launch sequence has no motion kernel
    p.triDisp = bvh.dispValid && !bvh.dispTraced ? bvh.triDisp : nullptr;
    p.nodes = bvh.nodes;
    p.tlasNodes = bvh.tlasNodes;
    p.texAlbedo = fr.texAlbedo;
    p.texNormal = fr.texNormal;
    const SkySet& sk = fr.sky();  // the current sky set, held by value from here on
    p.skyBuffer = sk.sky;
    p.sunBuffer = sk.sun;
    p.skyCdf = sk.skyCdf;
    p.sunCdf = sk.sunCdf;
    p.skyTree = sk.skyTree;
    p.sunTree = sk.sunTree;
    p.lightSel = sk.lightSel;
    memcpy(p.sunDir, fr.sunDir, 12);
    p.cosThetaMax = sk.cosThetaMax;
    p.oneMinusCosThetaMax = 1.0f - sk.cosThetaMax;
    sun_frame(fr.sunDir, p.sunT, p.sunB);
    p.colorOut = cam.color;
    p.normalOut = cam.normal;
    p.albedoOut = cam.albedo;
    p.depthOut = cam.depth;
    p.motionOut = cam.motion;
    p.raysOut = with_detail ? fr.rays : nullptr;
    p.statsOut = with_detail ? fr.ptStats : nullptr;
    p.rayCounter = fr.rayCounter;
    p.ws = fr.ws;
    bind_workspace(p.ws, cam, q);
    p.ws.hitRec4 = p.ws.hitRec;  // one stream: queue 3's records are dead once queue 4 is traced
    p.ws.hitErr4 = p.ws.hitErr;
    p.ws.shade3 = q.shade3;  // null: resume<3> unsplit ([tuning] resumeSplit = 0)
    {  // material table (init.cu:215-251): only mirror / glass ids make steps 1-2 trace, only id 4 is
       // MICROFACET (rt_material_classes is the rule).  The override wins over the triangle table,
       // which such a launch does not get; without either it is the reference table, 3 / 6: no class
        const int m = ctx->materialOverride;
        uint32_t classes = ctx->dTriMat ? ctx->triMatClasses : 0u;
        if (m >= 0) {
            const uint8_t id = (uint8_t)(m > 255 ? 255 : m);  // every id >= 10 is of one class
            (void)rt_material_classes(&id, 1, &classes);
        }
        p.triMat = m >= 0 ? nullptr : ctx->dTriMat;
        p.ws.glossy = (classes & RT_MAT_CLASS_GLOSSY) != 0u;
        p.ws.microfacet = (classes & RT_MAT_CLASS_MICROFACET) != 0u;
        // a custom material table (rt_set_materials): an id's class follows its entry, so every class;
        // the one table-reading variant is the all-classes kernels' on the unsplit plan (pt_bounce_plan
        // gives it for these two flags), and an emitter makes queue 4 a closest-hit queue
        // ... and so does a texture-set binding (rt_set_material_textures), whose set index rides in the
        // records: without a custom table they hold rt_default_material's entries
        p.matTable = ctx->matCustom || ctx->matTexBound ? reinterpret_cast<const float4*>(ctx->dMatTable) : nullptr;
        if (p.matTable) p.ws.glossy = p.ws.microfacet = 1;
        p.ws.closest4 = ctx->matCustom && ctx->matEmits ? 1 : 0;
        // emitter sampling: the list of the build this launch traces, when that build wrote one
        if (emitter_active(ctx) && bvh.emBuilt && p.matTable) {
            p.emHeader = bvh.emHeader;
            p.emTris = bvh.emTris;
            p.emCdf = bvh.emCdf;
            p.emitterQ = ctx->emitterQ;
        }
    }
}

// Synchronous draws trace the next frame's camera rays ahead (launch_spec_camera): one GPU, no
// post stream, the G-buffer sets the context's own, [tuning] syncSpec
bool spec_on(const rt_context* ctx) {
    return ctx->tune.syncSpec && ctx->fr.specReady && !ctx->postStream && ctx->stripCount == 1 && !ctx->fr.gbBound;
}

// whether the camera and shade kernels launched with `a` wrote what ones launched with `b` would:
// the same parameters but for those they do not read (or that only select the later kernels)
bool spec_matches(const PathTraceParams& a, uint64_t epochA, uint64_t matA, uint64_t skyA, const PathTraceParams& b,
                  uint64_t epochB, uint64_t matB, uint64_t skyB) {
    // they read the LBVH set of the frame that launched them, the next frame reads the other: both
    // hold the same build (tests/test_gpu_bvh.py) exactly when no vertex update came between them
    if (epochA != epochB) return false;
    // the triangle materials: rt_set_triangle_materials and its reset wait for the streams like every
    // setter, and sync_streams drops what was traced ahead; rt_set_triangle_materials_device does not,
    // and the tables' buffers are recycled, so triMat's address does not tell its contents: the
    // table's serial does
    if (matA != matB) return false;
    // the sky tables: a set's address does not tell its contents either, the sets being taken in turn
    // (update_sky); every generation, into whichever set, moves the serial
    if (skyA != skyB) return false;
    // emitter sampling: whether a launch samples a list at all selects its kernels and must agree
    if ((a.emHeader != nullptr) != (b.emHeader != nullptr)) return false;
    PathTraceParams x = a, y = b;
    for (PathTraceParams* q : {&x, &y}) {
        q->rayCounter = nullptr;  // the launches ahead count into specRayCounter
        q->nodes = q->tlasNodes = nullptr;  // the two LBVH sets of one geometry epoch (above)
        q->triPos = nullptr;
        q->triNrm = nullptr;
        // ... and their emitter lists, which a build writes from its own triangle records and the
        // material tables: the same list under one epoch and one serial.  Compared by address, a draw
        // with emitter sampling on would never use what was traced ahead for it
        q->emHeader = nullptr;
        q->emTris = nullptr;
        q->emCdf = nullptr;
        // triDisp stays: launches ahead never carry one (their frame's own path trace came first),
        // and a launch that does must run its motion kernel
        q->ws.traceBlocks = 0;
        q->ws.shadeBlocksPerCu = 0;  // the shade's grid (dynamic claims: the same result on any grid)
        q->ws.countersZeroed = 0;
        q->ws.chain = 0;
        q->ws.q3HostOut = nullptr;
        q->ws.q3Tag = 0;
        q->ws.shade3 = nullptr;  // read from trace<3> on
    }
    return memcmp(&x, &y, sizeof x) == 0;
}

// PtLaunchHook of a synchronous frame whose successor's camera rays are traced ahead: after
// kernel tune.specAfter (1 = shade) the gate they wait for
hipError_t spec_hook(void* arg, int kernel) {
    rt_context* ctx = (rt_context*)arg;
    return kernel == ctx->tune.specAfter ? hipEventRecord(ctx->specGate, ctx->stream) : hipSuccess;
}

}  // namespace

int rt_path_trace(rt_context* ctx, int frame_num, int with_detail) {
    if (!ctx || frame_num < 1) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_path_trace before rt_init"; return RT_ERR_STATE; }
    FrameResources& fr = ctx->fr;
    if (ctx->postStream) {  // frame pipelining: trace into the set no denoise still reads
        use_frame_set(fr, (fr.gbSet + 1) % kGbSets);
        if (fr.cur().inFlight) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, fr.cur().postDone, 0));
    } else if (spec_on(ctx)) {  // synchronous frames alternate two sets: the next one's camera rays go ahead
        use_frame_set(fr, fr.gbSet ^ 1);
    }
    int rc = update_sky(ctx);
    if (rc != RT_OK) return rc;
    HostCamera hc;
    rt_camera_update(ctx->camera, ctx->renderW, ctx->renderH, hc);
    if (frame_num == 1 || !fr.histValid) fr.hist = hist_of(hc);  // kernel.cu:133-136
    const int g = fr.gbSet, qs = queue_slot(fr, g);  // camera-output slot = G-buffer set
    FrameSet& set = fr.set[g];
    PathTraceParams p;
    fill_pt_params(ctx, frame_num, with_detail, hc, set, fr.set[qs], p);
    if (!ctx->postStream) {  // serial frames: the counter block the resolve before last zeroed
        const int b = fr.syncIdx;
        p.ws.counters = fr.syncCount[b];
        p.ws.countersZeroed = fr.syncZeroed[b] ? 1 : 0;
        p.ws.zeroNext = fr.syncCount[(b + 2) % 3];
        p.ws.fetch = p.ws.counters + 64;
        fr.syncZeroed[b] = fr.syncZeroed[(b + 2) % 3] = false;  // until this frame's resolve is enqueued
    }
    fr.lastCounters = p.ws.counters;
    fr.lastSlot = qs;
    // the fused bounce chain shortens a serial frame; pipelined frames keep the four lean kernels,
    // beside which the next frame's camera waves fit (k_pt_chain's 168 VGPRs at 3 waves/SIMD leave
    // them no room); on ranks of 8 strips too, since the queue tracers' refill-free tail loops
    // (0.436 vs 0.450 ms per rank frame)
    // ... and only while queue 3 is short: a long queue (the terrain view's 3.85 M rays) runs the
    // four kernels faster serially too (4.64 against 5.11 ms per synchronous terrain draw).  The
    // length is that of the last serial frame a host sync completed (q3Host, stored by the frame's
    // resolve kernel, read in sync_streams: a fixed schedule, no event on the stream).
    poll_q3(ctx);
    p.ws.chain = fr.ws.chain == 2 || (fr.ws.chain == 1 && !ctx->postStream && fr.lastQ3 < kChainMaxQ3);
    if (spec_on(ctx)) {  // beside the next frame's camera rays
        if (ctx->tune.specChain >= 0) p.ws.chain = ctx->tune.specChain != 0;  // A/B aid
        // fewer bounce-chain / queue-3 workgroups per CU leave the camera waves room beside them
        // (synchronous draw 0.985 -> 0.972 ms at 2 per CU against 3)
        if (ctx->tune.specTracePerCu > 0) p.ws.traceBlocks = fr.ws.cus * (uint32_t)ctx->tune.specTracePerCu;
    }
    const PtBouncePlan plan = pt_bounce_plan(p.ws);
    fr.lastChain = plan == PtBouncePlan::chain;
    if (plan != PtBouncePlan::split) p.ws.shade3 = nullptr;  // only the split resume<3> keeps a shading list
    if (with_detail) {  // per-pixel counters: everything in order on the context stream
        if (ctx->postStream && (rc = sync_streams(ctx)) != RT_OK) return rc;
        HIP_TRY(ctx, hipMemsetAsync(fr.rays, 0, (size_t)ctx->renderW * ctx->renderH * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(fr.ptStats, 0, (size_t)ctx->renderW * ctx->renderH * 16, ctx->stream));
    }
    // Frame pipelining: the camera rays go to the side stream behind this frame's LBVH build,
    // so they run beside the previous frame's trace tails; they wait only for the readers of
    // this slot's G-buffers (the denoise of frame f-2) and camera outputs (shade of frame f-2).
    const bool side = ctx->postStream && !with_detail;
    hipStream_t cs = side ? ctx->sideStream : ctx->stream;
    p.ws.shadeClaim = !ctx->postStream;  // dynamic batch claims in synchronous frames (pathtrace.hip)
    if (side) {
        if (set.inFlight) HIP_TRY(ctx, hipStreamWaitEvent(cs, set.postDone, 0));
        if (set.camInFlight) HIP_TRY(ctx, hipStreamWaitEvent(cs, set.restDone, 0));
        if (ctx->cameraGated) HIP_TRY(ctx, hipStreamWaitEvent(cs, ctx->cameraGate, 0));
    } else if ((rc = wait_bvh(ctx)) != RT_OK) {
        return rc;
    }
    // rt_frame_marks_begin: this path trace's kernels are bracketed by events (caller's timed frames)
    hipEvent_t* const savedMarks = ctx->ptMarks;
    const bool ringSlot = !ctx->ptMarks && ctx->markNext < ctx->markFrames;
    if (ringSlot) ctx->ptMarks = ctx->markRing.data() + (size_t)(ctx->markNext++) * 2 * kFrameKernels;
    ctx->dnMarks = ctx->ptMarks ? ctx->ptMarks + 2 * kPtKernels : nullptr;  // for this frame's rt_denoise_post
    struct MarksReset {  // every return path leaves ptMarks as it found it
        rt_context* c;
        hipEvent_t* m;
        ~MarksReset() { c->ptMarks = m; }
    } marksReset{ctx, savedMarks};
    if (ringSlot)  // the slot's denoise pairs, recorded once here: a frame no rt_denoise_post follows
        for (int k = 2 * kPtKernels; k < 2 * kFrameKernels; ++k)  // reads 0 ms for them
            if (ctx->ptMarks[k]) HIP_TRY(ctx, hipEventRecord(ctx->ptMarks[k], cs));
    // the camera rays traced ahead by the previous synchronous draw: used when this launch would
    // write what they wrote, dropped otherwise; either way nothing after them runs before they end
    bool reuse = false, reuseShade = false;
    if (fr.spec.valid) {
        fr.spec.valid = false;
        HIP_TRY(ctx, hipStreamWaitEvent(cs, ctx->specDone, 0));
        reuse = !side && spec_matches(p, ctx->geomEpoch, ctx->matSerial, fr.skySerial, fr.spec.p, fr.spec.epoch,
                                        fr.spec.matSerial, fr.spec.skySerial);
        reuseShade = reuse && fr.spec.shade;
        if (!reuse) p.ws.countersZeroed = 0;  // their counts are in the block: the launcher clears it
        fr.specCounts = reuse ? 1 : 2;  // folded into the frame's (or cleared) ahead of the next ones
        ++(reuse ? fr.specReused : fr.specDropped);
    }
    if (reuse) {
        for (int k = 0; k < (reuseShade ? 4 : 2) && ctx->ptMarks; ++k)  // zero-length slots for the marks
            if (ctx->ptMarks[k]) HIP_TRY(ctx, hipEventRecord(ctx->ptMarks[k], cs));
    } else {
        HIP_TRY(ctx, rtk_launch_pt_camera(&p, cs, ctx->ptMarks));
    }
    // the shade kernel follows on the side stream, so it runs beside the previous frame's queue
    // tracers instead of after them (its bounce queues are this set's own)
    const bool shadeSide = side && ctx->shadeOnSide && qs == g;
    if (shadeSide) HIP_TRY(ctx, rtk_launch_pt_shade(&p, cs, ctx->ptMarks));
    if (side) {
        HIP_TRY(ctx, hipEventRecord(set.camDone, cs));
        // overlapAfter 0: the previous frame's denoise waits only for that frame's path trace
        // (everything on the context stream so far), not for this frame's camera rays and shade
        if (ctx->overlapAfter == 0 && ctx->postPending) HIP_TRY(ctx, issue_overlapped_post(ctx));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, set.camDone, 0));
    }
    PtLaunchHook hook{overlap_hook, ctx};
    const bool askQ3 = !side && !fr.q3Pending;  // serial frames: queue 3's length for the next chain choice
    if (askQ3) {
        if (!fr.q3Host) {
            HIP_TRY(ctx, hipHostMalloc((void**)&fr.q3Host, sizeof(unsigned long long), hipHostMallocDefault));
            *fr.q3Host = 0ull;
        }
        p.ws.q3HostOut = fr.q3Host;  // stored by k_pt_resolve (no copy on the stream)
        p.ws.q3Tag = ++fr.q3Tag;
    }
    PtLaunchHook shook{spec_hook, ctx};
    // The lean pass of the split resume<3> on its own stream (resumeSplit 2): pipelined one-GPU frames
    // only; serial frames, detail launches and strip ranks keep one stream.  Queue 4's hit records then
    // go to this set's camera-hit planes, which nothing reads once the shade kernel is done (the set's
    // next camera kernel waits for its restDone).
    PtLeanFork lean{ctx->leanStream, set.leanTraced, set.leanDone};
    const bool fork = side && plan == PtBouncePlan::split && ctx->leanStream && ctx->stripCount == 1;
    if (fork) {
        p.ws.hitRec4 = p.ws.hit0Rec;
        p.ws.hitErr4 = p.ws.hit0Err;
    }
    const PtLeanFork* lf = fork ? &lean : nullptr;
    if (shadeSide) HIP_TRY(ctx, rtk_launch_pt_rest_after_shade(&p, ctx->stream, ctx->ptMarks, &hook, lf));
    else if (reuseShade) HIP_TRY(ctx, rtk_launch_pt_rest_after_shade(&p, ctx->stream, ctx->ptMarks, &shook, lf));
    else {
        const PtLaunchHook* h = ctx->postStream ? &hook : spec_on(ctx) && !with_detail ? &shook : nullptr;
        HIP_TRY(ctx, rtk_launch_pt_rest(&p, ctx->stream, ctx->ptMarks, h, lf));
    }
    // pending only once the launches that store it are enqueued: a failed launch leaves the next
    // serial frame to ask again instead of freezing the chain choice
    if (askQ3) fr.q3Pending = true;
    // the material table this path trace read, marked behind its last reading kernel: the shade kernel
    // on the side stream and the forked lean pass are joined into the context stream above
    if (p.triMat && ctx->matPoolReady) {
        rt_context::MatTable& tab = ctx->matPool[ctx->matCur];
        HIP_TRY(ctx, hipEventRecord(tab.read, ctx->stream));
        tab.readValid = true;
    }
    // ... and the sky set, which the next generation into it waits for (update_sky)
    if (ctx->skySets > 1) {
        SkySet& sk = fr.sky();
        HIP_TRY(ctx, hipEventRecord(sk.read, ctx->stream));
        sk.readValid = true;
    }
    if (p.triDisp) ctx->lbvh().dispTraced = true;  // later path traces on this build see no motion of the geometry
    if (!ctx->postStream) {  // block b + 2 is zeroed by this frame's resolve, enqueued above
        const int b = fr.syncIdx;
        fr.syncZeroed[(b + 2) % 3] = true;
        fr.syncIdx = (b + 1) % 3;
    }
    if (ctx->postPending && (rc = issue_pending_post(ctx)) != RT_OK) return rc;
    if (ctx->postStream) {
        HIP_TRY(ctx, hipEventRecord(set.restDone, ctx->stream));
        set.camInFlight = true;
        HIP_TRY(ctx, hipEventRecord(ctx->lbvh().readDone, ctx->stream));
        ctx->lbvh().readInFlight = true;
    }
    fr.renderColor = set.color;
    fr.hist = hist_of(hc);  // HistoryCamera::Setup after PathTrace (kernel.cu:357)
    fr.histValid = true;
    ctx->lastFrame = frame_num;
    return RT_OK;
}

int rt_get_ray_count(rt_context* ctx, uint64_t* rays, int reset) {
    if (!ctx || !rays) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_get_ray_count before rt_init"; return RT_ERR_STATE; }
    if (int rc = sync_streams(ctx)) return rc;  // the side stream's camera and shade kernels add rays too
    std::vector<unsigned long long> part((size_t)kRayCounterSlots * kRayCounterStride);
    const size_t bytes = part.size() * 8;
    HIP_TRY(ctx, hipMemcpy(part.data(), ctx->fr.rayCounter, bytes, hipMemcpyDeviceToHost));
    unsigned long long v = 0;
    for (int k = 0; k < kRayCounterSlots; ++k) v += part[(size_t)k * kRayCounterStride];
    *rays = v;
    if (reset) HIP_TRY(ctx, hipMemset(ctx->fr.rayCounter, 0, bytes));
    return RT_OK;
}

// TemporalSpatialDenoising + PostProcessing + CopyToOutput for the frame just path traced
int rt_denoise_post(rt_context* ctx, int frame_num, int with_hdr) {
    if (!ctx || frame_num < 1) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_denoise_post before rt_init"; return RT_ERR_STATE; }
    const rt_render_pass_settings& ps = ctx->params.pass;
    if (ps.enablePostProcess && ps.enableToneMapping &&
        (ctx->params.post.toneMappingType < 0 || ctx->params.post.toneMappingType > 3)) {
        ctx->err = "toneMappingType must be 0 (Uncharted), 1 (ACES1), 2 (ACES2) or 3 (Reinhard)";
        return RT_ERR_ARG;
    }
    FrameResources& fr = ctx->fr;
    DenoisePostParams p;
    p.W = (uint32_t)ctx->renderW;
    p.H = (uint32_t)ctx->renderH;
    p.Ws = (uint32_t)ctx->screenW;
    p.Hs = (uint32_t)ctx->screenH;
    p.frameNum = frame_num;
    p.histW = (uint32_t)ctx->histW;
    p.histH = (uint32_t)ctx->histH;
    p.deltaTime = frame_delta(ctx);
    p.temporal = ps.enableTemporalDenoising;
    p.localSpatial = ps.enableLocalSpatialFilter;
    p.visualize = ps.enableNoiseLevelVisualize;
    p.wideSpatial = ps.enableWideSpatialFilter;
    p.temporal2 = ps.enableTemporalDenoising2;
    p.postProcess = ps.enablePostProcess;
    p.downScale = ps.enableDownScalePasses;
    p.histogramOn = ps.enableHistogram;
    p.autoExposure = ps.enableAutoExposure;
    p.sharpen = ps.enableSharpening;
    p.tonemap = ps.enableToneMapping;
    p.gain = ctx->params.post.gain;
    p.fixedExposure = ctx->params.post.exposure;
    p.maxWhite = ctx->params.post.maxWhite;
    p.gamma = ctx->params.post.gamma;
    p.dn = ctx->params.denoise;
    {  // the depth weights' divisors as reciprocals (rtmath.h rt_div_rcp), where that is exact
        const float sig[3] = {p.dn.temporal_denoise_sigma_depth, p.dn.local_denoise_sigma_depth,
                              p.dn.large_denoise_sigma_depth};
        p.rcpDepthOk = 0;
        for (int k = 0; k < 3; ++k) {
            volatile float d = sig[k];  // the IEEE reciprocal, as the oracle's check computes it
            p.rcpDepth[k] = 1.0f / d;
            if (rt_div_rcp_ok(sig[k])) p.rcpDepthOk |= 1 << k;
        }
    }
    FrameSet& set = fr.cur();  // the set the frame's path trace wrote
    p.colorA = set.color;
    p.colorB = fr.colorB;
    p.normal = set.normal;
    p.albedo = set.albedo;
    p.depth = set.depth;
    p.motion = set.motion;
    p.accum = fr.accum;
    p.histColor = fr.histBuf[fr.histIdx];
    p.histColorOut = fr.histBuf[fr.histIdx ^ 1];
    p.histOutSet = fr.histIdx ^ 1;
    p.gbSet = fr.gbSet;
    p.ty0 = 0;
    p.ty1 = (int)((p.H + 15) / 16);
    {  // multi-GPU strip-local denoise: only with a collective hook, and for the passes it covers
        uint32_t a = 0, b = p.H;
        p.stripLocal = strip_local_denoise(ctx, a, b) ? 1 : 0;
        // the list passes at two threads per pixel ([tuning] dnSplit: 0 never, 1 synchronous frames
        // only, 2 always): in pipelined frames their 512-thread workgroups wait for room beside the
        // next frame's camera and shade waves (A/B in DESIGN.md §4.2)
        p.listSplit = ctx->tune.dnSplit == 2 || (ctx->tune.dnSplit == 1 && !ctx->postStream) ? 1 : 0;
        p.listFold = ctx->tune.dnFold ? 1 : 0;
        p.rowA = a;
        p.rowB = b;
    }
    p.histDepth = fr.histDepth;
    p.noise8 = fr.noise8;
    p.noise16 = fr.noise16;
    p.chainCounter = fr.chainCounter;
    p.tileList = fr.tileList;
    p.tileCap = fr.tileCap;
    p.tileParity = fr.tileParity;
    p.listUsed = 0;
    p.exposureDone = 0;
    p.histDepthInTemporal = 0;
    p.c4 = fr.c4;
    p.c16 = fr.c16;
    p.c64 = fr.c64;
    p.histogram = fr.histogram;
    p.exposure = fr.exposure;
    p.scaledA = fr.scaledA;
    p.scaledB = fr.scaledB;
    // rt_draw_device: the caller's device target; a strip-local denoise writes its rows into the
    // exchanged buffer instead and copies the whole frame to the target after the rows exchange
    p.rgbaTarget = (p.stripLocal && fr.drawTarget) ? fr.drawTarget : nullptr;
    p.rgbaTargetPitch = fr.drawTarget ? fr.drawPitch : 0u;
    p.rgba = (fr.drawTarget && !p.stripLocal) ? fr.drawTarget : fr.rgba;
    p.rgbaPitch = (fr.drawTarget && !p.stripLocal) ? fr.drawPitch : (uint32_t)ctx->screenW;
    fr.outRgba = fr.drawTarget ? fr.drawTarget : fr.rgba;
    fr.outPitch = fr.drawTarget ? fr.drawPitch : (uint32_t)ctx->screenW;
    p.bluenoise = ctx->dBlueNoise;
    p.hdrOut = with_hdr ? fr.hdr : nullptr;
    p.marks = ctx->dnMarks;  // the frame's denoise marks (rt_frame_marks_begin / rt_time_frame_kernels)
    ctx->dnMarks = nullptr;
    p.bloom = ps.enablePostProcess && ps.enableBloomEffect;
    p.toneMappingType = ctx->params.post.toneMappingType;
    p.bloom4 = fr.bloom4;
    p.bloom16 = fr.bloom16;
    p.lensFlare = 0;
    p.sunPos[0] = p.sunPos[1] = 0.0f;
    p.sunUv[0] = p.sunUv[1] = 0;
    if (ps.enablePostProcess && ps.enableLensFlare) {
        // UpdateFrame's sunPos / sunUv (kernel.cu:126-127): Camera::WorldToScreenSpace(pos + sunDir)
        HostCamera hc;
        rt_camera_update(ctx->camera, ctx->renderW, ctx->renderH, hc);
        const V3 pos = v3(hc.pos[0], hc.pos[1], hc.pos[2]);
        const V3 sd = v3(fr.sunDir[0], fr.sunDir[1], fr.sunDir[2]);
        const V3 w = pos + sd;
        const V3 d = v3(w.x - pos.x, w.y - pos.y, w.z - pos.z);
        const V3 vs = v3(dot(v3(hc.left[0], hc.left[1], hc.left[2]), d), dot(v3(hc.up[0], hc.up[1], hc.up[2]), d),
                         dot(v3(hc.dir[0], hc.dir[1], hc.dir[2]), d));
        const float sx = vs.x / vs.z, sy = vs.y / vs.z;
        const float nx = sx / hc.tanHalfFov[0], ny = sy / hc.tanHalfFov[1];
        float px = 0.5f - nx * 0.5f, py = 0.5f - ny * 0.5f;
        const int ux = (int)floorf(px * (float)ctx->renderW), uy = (int)floorf(py * (float)ctx->renderH);
        // PostProcessing's predicate (postprocessing.cu:90)
        if (px > 0 && px < 1 && py > 0 && py < 1 && sd.y > -0.0f &&
            dot(sd, v3(hc.dir[0], hc.dir[1], hc.dir[2])) > 0) {
            px -= 0.5f;
            py -= 0.5f;
            px *= (float)ctx->renderW / (float)ctx->renderH;
            p.lensFlare = 1;
            p.sunPos[0] = px;
            p.sunPos[1] = py;
            p.sunUv[0] = ux;
            p.sunUv[1] = uy;
        }
    }
    if (ctx->postStream) {
        // deferred: enqueued behind the next path trace's first kernels (overlap_hook) or at the
        // next host read; it waits for everything enqueued so far on the context stream (this
        // frame's path trace and any G-buffer gathers)
        int rc = issue_pending_post(ctx);
        if (rc != RT_OK) return rc;
        HIP_TRY(ctx, hipEventRecord(set.ptDone, ctx->stream));
        ctx->postGather = ctx->gatherOn;
        if (ctx->postGather) HIP_TRY(ctx, hipEventRecord(set.gatherDone, ctx->gatherStream));
        ctx->postParams = p;
        ctx->postPendingSet = fr.gbSet;
        ctx->postPending = true;
        set.inFlight = true;
    } else {
        if (ctx->gatherOn) {
            HIP_TRY(ctx, hipEventRecord(fr.set[0].gatherDone, ctx->gatherStream));
            HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, fr.set[0].gatherDone, 0));
        }
        if (int rc = run_denoise(ctx, p, ctx->stream)) return rc;
        fr.renderColor = p.finalColor;
        fr.scaledColor = p.finalScaled;
    }
    if (p.temporal2) fr.histIdx ^= 1;
    ctx->histW = ctx->renderW;  // the history buffers now hold this frame's size
    ctx->histH = ctx->renderH;
    return RT_OK;
}

// the last frame's RGBA8 (screen size) into tightly packed host memory; waits for the frame
int copy_rgba_out(rt_context* ctx, void* dst) {
    if (int rc = sync_streams(ctx)) return rc;
    const FrameResources& fr = ctx->fr;
    const size_t row = (size_t)ctx->screenW * 4;
    HIP_TRY(ctx, hipMemcpy2D(dst, row, fr.outRgba, (size_t)fr.outPitch * 4, row, (size_t)ctx->screenH,
                             hipMemcpyDeviceToHost));
    return RT_OK;
}

namespace {
// Synchronous draws: the next frame's LBVH rebuild (BuildBvhLevel1/2, one per frame as in the
// reference) goes into the other set on the side stream, where it runs beside this frame's
// denoise instead of ahead of the next frame's path trace.  The build depends on nothing this
// frame computes, only on the geometry: it carries the epoch it gathered (prebuiltEpoch), and a
// draw that finds another one (a vertex update since) builds again.  The other set was last read
// by the previous frame, which has finished, or by a device ray query enqueued since
// (rt_trace_rays_device), which may not have: the side stream waits for the last such query.
int prebuild_next_bvh(rt_context* ctx) {
    RT_TRY(ensure_bvh_pair(ctx));
    const int next = ctx->bvhSet ^ 1;
    BvhBufs& b = ctx->bvh[next];
    if (b.queryInFlight) {
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->sideStream, b.queryDone, 0));
        b.queryInFlight = false;
    }
    int rc = check_device_status(ctx);  // a previous build's failure, as in rt_build_bvh
    if (rc == RT_OK) rc = build_bvh(ctx, next, ctx->sideStream);
    ctx->bvhPrebuilt = rc == RT_OK;
    ctx->prebuiltEpoch = ctx->geomEpoch;
    ctx->prebuiltMatSerial = ctx->matSerial;
    return rc;
}

// Set 1's G-buffers and camera outputs and the events of the synchronous draws' camera rays traced
// ahead (allocated at full size, once)
int ensure_sync_spec(rt_context* ctx) {
    FrameResources& fr = ctx->fr;
    RT_TRY(alloc_frame_set(ctx, 1, true));  // with bounce queues: the shade goes ahead too
    if (!fr.specRayCounter) {  // zero between uses (rtk_fold_ray_counts)
        RT_TRY(dalloc_once(ctx, fr.specRayCounter, (size_t)kRayCounterSlots * kRayCounterStride * 8));
        HIP_TRY(ctx, hipMemset(fr.specRayCounter, 0, (size_t)kRayCounterSlots * kRayCounterStride * 8));
    }
    RT_TRY(rt_event(ctx, ctx->specGate));
    RT_TRY(rt_event(ctx, ctx->specDone));
    fr.specReady = true;
    return RT_OK;
}

// Synchronous draws: the next frame's camera rays, traced ahead on the side stream after this
// frame's shade kernel (spec_hook) and ahead of the next frame's LBVH build (prebuild_next_bvh), on
// this frame's LBVH, into the other G-buffer set and the next counter block, with the camera, sky
// and frame number as they are now.
// They then run beside this frame's bounces and denoise instead of at the head of the next draw.
// The next rt_path_trace uses them only when its own launch parameters equal these (spec_matches:
// a host that moves the camera, changes the sky, the size or the frame number, or updates vertices
// (another geometry epoch) between the draws gets them traced again), and any call that waits for
// the streams drops them, so no draw's output depends on this.
int launch_spec_camera(rt_context* ctx) {
    FrameResources& fr = ctx->fr;
    if (!ctx->tune.syncSpec || ctx->postStream || ctx->stripCount != 1 || fr.gbBound) return RT_OK;
    int rc;
    if (!fr.specReady && (rc = ensure_sync_spec(ctx)) != RT_OK) return rc;
    HostCamera hc;
    rt_camera_update(ctx->camera, ctx->renderW, ctx->renderH, hc);
    PathTraceParams p;  // on this frame's LBVH set (spec_matches)
    const int g = fr.gbSet ^ 1;
    fill_pt_params(ctx, ctx->nextFrame, 0, hc, fr.set[g], fr.set[queue_slot(fr, g)], p);
    const int b = fr.syncIdx;
    p.ws.counters = fr.syncCount[b];
    p.ws.countersZeroed = fr.syncZeroed[b] ? 1 : 0;
    p.ws.zeroNext = fr.syncCount[(b + 2) % 3];
    p.ws.fetch = p.ws.counters + 64;
    p.ws.shadeClaim = 1;  // as rt_path_trace sets it for synchronous frames
    p.rayCounter = fr.specRayCounter;
    if (fr.specCounts) {  // the last launches' ray counts: into the frame's if they were used, then cleared
        HIP_TRY(ctx, rtk_fold_ray_counts(fr.specCounts == 1 ? fr.rayCounter : nullptr, fr.specRayCounter, ctx->sideStream));
        fr.specCounts = 0;
    }
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->sideStream, ctx->specGate, 0));
    HIP_TRY(ctx, rtk_launch_pt_camera(&p, ctx->sideStream, nullptr));
    // then the next frame's shade kernel, which runs beside this frame's denoise (synchronous draw
    // 0.969 -> 0.945 ms, the terrain view 3.70 -> 3.33 ms), on 2 workgroups per CU so that the
    // denoise passes' workgroups fit beside it (0.942 -> 0.935 ms)
    const bool shade = ctx->tune.specShade == 2 || (ctx->tune.specShade == 1 && !fr.lastChain);
    if (shade) {
        if (ctx->tune.specShadePerCu > 0) p.ws.shadeBlocksPerCu = (uint32_t)ctx->tune.specShadePerCu;
        HIP_TRY(ctx, rtk_launch_pt_shade(&p, ctx->sideStream, nullptr));
    }
    HIP_TRY(ctx, hipEventRecord(ctx->specDone, ctx->sideStream));
    if (shade && p.triMat && ctx->matPoolReady) {  // the table that shade kernel reads (rt_set_triangle_materials_device)
        rt_context::MatTable& tab = ctx->matPool[ctx->matCur];
        HIP_TRY(ctx, hipEventRecord(tab.specRead, ctx->sideStream));
        tab.specValid = true;
    }
    if (ctx->skySets > 1) {  // the sky set these kernels read
        SkySet& sk = fr.sky();
        HIP_TRY(ctx, hipEventRecord(sk.specRead, ctx->sideStream));
        sk.specValid = true;
    }
    fr.syncZeroed[b] = false;
    fr.spec.valid = true;
    ++fr.specLaunched;
    fr.spec.shade = shade;
    fr.spec.block = b;
    fr.spec.epoch = ctx->geomEpoch;  // of this frame's LBVH, built or checked by enqueue_frame just before
    fr.spec.matSerial = ctx->matSerial;
    fr.spec.skySerial = fr.skySerial;
    fr.spec.p = p;
    return RT_OK;
}

// UpdateFrame (kernel.cu:61-137) + BuildBvhLevel1/2 + PathTrace + TemporalSpatialDenoising +
// PostProcessing + CopyToOutput of one frame, enqueued (draw, kernel.cu:259-398); the RGBA8 image
// goes to `target` (pitch in pixels) or, when NULL, to the context's own buffer
int enqueue_frame(rt_context* ctx, uint32_t* target, uint32_t pitch, bool hdr) {
    const int frame = ctx->nextFrame++;
    int rc;
    ctx->fr.drawDt = -1.0f;
    const float dt = frame_delta(ctx);  // UpdateFrame's timer, read once per frame
    if (ctx->useDynamicResolution && frame > 1 && ctx->fullFrame) update_dynamic_resolution(ctx, dt);
    rt_input_control_update(ctx, dt);  // UpdateFrame's InputControlUpdate (kernel.cu:117)
    ctx->fr.drawDt = dt;
    // built beside the previous synchronous frame, from the geometry this frame draws
    // (with emitter sampling the build carries a list of the triangle materials too: also from this table)
    if (ctx->bvhPrebuilt && !ctx->postStream && ctx->prebuiltEpoch == ctx->geomEpoch &&
        (!emitter_active(ctx) || ctx->prebuiltMatSerial == ctx->matSerial)) {
        ctx->bvhPrebuilt = false;
        ctx->bvhSet ^= 1;  // the path trace waits for its build (wait_bvh)
    } else if ((rc = rt_build_bvh(ctx)) != RT_OK) {
        return rc;
    }
    if ((rc = rt_path_trace(ctx, frame, 0)) != RT_OK) return rc;
    // the next frame's camera rays first on the side stream, then its LBVH (which only its bounces read)
    if (!ctx->postStream && (rc = launch_spec_camera(ctx)) != RT_OK) return rc;
    if (!ctx->postStream && (rc = prebuild_next_bvh(ctx)) != RT_OK) return rc;
    ctx->fr.drawTarget = target;
    ctx->fr.drawPitch = pitch;
    rc = rt_denoise_post(ctx, frame, hdr ? 1 : 0);
    ctx->fr.drawTarget = nullptr;
    return rc;
}
}  // namespace

// RayTracer::draw (kernel.cu:259-398) with host outputs: BVH rebuild, path trace, denoise, post,
// output, then the copies to the caller's host buffers
int rt_draw(rt_context* ctx, uint8_t* rgba8_out, float* hdr_out) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_draw before rt_init"; return RT_ERR_STATE; }
    int rc;
    if ((rc = enqueue_frame(ctx, nullptr, 0, hdr_out != nullptr)) != RT_OK) return rc;
    if ((rc = sync_draw(ctx)) != RT_OK) return rc;
    if (rgba8_out && (rc = copy_rgba_out(ctx, rgba8_out)) != RT_OK) return rc;
    if (hdr_out)
        HIP_TRY(ctx, hipMemcpy(hdr_out, ctx->fr.hdr, (size_t)ctx->renderW * ctx->renderH * 16, hipMemcpyDeviceToHost));
    return RT_OK;
}

// RayTracer::draw(SurfObj* renderTarget) (kernel.cu:259, CopyToOutput kernel.cu:26-59): the frame's
// RGBA8 image is written straight into caller-owned device memory.  RT_DRAW_ASYNC returns once the
// frame is enqueued and runs the frame pipeline (an internal post stream unless the caller set one).
int rt_draw_device(rt_context* ctx, void* rgba8_device, size_t pitch_bytes, int flags) {
    if (!ctx || !rgba8_device) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_draw_device before rt_init"; return RT_ERR_STATE; }
    const size_t row = (size_t)ctx->screenW * 4;
    if (pitch_bytes == 0) pitch_bytes = row;
    if (pitch_bytes < row || pitch_bytes % 4 != 0 || ((uintptr_t)rgba8_device & 3u) != 0) {
        ctx->err = "rt_draw_device: pitch must be >= screen width * 4 and a multiple of 4, target 4-byte aligned";
        return RT_ERR_ARG;
    }
    if ((flags & ~RT_DRAW_ASYNC) != 0) { ctx->err = "rt_draw_device: unknown flags"; return RT_ERR_ARG; }
    int rc;
    if ((flags & RT_DRAW_ASYNC) && !ctx->postStream) {  // pipelined frames on an internal low-priority stream
        if (!ctx->ownPostStream && (rc = rt_create_stream(ctx, &ctx->ownPostStream, false)) != RT_OK) return rc;
        if ((rc = rt_set_post_stream(ctx, ctx->ownPostStream)) != RT_OK) return rc;
    }
    if ((rc = enqueue_frame(ctx, (uint32_t*)rgba8_device, (uint32_t)(pitch_bytes / 4), false)) != RT_OK) return rc;
    if (!(flags & RT_DRAW_ASYNC)) return sync_draw(ctx);  // draw ends with a device sync (kernel.cu:393-397)
    return RT_OK;
}

int rt_set_stream(rt_context* ctx, void* stream) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_set_stream before rt_init"; return RT_ERR_STATE; }
    int rc = sync_streams(ctx, false);
    if (rc != RT_OK) return rc;
    ctx->stream = stream == RT_OWN_STREAM ? ctx->ownStream : (hipStream_t)stream;  // NULL: the null stream
    return RT_OK;
}

int rt_set_collective_hook(rt_context* ctx, rt_collective_fn fn, void* arg) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_set_collective_hook before rt_init"; return RT_ERR_STATE; }
    int rc = sync_streams(ctx, false);
    if (rc != RT_OK) return rc;
    ctx->hook = fn;
    ctx->hookArg = arg;
    return RT_OK;
}

int rt_set_hook_stages(rt_context* ctx, uint32_t stage_mask) {
    if (!ctx || (stage_mask & ~7u) != 0) return RT_ERR_ARG;
    // HISTOGRAM and ROWS are what make a strip-local denoise equal one GPU's: a mask without them
    // would leave each rank with its own exposure and stale peer rows, so it is refused
    const uint32_t need = (1u << RT_HOOK_HISTOGRAM) | (1u << RT_HOOK_ROWS);
    if ((stage_mask & need) != need) {
        ctx->err = "rt_set_hook_stages: HISTOGRAM and ROWS are mandatory; the mask only opts into GBUFFERS";
        return RT_ERR_ARG;
    }
    ctx->hookStages = stage_mask;
    return RT_OK;
}

int rt_set_gather_stream(rt_context* ctx, void* stream) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_set_gather_stream before rt_init"; return RT_ERR_STATE; }
    int rc = sync_streams(ctx, false);
    if (rc != RT_OK) return rc;
    for (FrameSet& s : ctx->fr.set) RT_TRY(rt_event(ctx, s.gatherDone));
    ctx->gatherOn = stream != RT_STREAM_OFF;  // NULL is the null stream, as in rt_set_stream
    ctx->gatherStream = ctx->gatherOn ? (hipStream_t)stream : nullptr;
    return RT_OK;
}

// The second LBVH set, the side stream and the build events: frame f+1's build beside frame f
// (pipelined frames, and the prebuild of synchronous draws)
int ensure_bvh_pair(rt_context* ctx) {
    RT_TRY(alloc_bvh_set(ctx, ctx->bvh[1]));
    if (ctx->geomMotion) RT_TRY(ensure_geometry_motion(ctx));  // else with rt_set_geometry_motion
    if (ctx->emitterOn) RT_TRY(ensure_emitter_lists(ctx));     // else with rt_set_emitter_sampling
    if (ctx->sdfOn) RT_TRY(ensure_sdf_tables(ctx));            // else with rt_set_signed_distance
    // lowest priority: it should fill what the trace chain leaves idle
    if (!ctx->sideStream) RT_TRY(rt_create_stream(ctx, &ctx->sideStream, false));
    for (BvhBufs& b : ctx->bvh) RT_TRY(rt_event(ctx, b.buildDone));
    for (BvhBufs& b : ctx->bvh) RT_TRY(rt_event(ctx, b.readDone));
    return RT_OK;
}

int rt_set_post_stream(rt_context* ctx, void* stream) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_set_post_stream before rt_init"; return RT_ERR_STATE; }
    int rc = sync_streams(ctx, false);
    if (rc != RT_OK) return rc;
    FrameResources& fr = ctx->fr;
    for (FrameSet& s : fr.set) s.inFlight = false;
    fr.syncZeroed[0] = fr.syncZeroed[1] = fr.syncZeroed[2] = false;  // pipelined frames use (and dirty) set 0's block too
    if (!stream) {
        ctx->postStream = nullptr;
        return RT_OK;
    }
    // further G-buffer sets and camera outputs, sized for the largest frame: with dynamic resolution the
    // current size may be smaller and grow back later
    for (int k = 1; k < kGbSets; ++k) RT_TRY(alloc_frame_set(ctx, k, false));
    // the shade kernel runs on the side stream, with bounce queues per set ([tuning] shadeOnSide:
    // A/B aid); measured: one GPU 1.025 -> 0.970 ms/frame, one rank's share at
    // 2 / 4 / 8 ranks 0.648 -> 0.650 / 0.495 -> 0.482 / 0.453 -> 0.411 ms
    ctx->shadeOnSide = ctx->tune.shadeOnSide;
    for (int k = 1; ctx->shadeOnSide && k < kGbSets; ++k) RT_TRY(alloc_frame_set(ctx, k, true));
    RT_TRY(ensure_bvh_pair(ctx));
    for (FrameSet& s : fr.set) {
        for (hipEvent_t* e : {&s.camDone, &s.restDone, &s.ptDone, &s.postDone}) RT_TRY(rt_event(ctx, *e));
        if (ctx->tune.resumeSplit == 2) {
            RT_TRY(rt_event(ctx, s.leanTraced));
            RT_TRY(rt_event(ctx, s.leanDone));
        }
        s.camInFlight = false;
    }
    for (BvhBufs& b : ctx->bvh) b.readInFlight = b.buildOnSide = false;
    RT_TRY(rt_event(ctx, ctx->overlapEv));
    RT_TRY(rt_event(ctx, ctx->cameraGate));
    ctx->cameraGated = false;
    // the next frame's camera rays: ungated on one GPU (they run beside this frame's shade and
    // queue-3 traversal), after this frame's trace<3> on two GPUs and its resume<3> on four, where
    // a rank's tails are shorter, and after its shade on eight (measured per N: DESIGN.md §7)
    ctx->cameraAfter = ctx->stripCount == 1 ? 0 : ctx->stripCount == 2 ? 2 : ctx->stripCount < 8 ? 3 : 1;
    if (ctx->tune.overlapAfter >= 0) ctx->overlapAfter = ctx->tune.overlapAfter;  // [tuning] A/B aids
    if (ctx->tune.cameraAfter >= 0) ctx->cameraAfter = ctx->tune.cameraAfter;
    if (ctx->tune.resumeSplit == 2 && !ctx->leanStream) RT_TRY(rt_create_stream(ctx, &ctx->leanStream, false));
    ctx->postStream = (hipStream_t)stream;
    return RT_OK;
}

int rt_bind_buffer(rt_context* ctx, int name, void* device_ptr, size_t bytes) {
    if (!ctx || !device_ptr) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_bind_buffer before rt_init"; return RT_ERR_STATE; }
    const int set = (name >> 8) & 3;  // RT_BUF_SET1 / RT_BUF_SET2 / RT_BUF_SET3
    name &= 0xFF;
    if (set >= kGbSets) { ctx->err = "rt_bind_buffer: no such G-buffer set"; return RT_ERR_ARG; }
    const size_t need = rt_alloc_bytes(ctx, name);  // later frames may be larger than the current one
    if (need == 0 || bytes < need) { ctx->err = "rt_bind_buffer: unknown buffer or too small"; return RT_ERR_ARG; }
    if (((uintptr_t)device_ptr & 15u) != 0) { ctx->err = "rt_bind_buffer: pointer must be 16-byte aligned"; return RT_ERR_ARG; }
    int rc = sync_streams(ctx, false);
    if (rc != RT_OK) return rc;
    FrameResources& fr = ctx->fr;
    FrameSet& s = fr.set[set];
    switch (name) {
        case RT_BUF_RENDER_COLOR:
            // RenderColorBuffer follows when it is the current set's colour buffer (as in use_frame_set)
            if (set == fr.gbSet && fr.renderColor == s.color) fr.renderColor = (uint2*)device_ptr;
            s.color = (uint2*)device_ptr;
            break;
        case RT_BUF_NORMAL: s.normal = (uint2*)device_ptr; break;
        case RT_BUF_ALBEDO: s.albedo = (uint2*)device_ptr; break;
        case RT_BUF_DEPTH: s.depth = (uint16_t*)device_ptr; break;
        case RT_BUF_MOTION: s.motion = (uint32_t*)device_ptr; break;
        // the strip-local denoise's exchanged buffers (set 0 only, except the history pair 0 / 1);
        // the new memory takes over the old contents (a frame-persistent state)
        case RT_BUF_ACCUMULATION:
        case RT_BUF_HISTORY_COLOR:
        case RT_BUF_HISTOGRAM:
        case RT_BUF_RGBA8: {
            if (set > (name == RT_BUF_HISTORY_COLOR ? 1 : 0)) { ctx->err = "rt_bind_buffer: no such set"; return RT_ERR_ARG; }
            void** slot = name == RT_BUF_ACCUMULATION ? (void**)&fr.accum
                          : name == RT_BUF_HISTORY_COLOR ? (void**)&fr.histBuf[set]
                          : name == RT_BUF_HISTOGRAM ? (void**)&fr.histogram : (void**)&fr.rgba;
            HIP_TRY(ctx, hipMemcpy(device_ptr, *slot, need, hipMemcpyDeviceToDevice));
            if (name == RT_BUF_RGBA8 && fr.outRgba == fr.rgba) fr.outRgba = (uint32_t*)device_ptr;
            // a caller-owned accumulation buffer stays the accumulation buffer: the list chain
            // writes the internal one and copies its rows back instead of swapping the two
            if (name == RT_BUF_ACCUMULATION) fr.accumBound = true;
            *slot = device_ptr;
            return RT_OK;
        }
        default: ctx->err = "rt_bind_buffer: this buffer cannot be bound"; return RT_ERR_ARG;
    }
    fr.gbBound = true;  // synchronous frames then stay in their set (no camera rays traced ahead)
    // ... and that set is 0, the one a name without a set flag binds: the launches ahead alternated
    // two sets up to here and may have left the context in set 1, whose buffers are its own
    if (!ctx->postStream && fr.gbSet != 0) use_frame_set(fr, 0);
    return RT_OK;
}

// bytes a render-size buffer has at the allocation (maximum) size
size_t rt_alloc_bytes(const rt_context* ctx, int name) {
    const size_t P = (size_t)ctx->allocW * ctx->allocH;
    switch (name) {
        case RT_BUF_RENDER_COLOR: case RT_BUF_NORMAL: case RT_BUF_ALBEDO: case RT_BUF_ACCUMULATION:
        case RT_BUF_HISTORY_COLOR: return P * 8;
        case RT_BUF_HISTOGRAM: return 256;
        case RT_BUF_RGBA8: return (size_t)ctx->screenW * ctx->screenH * 4;
        case RT_BUF_DEPTH: return P * 2;
        case RT_BUF_MOTION: return P * 4;
        default: return 0;
    }
}

size_t rt_buffer_bytes(const rt_context* ctx, int name) {
    if (!ctx) return 0;
    const size_t P = (size_t)ctx->renderW * ctx->renderH;
    switch (name) {
        case RT_BUF_RENDER_COLOR: case RT_BUF_NORMAL: case RT_BUF_ALBEDO: case RT_BUF_ACCUMULATION:
        case RT_BUF_HISTORY_COLOR: return P * 8;
        case RT_BUF_SCALED_COLOR: return (size_t)ctx->screenW * ctx->screenH * 8;
        case RT_BUF_DEPTH: case RT_BUF_HISTORY_DEPTH: return P * 2;
        case RT_BUF_NOISE_LEVEL: return (size_t)((ctx->renderW + 7) / 8) * ((ctx->renderH + 7) / 8) * 2;
        case RT_BUF_NOISE_LEVEL16: return (size_t)((ctx->renderW + 15) / 16) * ((ctx->renderH + 15) / 16) * 2;
        case RT_BUF_MOTION: return P * 4;
        case RT_BUF_SKY: return (size_t)kSkySize * 16;
        case RT_BUF_SUN: return (size_t)kSunSize * 16;
        case RT_BUF_HISTOGRAM: return 256;
        case RT_BUF_RGBA8: return (size_t)ctx->screenW * ctx->screenH * 4;
        default: return 0;
    }
}

int rt_get_buffer(const rt_context* cctx, int name, void* dst, size_t bytes) {
    rt_context* ctx = const_cast<rt_context*>(cctx);
    if (!ctx || !dst) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_get_buffer before rt_init"; return RT_ERR_STATE; }
    if (int rc = sync_streams(ctx)) return rc;  // also issues a deferred denoise (buffer plan)
    const FrameResources& fr = ctx->fr;
    const void* src = nullptr;
    switch (name) {
        case RT_BUF_RENDER_COLOR: src = fr.renderColor; break;
        case RT_BUF_ACCUMULATION: src = fr.accum; break;
        case RT_BUF_HISTORY_COLOR: src = fr.histBuf[fr.histIdx]; break;
        case RT_BUF_HISTORY_DEPTH: src = fr.histDepth; break;
        case RT_BUF_SCALED_COLOR: src = fr.scaledColor; break;
        case RT_BUF_NOISE_LEVEL: src = fr.noise8; break;
        case RT_BUF_NOISE_LEVEL16: src = fr.noise16; break;
        case RT_BUF_NORMAL: src = fr.cur().normal; break;
        case RT_BUF_ALBEDO: src = fr.cur().albedo; break;
        case RT_BUF_DEPTH: src = fr.cur().depth; break;
        case RT_BUF_MOTION: src = fr.cur().motion; break;
        case RT_BUF_SKY: src = fr.sky().sky; break;
        case RT_BUF_SUN: src = fr.sky().sun; break;
        case RT_BUF_HISTOGRAM: src = fr.histogram; break;
        case RT_BUF_RGBA8:
            if (bytes < rt_buffer_bytes(ctx, name)) { ctx->err = "destination too small"; return RT_ERR_ARG; }
            return copy_rgba_out(ctx, dst);
        default: ctx->err = "buffer not available in this revision"; return RT_ERR_ARG;
    }
    const size_t need = rt_buffer_bytes(ctx, name);
    if (bytes < need) { ctx->err = "destination too small"; return RT_ERR_ARG; }
    if (int rc = sync_streams(ctx)) return rc;
    HIP_TRY(ctx, hipMemcpy(dst, src, need, hipMemcpyDeviceToHost));
    return RT_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- camera file I/O, image dumps
namespace {
// Camera (kernel.cuh:78-100), __align__(16): the reference's on-disk record
struct CameraRecord {
    float pos[3], pitch;
    float dir[3], focal;
    float left[3], aperture;
    float up[3], yaw;
    float resolution[2], inversedResolution[2];
    float fov[2], tanHalfFov[2];
    float adjustedLeft[3], unused3;
    float adjustedUp[3], unused4;
    float adjustedFront[3], unused5;
    float apertureLeft[3], unused6;
    float apertureUp[3], unused7;
};
static_assert(sizeof(CameraRecord) == 176, "Camera record layout");
}  // namespace

extern "C" int rt_save_camera(const rt_context* cctx, const char* path) {
    rt_context* ctx = const_cast<rt_context*>(cctx);
    if (!ctx || !path || !*path) return RT_ERR_ARG;
    HostCamera hc;
    rt_camera_update(ctx->camera, ctx->renderW, ctx->renderH, hc);
    CameraRecord r{};
    memcpy(r.pos, hc.pos, 12);
    r.pitch = hc.pitch;
    memcpy(r.dir, hc.dir, 12);
    r.focal = hc.focal;
    memcpy(r.left, hc.left, 12);
    r.aperture = hc.aperture;
    memcpy(r.up, hc.up, 12);
    r.yaw = hc.yaw;
    memcpy(r.resolution, hc.res, 8);
    memcpy(r.inversedResolution, hc.invRes, 8);
    memcpy(r.fov, hc.fov, 8);
    memcpy(r.tanHalfFov, hc.tanHalfFov, 8);
    memcpy(r.adjustedLeft, hc.adjustedLeft, 12);
    memcpy(r.adjustedUp, hc.adjustedUp, 12);
    memcpy(r.adjustedFront, hc.adjustedFront, 12);
    memcpy(r.apertureLeft, hc.apertureLeft, 12);
    memcpy(r.apertureUp, hc.apertureUp, 12);
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f) { ctx->err = std::string("cannot write camera file ") + path; return RT_ERR_IO; }
    f.write(reinterpret_cast<const char*>(&r), sizeof(r));
    return f ? RT_OK : RT_ERR_IO;
}

extern "C" int rt_load_camera(rt_context* ctx, const char* path) {
    if (!ctx || !path || !*path) return RT_ERR_ARG;
    std::ifstream f(path, std::ios::binary);
    CameraRecord r{};
    if (!f || !f.read(reinterpret_cast<char*>(&r), sizeof(r))) {
        ctx->err = std::string("cannot read camera file ") + path;
        return RT_ERR_IO;
    }
    memcpy(ctx->camera.pos, r.pos, 12);
    ctx->camera.pitch = r.pitch;
    ctx->camera.yaw = r.yaw;
    ctx->camera.focal = r.focal;
    ctx->camera.aperture = r.aperture;
    ctx->camera.fovX = r.fov[0];
    return RT_OK;
}

extern "C" int rt_save_image(rt_context* ctx, const char* path, int kind) {
    if (!ctx || !path || !*path || (kind != RT_IMAGE_PPM_RGBA8 && kind != RT_IMAGE_PFM_HDR)) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_save_image before rt_init"; return RT_ERR_STATE; }
    if (int rc = sync_streams(ctx)) return rc;
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f) { ctx->err = std::string("cannot write image ") + path; return RT_ERR_IO; }
    if (kind == RT_IMAGE_PPM_RGBA8) {
        const size_t n = (size_t)ctx->screenW * ctx->screenH;
        std::vector<uint8_t> rgba(n * 4), rgb(n * 3);
        if (int rc = copy_rgba_out(ctx, rgba.data())) return rc;
        for (size_t i = 0; i < n; ++i) memcpy(&rgb[3 * i], &rgba[4 * i], 3);
        f << "P6\n" << ctx->screenW << " " << ctx->screenH << "\n255\n";
        f.write(reinterpret_cast<const char*>(rgb.data()), (std::streamsize)rgb.size());
    } else {
        const int W = ctx->renderW, H = ctx->renderH;
        std::vector<uint16_t> c((size_t)W * H * 4);
        HIP_TRY(ctx, hipMemcpy(c.data(), ctx->fr.renderColor, c.size() * 2, hipMemcpyDeviceToHost));
        std::vector<float> rgb((size_t)W * H * 3);
        for (int y = 0; y < H; ++y)  // PFM rows run bottom to top
            for (int x = 0; x < W; ++x)
                for (int k = 0; k < 3; ++k)
                    rgb[((size_t)(H - 1 - y) * W + x) * 3 + k] = rt_h2f(c[((size_t)y * W + x) * 4 + k]);
        f << "PF\n" << W << " " << H << "\n-1.0\n";  // negative scale: little endian
        f.write(reinterpret_cast<const char*>(rgb.data()), (std::streamsize)(rgb.size() * 4));
    }
    return f ? RT_OK : RT_ERR_IO;
}

// Batch ray query through the persistent queue tracer (the RaySceneIntersect traversal of
// traverse.cuh:107-253 for caller rays): rays = n x (org.xyz, pad, dir.xyz, pad) floats,
// hits = n x (t, triangle index as int bits (-1: miss), u, v), iters = per-ray TraverseBvh
// iterations (optional), kernel_ms = the tracer kernel's HIP-event time (optional).
int rt_trace_rays(rt_context* ctx, const float* rays, uint32_t n, float* hits, uint32_t* iters, float* kernel_ms) {
    if (!ctx || (n > 0 && (!rays || !hits))) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_trace_rays before rt_init"; return RT_ERR_STATE; }
    FrameResources& fr = ctx->fr;
    if (n > fr.ws.cap) { ctx->err = "more rays than the queue capacity (width x strip rows x spp)"; return RT_ERR_ARG; }
    if (kernel_ms) *kernel_ms = 0.0f;
    if (n == 0) return RT_OK;
    std::vector<float4> o(n), d(n);
    for (uint32_t i = 0; i < n; ++i) {
        float tag;
        memcpy(&tag, &i, 4);  // the queue's pixel slot carries the ray index
        o[i] = make_float4(rays[8 * i], rays[8 * i + 1], rays[8 * i + 2], tag);
        d[i] = make_float4(rays[8 * i + 4], rays[8 * i + 5], rays[8 * i + 6], 0.0f);
    }
    PathTraceParams p = {};
    p.triPos = ctx->lbvh().triPos;
    p.triNrm = ctx->lbvh().triNrm;
    p.nodes = ctx->lbvh().nodes;
    p.tlasNodes = ctx->lbvh().tlasNodes;
    p.ws = fr.ws;
    bind_workspace(p.ws, fr.set[0], fr.set[0]);  // no shading list: the queue is traced only
    const PtWorkspace& ws = p.ws;
    p.ws.itersOut = iters ? reinterpret_cast<uint32_t*>(ws.pathL) : nullptr;  // pathL: per-frame scratch
    if (int rc = sync_streams(ctx)) return rc;  // the queue buffers are shared with in-flight frames
    HIP_TRY(ctx, hipMemcpyAsync(ws.q3.rayO, o.data(), (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ws.q3.rayD, d.data(), (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    fr.syncZeroed[0] = false;  // set 0's counter block is syncCount[0]
    HIP_TRY(ctx, hipMemsetAsync(ws.counters, 0, kWsCounterWords * sizeof(uint32_t), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ws.counters + kCntQ3, &n, 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    HIP_TRY(ctx, rtk_launch_trace_queue(&p, 3, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(hits, ws.hitRec, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
    if (iters) HIP_TRY(ctx, hipMemcpyAsync(iters, p.ws.itersOut, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (kernel_ms) HIP_TRY(ctx, hipEventElapsedTime(kernel_ms, ctx->ev0, ctx->ev1));
    return RT_OK;
}

// Device ray queries (trace_rays.hip): the same traversal for caller rays in device memory, enqueued
// on the context stream between whatever else the host enqueues there.  Unlike rt_trace_rays it
// drains nothing, keeps what a synchronous draw traced ahead, and uses none of the path tracer's
// workspace (the counter blocks, the queues, hitRec*, pathL, syncZeroed) nor the ray counter.
// Check order: NULL ctx / q, then the other argument checks, then the init state.

// what is wrong with a query's arguments, or null (rt_trace_rays_device, rt_trace_surfaces_device)
static const char* ray_query_fault(const rt_ray_query* q) {
    if (q->org_stride < 3u || q->dir_stride < 3u) return "strides are in floats and at least 3";
    if (q->n > RT_QUERY_MAX_RAYS) return "more rays than RT_QUERY_MAX_RAYS";
    if ((q->flags & ~RT_QUERY_ANY_HIT) != 0u) return "unknown flags";
    if (q->n > 0u && (!q->org || !q->dir || !q->hits)) return "org, dir and hits must not be NULL";
    if (((uintptr_t)q->hits & 15u) != 0) return "hits must be 16-byte aligned";
    if ((((uintptr_t)q->org | (uintptr_t)q->dir | (uintptr_t)q->iters) & 3u) != 0) return "org, dir and iters must be 4-byte aligned";
    return nullptr;
}

// the tracer of a query with n > 0 on LBVH set b, enqueued on s
static int enqueue_ray_trace(rt_context* ctx, const rt_ray_query* q, const BvhBufs& b, hipStream_t s) {
    RayQueryParams p;
    p.nodes = b.nodes;
    p.tlasNodes = b.tlasNodes;
    p.triPos = b.triPos;
    p.org = q->org;
    p.dir = q->dir;
    p.orgStride = q->org_stride;
    p.dirStride = q->dir_stride;
    p.n = q->n;
    p.hits = reinterpret_cast<float4*>(q->hits);
    p.iters = q->iters;
    p.fetch = ctx->queryFetch;
    HIP_TRY(ctx, hipMemsetAsync(ctx->queryFetch, 0, 512, s));
    // the queue tracers' grid policy (rt_frame_init: cus x tracePerCu, [tuning] tracePerCu)
    HIP_TRY(ctx, rtk_launch_trace_rays(&p, ctx->fr.ws.traceBlocks, (q->flags & RT_QUERY_ANY_HIT) != 0u, s));
    return RT_OK;
}

// The set a query read is held against the builds that would overwrite it, from this point of s on: a
// pipelined context's next build but one (rt_build_bvh waits for readDone), a synchronous draw's
// prebuild (prebuild_next_bvh)
static int hold_query_set(rt_context* ctx, BvhBufs& b, hipStream_t s) {
    if (ctx->postStream) {
        HIP_TRY(ctx, hipEventRecord(b.readDone, s));
        b.readInFlight = true;
    } else {
        HIP_TRY(ctx, hipEventRecord(b.queryDone, s));
        b.queryInFlight = true;
    }
    return RT_OK;
}

int rt_trace_rays_device(rt_context* ctx, const rt_ray_query* q) {
    if (!ctx || !q) return RT_ERR_ARG;
    if (const char* bad = ray_query_fault(q)) { ctx->err = std::string("rt_trace_rays_device: ") + bad; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = "rt_trace_rays_device before rt_init"; return RT_ERR_STATE; }
    hipStream_t s = ctx->stream;
    if (q->n > 0u) {
        if (q->ready_event) HIP_TRY(ctx, hipStreamWaitEvent(s, (hipEvent_t)q->ready_event, 0));
        if (int rc = wait_bvh(ctx)) return rc;  // the current set's build, wherever it ran
        BvhBufs& b = ctx->lbvh();
        if (int rc = enqueue_ray_trace(ctx, q, b, s)) return rc;
        if (int rc = hold_query_set(ctx, b, s)) return rc;
    }
    if (q->done_event) HIP_TRY(ctx, hipEventRecord((hipEvent_t)q->done_event, s));
    return RT_OK;
}

// Surface queries (surface_rays.hip): rt_trace_rays_device's tracer, or none (RT_SURFACE_FROM_HITS),
// and behind it on the context stream the dense surface pass over the records.  Everything the ray
// query leaves alone this leaves alone; dispTraced is not touched either, since a query never
// consumes the displacement a frame is still to apply.  Check order: NULL ctx / q, the ray query's
// argument checks, the surface query's own, then the init state.
int rt_trace_surfaces_device(rt_context* ctx, const rt_surface_query* q) {
    if (!ctx || !q) return RT_ERR_ARG;
    const rt_ray_query* r = &q->rays;
    const bool fromHits = (q->flags & RT_SURFACE_FROM_HITS) != 0u;
    const char* bad = ray_query_fault(r);
    if (!bad) {
        if ((q->flags & ~(RT_SURFACE_FROM_HITS | RT_SURFACE_MOTION)) != 0u) bad = "unknown surface flags";
        else if (r->n > 0u && !q->surface) bad = "surface must not be NULL";
        else if (r->n > 0u && ((uintptr_t)q->surface & 15u) != 0) bad = "surface must be 16-byte aligned";
        else if (fromHits && r->iters) bad = "RT_SURFACE_FROM_HITS traces nothing: iters must be NULL";
        else if (fromHits && (r->flags & RT_QUERY_ANY_HIT)) bad = "RT_SURFACE_FROM_HITS traces nothing: RT_QUERY_ANY_HIT must be clear";
    }
    if (bad) { ctx->err = std::string("rt_trace_surfaces_device: ") + bad; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = "rt_trace_surfaces_device before rt_init"; return RT_ERR_STATE; }
    hipStream_t s = ctx->stream;
    if (r->n > 0u) {
        if (r->ready_event) HIP_TRY(ctx, hipStreamWaitEvent(s, (hipEvent_t)r->ready_event, 0));
        if (int rc = wait_bvh(ctx)) return rc;
        BvhBufs& b = ctx->lbvh();
        if (!fromHits)
            if (int rc = enqueue_ray_trace(ctx, r, b, s)) return rc;
        RaySurfaceParams p;
        p.nodes = b.nodes;
        p.tlasNodes = b.tlasNodes;
        p.triPos = b.triPos;
        p.triNrm = b.triNrm;
        // the displacement the set's build recorded, whether or not a path trace has applied it
        p.triDisp = b.dispValid ? b.triDisp : nullptr;
        // the material table of a path trace enqueued now (fill_pt_params): the override wins over it
        p.materialOverride = ctx->materialOverride;
        p.triMat = ctx->materialOverride >= 0 ? nullptr : ctx->dTriMat;
        p.triCount = b.triCount;
        p.triCountPadded = b.triCountPadded;
        p.org = r->org;
        p.dir = r->dir;
        p.orgStride = r->org_stride;
        p.dirStride = r->dir_stride;
        p.n = r->n;
        p.hits = reinterpret_cast<const float4*>(r->hits);
        p.surface = reinterpret_cast<float4*>(q->surface);
        HIP_TRY(ctx, rtk_launch_ray_surface(&p, (q->flags & RT_SURFACE_MOTION) != 0u, s));
        if (int rc = hold_query_set(ctx, b, s)) return rc;  // behind the surface kernel: triDisp is the set's
        if (p.triMat && ctx->matPoolReady) {  // a later rt_set_triangle_materials_device writes behind this reader
            rt_context::MatTable& tab = ctx->matPool[ctx->matCur];
            HIP_TRY(ctx, hipEventRecord(tab.read, s));
            tab.readValid = true;
        }
    }
    if (r->done_event) HIP_TRY(ctx, hipEventRecord((hipEvent_t)r->done_event, s));
    return RT_OK;
}

// Closest-point queries (closest_points.hip): the nearest triangle of the current build for caller points
// in device memory, by the rule of closest_kernels.h.  Ordering and state are the ray query's: the
// context stream, behind ready_event and the current set's build, the set held against later builds, no
// host synchronisation, nothing of the path tracer's touched.  Check order: NULL ctx / q, then the
// other argument checks, then the init state.
static const char* closest_query_fault(const rt_closest_query* q) {
    if (q->stride < 3u) return "stride is in floats and at least 3";
    if (q->n > RT_QUERY_MAX_RAYS) return "more points than RT_QUERY_MAX_RAYS";
    if (!closest_distance_ok(q->max_distance)) return "max_distance must be >= 0 or +inf";
    if (q->n > 0u && (!q->points || !q->out)) return "points and out must not be NULL";
    if (q->n > 0u && ((uintptr_t)q->points & 3u) != 0) return "points must be 4-byte aligned";
    if (q->n > 0u && ((uintptr_t)q->out & 15u) != 0) return "out must be 16-byte aligned";
    return nullptr;
}

// the descent of a query with n > 0 on LBVH set b, enqueued on s
static int enqueue_closest(rt_context* ctx, const rt_closest_query* q, const BvhBufs& b, hipStream_t s) {
    ClosestParams p;
    p.nodes = b.nodes;
    p.tlasNodes = b.tlasNodes;
    p.triPos = b.triPos;
    p.reorder = b.reorder;
    p.triCount = b.triCount;
    p.batchCount = b.B;
    p.points = q->points;
    p.stride = q->stride;
    p.n = q->n;
    p.limit = q->max_distance * q->max_distance;  // fp32 (-ffp-contract=off): closest_limit
    p.stackCap = (uint32_t)ctx->closestStack;
    p.out = q->out;
    HIP_TRY(ctx, rtk_launch_closest_points(&p, s));
    return RT_OK;
}

int rt_closest_points_device(rt_context* ctx, const rt_closest_query* q) {
    if (!ctx || !q) return RT_ERR_ARG;
    if (const char* bad = closest_query_fault(q)) { ctx->err = std::string("rt_closest_points_device: ") + bad; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = "rt_closest_points_device before rt_init"; return RT_ERR_STATE; }
    hipStream_t s = ctx->stream;
    if (q->n > 0u) {
        if (q->ready_event) HIP_TRY(ctx, hipStreamWaitEvent(s, (hipEvent_t)q->ready_event, 0));
        if (int rc = wait_bvh(ctx)) return rc;  // the current set's build, wherever it ran
        BvhBufs& b = ctx->lbvh();
        if (b.B == 0u || b.triCount == 0u) { ctx->err = "rt_closest_points_device before the first rt_build_bvh"; return RT_ERR_STATE; }
        if (int rc = enqueue_closest(ctx, q, b, s)) return rc;
        if (int rc = hold_query_set(ctx, b, s)) return rc;
    }
    if (q->done_event) HIP_TRY(ctx, hipEventRecord((hipEvent_t)q->done_event, s));
    return RT_OK;
}

// Signed distance queries (sdf.hip): rt_closest_points_device's descent, or none
// (RT_DISTANCE_FROM_RECORDS), and behind it on the context stream the dense sign pass over the records,
// which reads the pseudo-normal table the current set's build wrote (rt_set_signed_distance).  Everything
// the closest query leaves alone this leaves alone.  Check order: NULL ctx / q, the closest query's
// argument checks, the distance query's own, then the init state and the table.
int rt_signed_distance_device(rt_context* ctx, const rt_distance_query* q) {
    if (!ctx || !q) return RT_ERR_ARG;
    const rt_closest_query* c = &q->closest;
    const char* bad = closest_query_fault(c);
    if (!bad) {
        if ((q->flags & ~RT_DISTANCE_FROM_RECORDS) != 0u) bad = "unknown flags";
        else if (c->n > 0u && !q->signed_out) bad = "signed_out must not be NULL";
        else if (c->n > 0u && ((uintptr_t)q->signed_out & 15u) != 0) bad = "signed_out must be 16-byte aligned";
    }
    if (bad) { ctx->err = std::string("rt_signed_distance_device: ") + bad; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = "rt_signed_distance_device before rt_init"; return RT_ERR_STATE; }
    // host state of the current set: its build was issued with or without a table, wherever it runs
    if (!ctx->lbvh().sdfBuilt) {
        ctx->err = "rt_signed_distance_device: the current build wrote no pseudo-normal table (rt_set_signed_distance, then a build)";
        return RT_ERR_STATE;
    }
    hipStream_t s = ctx->stream;
    if (c->n > 0u) {
        if (c->ready_event) HIP_TRY(ctx, hipStreamWaitEvent(s, (hipEvent_t)c->ready_event, 0));
        if (int rc = wait_bvh(ctx)) return rc;  // the current set's build and its table, wherever they ran
        BvhBufs& b = ctx->lbvh();
        if (b.B == 0u || b.triCount == 0u) { ctx->err = "rt_signed_distance_device before the first rt_build_bvh"; return RT_ERR_STATE; }
        if (!(q->flags & RT_DISTANCE_FROM_RECORDS))
            if (int rc = enqueue_closest(ctx, c, b, s)) return rc;
        SdfSignParams p;
        p.triPos = b.triPos;
        p.table = b.sdfTable;
        p.triCount = b.triCount;
        p.points = c->points;
        p.stride = c->stride;
        p.n = c->n;
        p.records = c->out;
        p.out = q->signed_out;
        HIP_TRY(ctx, rtk_launch_sdf_sign(&p, s));
        if (int rc = hold_query_set(ctx, b, s)) return rc;  // behind the sign pass: the table is the set's
    }
    if (c->done_event) HIP_TRY(ctx, hipEventRecord((hipEvent_t)c->done_event, s));
    return RT_OK;
}
