// environment.cpp — environment maps behind the C-ABI: the rule compiled for the
// host (rt_environment_table) and the setters.  The table an image gives is kept once per context
// (envTable / envPdf); generating a sky set copies it where k_sky would run (frame.cpp generate_sky).
#include <cmath>
#include <vector>

#include "context.h"
#include "env_kernels.h"

namespace {

// the argument checks every entry point shares, in the documented order; null: fine
const char* env_check(const rt_environment* e, bool device) {
    if (!e->texels) return "texels must not be NULL";
    if (e->format != RT_ENV_FORMAT_F32X4 && e->format != RT_ENV_FORMAT_F16X4) return "unknown format";
    if (e->layout != RT_ENV_LAYOUT_TABLE && e->layout != RT_ENV_LAYOUT_LATLONG) return "unknown layout";
    if (e->layout == RT_ENV_LAYOUT_TABLE) {
        if (e->width != kEnvW || e->height != kEnvH) return "the TABLE layout is 512 x 256";
    } else if (e->width < kEnvMinW || e->height < kEnvMinH || e->width > kEnvMaxDim || e->height > kEnvMaxDim) {
        return "a LATLONG image is 4..16384 wide and 2..16384 high";
    }
    if (!std::isfinite(e->scale) || !(e->scale > 0.0f)) return "scale must be finite and positive";
    if (device && ((uintptr_t)e->texels & (env_texel_bytes(e->format) - 1u)) != 0u)
        return "texels must be 16-byte (F32X4) or 8-byte (F16X4) aligned";
    return nullptr;
}

// the rows of the image the rule reads: all of a table, the ones above the horizon of a LATLONG image
uint32_t env_rows_read(const rt_environment* e) { return e->layout == RT_ENV_LAYOUT_TABLE ? e->height : e->height / 2u; }

// texel (r, c) of a host image, sanitised
void host_texel(const rt_environment* e, uint32_t r, uint32_t c, float* rgb) {
    const size_t i = (size_t)r * e->width + c;
    if (e->format == RT_ENV_FORMAT_F32X4) {
        const float* t = (const float*)e->texels + i * 4;
        for (int k = 0; k < 3; ++k) rgb[k] = env_sanitize(t[k]);
    } else {
        const uint16_t* t = (const uint16_t*)e->texels + i * 4;
        for (int k = 0; k < 3; ++k) rgb[k] = env_sanitize(env_half_bits(t[k]));
    }
}

void host_store(float* table, float* pdf, uint32_t i, const float* v, float scale) {
    const float x = env_final(v[0], scale), y = env_final(v[1], scale), z = env_final(v[2], scale);
    table[4 * (size_t)i] = x;
    table[4 * (size_t)i + 1] = y;
    table[4 * (size_t)i + 2] = z;
    table[4 * (size_t)i + 3] = 0.0f;
    pdf[i] = env_pdf(x, y, z);
}

// the context's environment table, the ingest's scratch, and row sums for `rows` upper rows.  Buffers
// are never freed before rt_destroy: an ingest in flight may still use the smaller row-sum buffer.
int ensure_env_buffers(rt_context* ctx, uint32_t rows) {
    RT_TRY(dalloc_once(ctx, ctx->envTable, (size_t)kEnvSize * 16));
    RT_TRY(dalloc_once(ctx, ctx->envPdf, (size_t)kEnvSize * 4));
    RT_TRY(dalloc_once(ctx, ctx->envRowY, (size_t)kEnvMaxRows * 4));
    RT_TRY(dalloc_once(ctx, ctx->envRowW, (size_t)kEnvMaxRows * 4));
    RT_TRY(dalloc_once(ctx, ctx->envRuns, (size_t)3 * kEnvH * 4));
    if (rows > ctx->envRowSumsRows) {
        float4* p = nullptr;
        RT_TRY(dalloc(ctx, &p, (size_t)rows * kEnvW * 16));
        ctx->envRowSums = p;
        ctx->envRowSumsRows = rows;
    }
    return RT_OK;
}

EnvIngestParams ingest_params(const rt_context* ctx, const rt_environment* e, const void* texels) {
    EnvIngestParams p;
    p.texels = texels;
    p.width = e->width;
    p.height = e->height;
    p.format = e->format;
    p.layout = e->layout;
    p.scale = e->scale;
    p.table = ctx->envTable;
    p.pdf = ctx->envPdf;
    p.rowY = ctx->envRowY;
    p.rowW = ctx->envRowW;
    p.runs = ctx->envRuns;
    p.rowSums = ctx->envRowSums;
    p.rowSumsRows = (uint32_t)ctx->envRowSumsRows;
    return p;
}

}  // namespace

extern "C" {

int rt_environment_table(const rt_environment* e, float* table, float* pdf) {
    if (!e || !table || !pdf || env_check(e, false)) return RT_ERR_ARG;
    float v[3];
    if (e->layout == RT_ENV_LAYOUT_TABLE) {
        for (uint32_t i = 0; i < kEnvSize; ++i) {
            host_texel(e, i / kEnvW, i % kEnvW, v);
            host_store(table, pdf, i, v, e->scale);
        }
        return RT_OK;
    }
    const uint32_t Ws = e->width, Hs = e->height, Hu = Hs / 2u;
    // membership by texel centres: the columns each table column owns, or its single nearest one
    std::vector<uint32_t> owned(kEnvW, 0u), nearestCol(kEnvW);
    for (uint32_t c = 0; c < Ws; ++c) ++owned[env_col_cell(c, Ws)];
    for (uint32_t x = 0; x < kEnvW; ++x) nearestCol[x] = ((2u * x + 1u) * Ws) / 1024u;
    std::vector<float> s((size_t)kEnvW * 3), acc((size_t)kEnvSize * 3, 0.0f), wsum(kEnvH, 0.0f);
    std::vector<uint32_t> rowsOwned(kEnvH, 0u);
    // s_r: row r summed over each table column's source columns, ascending
    auto row_sums = [&](uint32_t r) {
        std::fill(s.begin(), s.end(), 0.0f);
        for (uint32_t c = 0; c < Ws; ++c) {
            host_texel(e, r, c, v);
            float* d = s.data() + (size_t)env_col_cell(c, Ws) * 3;
            for (int k = 0; k < 3; ++k) d[k] = d[k] + v[k];
        }
        for (uint32_t x = 0; x < kEnvW; ++x)
            if (!owned[x]) {
                host_texel(e, r, nearestCol[x], v);
                for (int k = 0; k < 3; ++k) s[(size_t)x * 3 + k] = 0.0f + v[k];
            }
    };
    auto add_row = [&](uint32_t y, float w) {
        float* a = acc.data() + (size_t)y * kEnvW * 3;
        for (size_t k = 0; k < (size_t)kEnvW * 3; ++k) a[k] = a[k] + w * s[k];
        wsum[y] = wsum[y] + w;
    };
    for (uint32_t r = 0; r < Hu; ++r) {  // rows ascending
        const float theta = env_row_theta(r, Hs);
        const uint32_t y = (uint32_t)env_row_cell(theta);
        row_sums(r);
        add_row(y, env_row_weight(theta));
        ++rowsOwned[y];
    }
    for (uint32_t y = 0; y < kEnvH; ++y) {
        if (!rowsOwned[y]) {  // the single nearest row, weight 1
            row_sums(env_nearest_row(y, Hs));
            add_row(y, 1.0f);
        }
        for (uint32_t x = 0; x < kEnvW; ++x) {
            const float d = (float)(owned[x] ? owned[x] : 1u) * wsum[y];
            const float* a = acc.data() + ((size_t)y * kEnvW + x) * 3;
            const float m[3] = {a[0] / d, a[1] / d, a[2] / d};
            host_store(table, pdf, y * kEnvW + x, m, e->scale);
        }
    }
    return RT_OK;
}

int rt_get_environment(const rt_context* ctx, int* active) {
    if (!ctx || !active) return RT_ERR_ARG;
    *active = ctx->envActive ? 1 : 0;
    return RT_OK;
}

int rt_set_environment(rt_context* ctx, const rt_environment* e) {
    if (!ctx || !e) return RT_ERR_ARG;
    if (const char* bad = env_check(e, false)) { ctx->err = std::string("rt_set_environment: ") + bad; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = "rt_set_environment before rt_init"; return RT_ERR_STATE; }
    RT_TRY(sync_streams(ctx, false));  // frames in flight may be reading the table; drops what was traced ahead
    const uint32_t rows = env_rows_read(e);
    RT_TRY(ensure_env_buffers(ctx, e->layout == RT_ENV_LAYOUT_LATLONG ? rows : 0u));
    const size_t bytes = (size_t)rows * e->width * env_texel_bytes(e->format);
    if (bytes > ctx->envStageBytes) {  // the streams are idle: the old staging has no reader
        if (ctx->envStage) HIP_TRY(ctx, hipFree(ctx->envStage));
        ctx->envStage = nullptr;
        ctx->envStageBytes = 0;
        HIP_TRY(ctx, hipMalloc(&ctx->envStage, bytes));
        ctx->envStageBytes = bytes;
    }
    HIP_TRY(ctx, hipMemcpy(ctx->envStage, e->texels, bytes, hipMemcpyHostToDevice));
    const EnvIngestParams p = ingest_params(ctx, e, ctx->envStage);
    HIP_TRY(ctx, rtk_launch_env_ingest(&p, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // whichever stream generates the next sky set reads the table
    ctx->envActive = true;
    return rt_regenerate_sky(ctx);
}

// The stream-ordered set.  The ingest and the generation of the next sky set run on the sky stream,
// behind the source's ready event (or the context stream's work so far) and, by stream order, behind
// the last generation that read the environment table; the context stream then waits for both.
int rt_set_environment_device(rt_context* ctx, const rt_environment* e) {
    if (!ctx || !e) return RT_ERR_ARG;
    if (const char* bad = env_check(e, true)) { ctx->err = std::string("rt_set_environment_device: ") + bad; return RT_ERR_ARG; }
    if (!ctx->inited) { ctx->err = "rt_set_environment_device before rt_init"; return RT_ERR_STATE; }
    if (ctx->skySets < 2) {
        ctx->err = "rt_set_environment_device needs [scene] skySets >= 2 (one set is rewritten in place, behind host waits)";
        return RT_ERR_STATE;
    }
    RT_TRY(ensure_env_buffers(ctx, e->layout == RT_ENV_LAYOUT_LATLONG ? env_rows_read(e) : 0u));
    for (hipEvent_t* ev : {&ctx->envSrc, &ctx->envDone}) RT_TRY(rt_event(ctx, *ev));
    hipStream_t s = sky_stream(ctx);
    if (e->ready_event) {
        HIP_TRY(ctx, hipStreamWaitEvent(s, (hipEvent_t)e->ready_event, 0));
    } else if (s != ctx->stream) {
        HIP_TRY(ctx, hipEventRecord(ctx->envSrc, ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->envSrc, 0));
    }
    const EnvIngestParams p = ingest_params(ctx, e, e->texels);
    HIP_TRY(ctx, rtk_launch_env_ingest(&p, s));
    ctx->envActive = true;
    const int rc = rt_regenerate_sky(ctx);  // the next sky set, on the same stream
    // the caller's later work on the context stream follows the read of its buffer
    HIP_TRY(ctx, hipEventRecord(ctx->envDone, s));
    if (s != ctx->stream) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->envDone, 0));
    return rc;
}

int rt_reset_environment(rt_context* ctx) {
    if (!ctx) return RT_ERR_ARG;
    if (!ctx->inited) { ctx->err = "rt_reset_environment before rt_init"; return RT_ERR_STATE; }
    RT_TRY(sync_streams(ctx, false));
    if (!ctx->envActive) return RT_OK;
    ctx->envActive = false;
    return rt_regenerate_sky(ctx);
}

}  // extern "C"
