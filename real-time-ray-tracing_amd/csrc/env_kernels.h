// env_kernels.h — environment maps (rt_set_environment): the rule that turns a
// caller's image into the 512 x 256 equal-area sky table, shared by the host (rt_environment_table,
// environment.cpp) and the ingest kernels (environment.hip), and the kernels' launch interface.
//
// The rule is plain fp32, one rounding per operation (every translation unit is built with
// -ffp-contract=off) over rtmath.h's transcendentals, so the host function, which compiles these very
// functions, gives the kernels' bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtmath.h"

constexpr uint32_t kEnvW = 512, kEnvH = 256, kEnvSize = kEnvW * kEnvH;  // the sky table (kSkyW x kSkyH)
constexpr uint32_t kEnvMinW = 4, kEnvMinH = 2, kEnvMaxDim = 16384;       // LATLONG source limits
constexpr uint32_t kEnvMaxRows = kEnvMaxDim / 2;                         // upper rows of the tallest source
constexpr float kEnvMaxValue = 65504.0f;                                 // the largest half: what the G-buffers hold
constexpr float kEnvPi = 3.1415926535897932384626422832795028841971f;

// a half's bits as the float of the same value (exact: subnormals, infinities and NaNs included)
RT_HD float env_half_bits(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 0x3FFu;
    uint32_t bits;
    if (ex == 31u) bits = sign | 0x7F800000u | (man << 13);
    else if (ex != 0u) bits = sign | ((ex + 112u) << 23) | (man << 13);
    else {
        // man * 2^-24: the conversion and the product by a power of two are exact
        const float f = (float)man * 5.9604644775390625e-8f;
        uint32_t fb;
        __builtin_memcpy(&fb, &f, 4);
        bits = sign | fb;
    }
    float r;
    __builtin_memcpy(&r, &bits, 4);
    return r;
}

// a source value: NaN, negatives and -0 count as 0, everything above the largest half as that
RT_HD float env_sanitize(float x) { return (x == x && x > 0.0f) ? (x < kEnvMaxValue ? x : kEnvMaxValue) : 0.0f; }

// the table's value from a cell's mean
RT_HD float env_final(float v, float scale) {
    const float s = v * scale;
    return s < kEnvMaxValue ? s : kEnvMaxValue;
}

// dot(c, (0.3, 0.6, 0.1)) as k_sky evaluates it (rt_device.h inner3)
RT_HD float env_pdf(float a, float c, float e) {
    const float b = 0.3f, d = 0.6f, f = 0.1f;
    const float ef = e * f, efe = __builtin_fmaf(e, f, -ef);
    const float cd = c * d, cde = __builtin_fmaf(c, d, -cd);
    const float s2 = cd + ef, dl2 = s2 - cd, s2e = (cd - (s2 - dl2)) + (ef - dl2);
    const float tpv = s2, tpe = cde + (efe + s2e);
    const float ab = a * b, abe = __builtin_fmaf(a, b, -ab);
    const float s1 = ab + tpv, dl1 = s1 - ab, s1e = (ab - (s1 - dl1)) + (tpv - dl1);
    const float rv = s1, re = abe + (tpe + s1e);
    return rv + re;
}

// ---- LATLONG rows: row r of Hs has polar angle theta_r; the rows with 2 r + 1 < Hs (Hs / 2 of them)
// are read.  Row r belongs to table row env_row_cell(theta_r) with weight env_row_weight(theta_r).
RT_HD float env_row_theta(uint32_t r, uint32_t Hs) { return (kEnvPi * (float)(2u * r + 1u)) / (float)(2u * Hs); }
RT_HD int env_row_cell(float theta) {
    const int y = (int)(rt_cosf(theta) * 256.0f);
    return y > 255 ? 255 : (y < 0 ? 0 : y);  // theta < pi / 2: the lower guard is never taken
}
RT_HD float env_row_weight(float theta) { return rt_sinf(theta); }
// the single source row of a table row that owns none, taken with weight 1
RT_HD uint32_t env_nearest_row(uint32_t y, uint32_t Hs) {
    const int r = (int)((rt_acosf(((float)y + 0.5f) / 256.0f) * (float)Hs) / kEnvPi);
    const int last = (int)(Hs / 2u) - 1;
    return (uint32_t)(r > last ? last : (r < 0 ? 0 : r));
}

// ---- LATLONG columns: column c of Ws belongs to table column env_col_cell(c, Ws)
RT_HD uint32_t env_col_cell(uint32_t c, uint32_t Ws) { return ((2u * c + 1u) * 256u) / Ws; }
// the first source column whose cell is >= x (the cells ascend with c): the least c with
// (2 c + 1) * 256 >= x * Ws; x = 512 gives Ws
RT_HD uint32_t env_col_first(uint32_t x, uint32_t Ws) {
    const uint32_t t = x * Ws;
    return t <= 256u ? 0u : (t - 256u + 511u) / 512u;
}
// the columns [c0, c0 + n) table column x sums, n >= 1: the ones it owns, or the single nearest one
RT_HD void env_col_range(uint32_t x, uint32_t Ws, uint32_t& c0, uint32_t& n) {
    c0 = env_col_first(x, Ws);
    n = env_col_first(x + 1u, Ws) - c0;
    if (n == 0u) {
        c0 = ((2u * x + 1u) * Ws) / 1024u;
        n = 1u;
    }
}

inline size_t env_texel_bytes(uint32_t format) { return format == 0u ? 16u : 8u; }  // RT_ENV_FORMAT_*

// One ingest (environment.hip): the image into the context's environment table and pdf.  A LATLONG
// source goes through three kernels: the rows' cells and weights (rowY, rowW) with each table row's run
// of source rows (runs: [0, 256) first row, [256, 512) one past the last, [512, 768) 1 for a table row
// that owns none, whose run is its nearest row), every upper row's sums over each table column's
// source columns (rowSums, 512 float4 per row), and the gather of each table cell over its run.
struct EnvIngestParams {
    const void* texels;   // device memory, width x height texels of `format`
    uint32_t width, height, format, layout;
    float scale;
    float4* table;        // out [kEnvSize]
    float* pdf;           // out [kEnvSize]
    int* rowY;            // scratch [kEnvMaxRows]
    float* rowW;          // scratch [kEnvMaxRows]
    uint32_t* runs;       // scratch [3 * kEnvH]
    float4* rowSums;      // scratch [rowSumsRows * kEnvW], rowSumsRows >= height / 2
    uint32_t rowSumsRows;
};
extern "C" hipError_t rtk_launch_env_ingest(const EnvIngestParams* p, hipStream_t stream);
