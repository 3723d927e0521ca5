// environment.hip — environment-map ingest for gfx950 (rt_set_environment*): a
// caller's image into the context's 512 x 256 equal-area environment table and its pdf, by the rule of
// env_kernels.h, which rt_environment_table compiles for the host.
//
//   k_env_table     TABLE layout: one thread per table texel
//   k_env_rows      LATLONG: every upper source row's table row and weight, and each table row's run of
//                   source rows (one workgroup; integer min / max in LDS)
//   k_env_row_sums  LATLONG: one workgroup row per upper source row; a thread sums the source columns of
//                   one table column in ascending order.  A wave reads one contiguous stretch of the
//                   row; halves are read as packed pairs (8 B per texel) and converted in pairs
//   k_env_gather    LATLONG: one thread per table texel over its run of rows, ascending; the 256 threads
//                   of a workgroup share the table row, so the loop is uniform, and the long zenith runs
//                   (about Hs / 36 rows) cost those waves 16-byte reads of sums the whole device
//                   produced in parallel, not a serial walk over the source
// A gather throughout: no atomics on floats, every sum in the order the rule defines.
#include "env_kernels.h"

namespace {

typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));

struct Rgb { float r, g, b; };

// texel i of the source, sanitised
template <int kFormat>
__device__ __forceinline__ Rgb env_load(const void* texels, size_t i) {
    Rgb o;
    if (kFormat == 0) {
        const float4 v = reinterpret_cast<const float4*>(texels)[i];
        o.r = env_sanitize(v.x);
        o.g = env_sanitize(v.y);
        o.b = env_sanitize(v.z);
    } else {
        const uint2 v = reinterpret_cast<const uint2*>(texels)[i];
        const float2_t rg = __builtin_convertvector(__builtin_bit_cast(half2_t, v.x), float2_t);
        const float2_t ba = __builtin_convertvector(__builtin_bit_cast(half2_t, v.y), float2_t);
        o.r = env_sanitize(rg.x);
        o.g = env_sanitize(rg.y);
        o.b = env_sanitize(ba.x);
    }
    return o;
}

__device__ __forceinline__ void env_store(float4* table, float* pdf, uint32_t i, float r, float g, float b, float scale) {
    const float x = env_final(r, scale), y = env_final(g, scale), z = env_final(b, scale);
    table[i] = make_float4(x, y, z, 0.0f);
    pdf[i] = env_pdf(x, y, z);
}

}  // namespace

template <int kFormat>
__global__ __launch_bounds__(256) void k_env_table(const void* texels, float scale, float4* table, float* pdf) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= kEnvSize) return;
    const Rgb c = env_load<kFormat>(texels, i);
    env_store(table, pdf, i, c.r, c.g, c.b, scale);
}

__global__ __launch_bounds__(1024) void k_env_rows(uint32_t Hs, int* rowY, float* rowW, uint32_t* runs) {
    __shared__ uint32_t lo[kEnvH], hi[kEnvH];
    const uint32_t t = threadIdx.x, Hu = Hs / 2u;
    if (t < kEnvH) {
        lo[t] = 0xFFFFFFFFu;
        hi[t] = 0u;
    }
    __syncthreads();
    for (uint32_t r = t; r < Hu && r < kEnvMaxRows; r += 1024u) {
        const float theta = env_row_theta(r, Hs);
        const int y = env_row_cell(theta);  // in [0, 255]
        rowY[r] = y;
        rowW[r] = env_row_weight(theta);
        atomicMin(&lo[y], r);
        atomicMax(&hi[y], r + 1u);
    }
    __syncthreads();
    if (t < kEnvH) {
        const bool empty = hi[t] == 0u;
        const uint32_t near = env_nearest_row(t, Hs);  // in [0, Hu)
        runs[t] = empty ? near : lo[t];
        runs[kEnvH + t] = empty ? near + 1u : hi[t];
        runs[2u * kEnvH + t] = empty ? 1u : 0u;
    }
}

template <int kFormat>
__global__ __launch_bounds__(256) void k_env_row_sums(const void* texels, uint32_t Ws, uint32_t Hu, float4* rowSums) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, r = blockIdx.y;
    if (x >= kEnvW || r >= Hu) return;
    uint32_t c0, n;
    env_col_range(x, Ws, c0, n);  // c0 + n <= Ws
    const size_t row = (size_t)r * Ws;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    for (uint32_t k = 0; k < n; ++k) {
        const Rgb c = env_load<kFormat>(texels, row + c0 + k);
        sr = sr + c.r;
        sg = sg + c.g;
        sb = sb + c.b;
    }
    rowSums[(size_t)r * kEnvW + x] = make_float4(sr, sg, sb, 0.0f);
}

__global__ __launch_bounds__(256) void k_env_gather(const float4* rowSums, const int* rowY, const float* rowW,
                                                    const uint32_t* runs, uint32_t Ws, uint32_t Hu, float scale,
                                                    float4* table, float* pdf) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= kEnvSize) return;
    const uint32_t x = i % kEnvW, y = i / kEnvW;  // one y per workgroup
    const uint32_t r0 = runs[y], r1 = min(runs[kEnvH + y], Hu);
    const bool nearest = runs[2u * kEnvH + y] != 0u;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, ws = 0.0f;
    for (uint32_t r = r0; r < r1; ++r) {
        if (!nearest && rowY[r] != (int)y) continue;  // a run is the rows between a cell's first and last
        const float w = nearest ? 1.0f : rowW[r];
        const float4 s = rowSums[(size_t)r * kEnvW + x];
        ar = ar + w * s.x;
        ag = ag + w * s.y;
        ab = ab + w * s.z;
        ws = ws + w;
    }
    uint32_t c0, n;
    env_col_range(x, Ws, c0, n);
    const float d = (float)n * ws;
    env_store(table, pdf, i, ar / d, ag / d, ab / d, scale);
}

extern "C" hipError_t rtk_launch_env_ingest(const EnvIngestParams* p, hipStream_t stream) {
    if (!p->texels || !p->table || !p->pdf || p->format > 1u || p->layout > 1u) return hipErrorInvalidValue;
    if (p->layout == 0u) {  // TABLE
        if (p->width != kEnvW || p->height != kEnvH) return hipErrorInvalidValue;
        if (p->format == 0u)
            hipLaunchKernelGGL(k_env_table<0>, dim3(kEnvSize / 256), dim3(256), 0, stream, p->texels, p->scale, p->table, p->pdf);
        else
            hipLaunchKernelGGL(k_env_table<1>, dim3(kEnvSize / 256), dim3(256), 0, stream, p->texels, p->scale, p->table, p->pdf);
        return hipGetLastError();
    }
    const uint32_t Ws = p->width, Hs = p->height, Hu = Hs / 2u;
    if (Ws < kEnvMinW || Hs < kEnvMinH || Ws > kEnvMaxDim || Hs > kEnvMaxDim) return hipErrorInvalidValue;
    if (!p->rowY || !p->rowW || !p->runs || !p->rowSums || p->rowSumsRows < Hu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_env_rows, dim3(1), dim3(1024), 0, stream, Hs, p->rowY, p->rowW, p->runs);
    if (p->format == 0u)
        hipLaunchKernelGGL(k_env_row_sums<0>, dim3(kEnvW / 256, Hu), dim3(256), 0, stream, p->texels, Ws, Hu, p->rowSums);
    else
        hipLaunchKernelGGL(k_env_row_sums<1>, dim3(kEnvW / 256, Hu), dim3(256), 0, stream, p->texels, Ws, Hu, p->rowSums);
    hipLaunchKernelGGL(k_env_gather, dim3(kEnvSize / 256), dim3(256), 0, stream, (const float4*)p->rowSums,
                       (const int*)p->rowY, (const float*)p->rowW, (const uint32_t*)p->runs, Ws, Hu, p->scale, p->table,
                       p->pdf);
    return hipGetLastError();
}
