// emitters.hip — the emitter list of one LBVH build for gfx950 (rt_set_emitter_sampling, DESIGN.md
// §4.1.6): the emissive triangles of the build in ascending order, their weights and the weights' CDF.
//
//   k_em_weigh     one lane per triangle: the id the path tracer would read for it (update_material:
//                  the override, else the triangle's entry, else 3), its table record, and for an
//                  EMISSIVE one the weight (emitter_weight over the build's triangle record); 0 for every
//                  other triangle and past triCount.  The workgroup counts its emitters (ballots).
//   k_em_offsets   one workgroup: the exclusive scan of the <= 4096 workgroup counts, the list's length
//   k_em_scatter   one lane per triangle: an emitter's slot is its workgroup's offset plus its rank
//                  among the workgroup's emitters, so the list ascends; index and weight go to the slot
//   Scan           the reference scan (rtk_launch_scan, block 256) of the zero-padded weights
//   k_em_total     one thread: cdf[count - 1] beside the count
//
// Every step is a launch of its own on the build's stream: no workgroup waits for another and nothing
// spins.  Slots come from integer counts only, so the list, and with it the CDF's bits, do not depend
// on the order anything ran in.
#include "emitter_kernels.h"
#include "frame_kernels.h"
#include "rt_device.h"
#include "shade.h"

using namespace rtd;

namespace {

__global__ __launch_bounds__(256) void k_em_weigh(EmitterListParams P) {
    __shared__ uint32_t waveCount[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;  // < cdfLen: the grid is cdfLen / 256
    float w = 0.0f;
    if (t < P.triCount) {
        const int id = P.materialOverride >= 0 ? P.materialOverride : P.triMat ? (int)P.triMat[t] : 3;
        const float4 m0 = P.matTable[(id & 255) * kMatRecVecs];
        if ((int)(__float_as_uint(m0.w) & 0xFFu) == EMISSIVE) {
            const float4 m2 = P.matTable[(id & 255) * kMatRecVecs + 2];
            const float4 a = P.triPos[4u * t], b = P.triPos[4u * t + 1u], c = P.triPos[4u * t + 2u];
            const float xyz[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
            const float e[3] = {m2.x, m2.y, m2.z};
            w = emitter_weight(xyz, e);
            if (!(w > 0.0f)) w = 0.0f;  // a degenerate triangle, a black entry, NaN: no emitter
        }
    }
    P.triWeight[t] = w;
    const unsigned long long m = __ballot(w > 0.0f);
    if ((threadIdx.x & 63u) == 0u) waveCount[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) P.blockCount[blockIdx.x] = waveCount[0] + waveCount[1] + waveCount[2] + waveCount[3];
}

// blocks <= 4096: four counts per thread, a Hillis-Steele scan of the 1024 partial sums in LDS
__global__ __launch_bounds__(1024) void k_em_offsets(uint32_t* blockCount, uint32_t blocks, uint32_t* header) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x;
    uint32_t c[4], sum = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t b = 4u * t + j;
        c[j] = b < blocks ? blockCount[b] : 0u;
        sum += c[j];
    }
    part[t] = sum;
    __syncthreads();
    for (uint32_t o = 1u; o < 1024u; o <<= 1) {
        const uint32_t add = t >= o ? part[t - o] : 0u;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;  // exclusive
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t b = 4u * t + j;
        if (b < blocks) blockCount[b] = run;
        run += c[j];
    }
    if (t == 1023u) header[kEmCount] = part[1023];
}

__global__ __launch_bounds__(256) void k_em_scatter(EmitterListParams P) {
    __shared__ uint32_t waveCount[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const float w = P.triWeight[t];
    const bool emits = w > 0.0f;  // only below triCount (k_em_weigh)
    const unsigned long long m = __ballot(emits);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) waveCount[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!emits) return;
    uint32_t slot = P.blockCount[blockIdx.x] + lane_rank(m);
    for (uint32_t k = 0; k < wave; ++k) slot += waveCount[k];
    // slot < count <= triCount: the offsets are the counts of the same weights
    P.tris[slot] = t;
    P.weights[slot] = w;
}

__global__ void k_em_total(const float* cdf, uint32_t* header) {
    const uint32_t n = header[kEmCount];
    header[kEmTotal] = n ? __float_as_uint(cdf[n - 1u]) : 0u;
}

}  // namespace

extern "C" hipError_t rtk_launch_emitter_list(const EmitterListParams* p, hipStream_t stream) {
    if (!p->triPos || !p->matTable || !p->triWeight || !p->blockCount || !p->tris || !p->weights || !p->cdf ||
        !p->scanSums || !p->header || p->triCount == 0u || p->triCount > kEmMaxTris ||
        p->cdfLen != emitter_cdf_len(p->triCount))
        return hipErrorInvalidValue;
    const uint32_t blocks = p->cdfLen / 256u;  // a power of two <= 4096
    hipError_t e = hipMemsetAsync(p->weights, 0, (size_t)p->cdfLen * sizeof(float), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_em_weigh, dim3(blocks), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(k_em_offsets, dim3(1), dim3(1024), 0, stream, p->blockCount, blocks, p->header);
    hipLaunchKernelGGL(k_em_scatter, dim3(blocks), dim3(256), 0, stream, *p);
    if ((e = rtk_launch_scan(p->weights, p->cdf, p->scanSums, (int)p->cdfLen, (int)kEmScanBlock, stream)) != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_em_total, dim3(1), dim3(1), 0, stream, (const float*)p->cdf, p->header);
    return hipGetLastError();
}
