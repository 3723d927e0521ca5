// materials.hip — the stream-ordered material table for gfx950 (rt_set_triangle_materials_device):
// a new table from the previous one and the caller's range of ids.
//
//   k_mat_set      one lane per 16 bytes of the new table: the previous table's 16 bytes (3 without
//                  one), the caller's bytes that fall into them merged in (byte loads: the source has
//                  no alignment and `first` is arbitrary, so the head and tail lanes take the same
//                  path as every other), every id classified (mat_class_of) and one of an undeclared
//                  class replaced by 3, the bytes from triCount up 3, one 16-byte store.  The
//                  workgroup counts the ids below triCount into 256 LDS bins (integer atomics: only
//                  their totals are used) and adds the non-zero bins to the table's census; the
//                  replaced ids are counted with one integer atomic per wave that saw one.
//   k_mat_report   one thread: the count, if any, to the host's status word, and the counter re-armed
//
// Every step is a launch of its own on one stream: no workgroup waits for another, nothing spins, no
// result depends on the order atomics land in, and there is no float arithmetic.
#include "bvh_kernels.h"
#include "mat_kernels.h"
#include "rt_device.h"

using namespace rtd;

__global__ __launch_bounds__(256) void k_mat_set(MatSetParams P) {
    __shared__ uint32_t bins[256];
    const uint32_t t = threadIdx.x;
    bins[t] = 0u;
    __syncthreads();
    const uint32_t base = (blockIdx.x * 256u + t) * 16u;  // capBytes <= 2^32 - 16: no wrap in the grid
    const bool valid = base < P.capBytes;
    uint32_t w[4] = {kMatDefaultId * 0x01010101u, kMatDefaultId * 0x01010101u, kMatDefaultId * 0x01010101u,
                     kMatDefaultId * 0x01010101u};
    if (valid && P.prev) {
        const uint4 v = *reinterpret_cast<const uint4*>(P.prev + base);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
    }
    uint32_t bad = 0u;  // this wave's replaced ids (uniform: every lane takes every ballot)
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t i = base + j, sh = 8u * (j & 3u);
        uint32_t id = (w[j >> 2] >> sh) & 0xFFu;
        const uint32_t k = i - P.first;  // wraps below first: then not < count either (count <= triCount)
        const bool live = valid && i < P.triCount;
        if (live && i >= P.first && k < P.count) id = P.src[k];
        const bool undeclared = live && (mat_class_of(id) & ~P.classes) != 0u;
        if (!live || undeclared) id = kMatDefaultId;
        if (live) atomicAdd(&bins[id], 1u);
        w[j >> 2] = (w[j >> 2] & ~(0xFFu << sh)) | (id << sh);
        bad += (uint32_t)__popcll(__ballot(undeclared));
    }
    if (valid) *reinterpret_cast<uint4*>(P.dst + base) = make_uint4(w[0], w[1], w[2], w[3]);
    if ((t & 63u) == 0u && bad != 0u) atomicAdd(P.badCount, bad);
    __syncthreads();
    const uint32_t n = bins[t];
    if (n) atomicAdd(P.census + t, n);
}

__global__ void k_mat_report(uint32_t* badCount, uint32_t* status) {
    const uint32_t c = *badCount;
    if (c) {
        report_status(status, kStatusMatUndeclared, c);
        *badCount = 0u;
    }
}

extern "C" hipError_t rtk_launch_mat_set(const MatSetParams* p, hipStream_t stream) {
    if (!p->src || !p->dst || p->dst == p->prev || p->capBytes == 0u || (p->capBytes & 15u) != 0u ||
        p->capBytes > 0xFFFFF000u || (((uintptr_t)p->dst | (uintptr_t)p->prev) & 15u) != 0u || p->count == 0u ||
        p->triCount > p->capBytes || (uint64_t)p->first + p->count > (uint64_t)p->triCount)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(p->census, 0, 256 * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const uint32_t lanes = p->capBytes / 16u;
    hipLaunchKernelGGL(k_mat_set, dim3((lanes + 255u) / 256u), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(k_mat_report, dim3(1), dim3(1), 0, stream, p->badCount, p->status);
    return hipGetLastError();
}
