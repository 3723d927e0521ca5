// skin.hip — linear-blend skinning for gfx950 (rt_pose_skin / rt_pose_skin_device): one
// kernel on the update stream ahead of the whole-mesh vertex update (geometry.hip), which reads the
// positions it writes.
//
//   k_skin_vertices   one thread per vertex: the rest position (three floats), the four joints (one
//                     8-byte load), the four weights (one 16-byte load), per non-zero influence the three
//                     rows of its joint's matrix (16-byte loads) and three stores
//
// The rule is skin_kernels.h's skin_vertex, the text rt_skin_vertices compiles for the host.  The
// per-vertex arrays are read once, consecutive threads' records adjoining; the matrix table (at most
// 192 KB, more than a workgroup's LDS) is shared by every vertex and served by the caches.  No LDS, no
// atomics, no scratch.
#include "skin_kernels.h"

__global__ __launch_bounds__(256) void k_skin_vertices(SkinParams P) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v >= P.nverts) return;
    const float* r = P.rest + 3 * (size_t)v;
    const float p[3] = {r[0], r[1], r[2]};
    const uint2 jj = ((const uint2*)__builtin_assume_aligned(P.joints, 8))[v];
    const float4 ww = ((const float4*)__builtin_assume_aligned(P.weights, 16))[v];
    const uint16_t j[4] = {(uint16_t)(jj.x & 0xFFFFu), (uint16_t)(jj.x >> 16), (uint16_t)(jj.y & 0xFFFFu), (uint16_t)(jj.y >> 16)};
    const float w[4] = {ww.x, ww.y, ww.z, ww.w};
    float o[3];
    skin_vertex(p, j, w, (const float*)__builtin_assume_aligned(P.matrices, 16), o);
    float* out = P.out + 3 * (size_t)v;
    out[0] = o[0];
    out[1] = o[1];
    out[2] = o[2];
}

extern "C" hipError_t rtk_launch_skin(const SkinParams* p, hipStream_t stream) {
    hipLaunchKernelGGL(k_skin_vertices, dim3((p->nverts + 255) / 256), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
