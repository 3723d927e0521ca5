// geometry.hip — animated geometry for gfx950: new vertex positions for a range of the mesh and
// the smooth normals of the whole mesh, as two kernels on the frame's critical path ahead of the
// LBVH build (rt_update_vertices / rt_update_vertices_device).
//
// The normals are those of k_smooth_normals (trace_primary.hip), bit for bit: GenerateSmoothNormals
// run twice into an un-cleared buffer (kernel.cu:228-257, 313-327), angle-weighted, accumulated in
// triangle order.  That kernel recomputes a triangle's cross product and a corner's angle for every
// vertex that touches it, twice, behind a three-deep chain of dependent loads (corner -> indices ->
// positions).  Here every value is computed once:
//
//   k_geom_triangles  one thread per (padded) triangle: cross(v2-v0, v2-v1)/2 and the three angle
//                     weights, the three products pnma * w_k stored at the corners' CSR slots
//   k_geom_vertices   one thread per vertex: the sum of its slots [adjOff[v], adjOff[v+1]) in order,
//                     twice, acc = acc + c as k_smooth_normals associates it; it also stores the
//                     vertex's new position (and, for geometry motion vectors, first keeps the
//                     old one: GeomUpdateParams::prevVerts)
//
// and, behind an LBVH build, k_geom_displacement turns the kept positions into the build's
// displacement records (below; rt_set_geometry_motion).
//
// The contributions are kept in CSR order: the scattered side is then the triangle
// pass's stores, which no wave waits for, and the vertex pass reads one contiguous run per thread,
// consecutive threads' runs adjoining, with no index load between the offsets and the values.
// The same products summed in the same order with -ffp-contract=off: no float atomics, deterministic.
//
// The triangle pass reads a vertex of [first, first + count) from the caller's array and any other
// from the vertex array, which only the vertex pass (the next kernel on the stream) writes, so the
// scatter needs no kernel of its own.
#include "bvh_kernels.h"
#include "rt_device.h"

using namespace rtd;

namespace {

RT_DEV F3 geom_position(const GeomUpdateParams& P, uint32_t i) {
    const uint32_t r = i - P.first;  // wraps for i < first
    const float* p = r < P.count ? P.src + 3 * (size_t)r : P.vertices + 3 * (size_t)i;
    return f3(p[0], p[1], p[2]);
}

RT_DEV float corner_weight(F3 ea, F3 eb) {
    return rt_acosf(dot(ea, eb) / __builtin_sqrtf(length2(ea) * length2(eb)));
}

}  // namespace

__global__ __launch_bounds__(256) void k_geom_triangles(GeomUpdateParams P) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P.triCountPadded) return;
    const uint32_t i0 = P.indices[3 * t], i1 = P.indices[3 * t + 1], i2 = P.indices[3 * t + 2];
    const uint32_t s0 = P.cornerSlot[3 * t], s1 = P.cornerSlot[3 * t + 1], s2 = P.cornerSlot[3 * t + 2];
    const F3 v0 = geom_position(P, i0), v1 = geom_position(P, i1), v2 = geom_position(P, i2);
    const F3 pnma = cross(v2 - v0, v2 - v1) / 2.0f;
    const F3 c0 = pnma * corner_weight(v2 - v0, v1 - v0);
    const F3 c1 = pnma * corner_weight(v2 - v1, v0 - v1);
    const F3 c2 = pnma * corner_weight(v0 - v2, v1 - v2);
    float* o0 = P.contrib + 3 * (size_t)s0;
    float* o1 = P.contrib + 3 * (size_t)s1;
    float* o2 = P.contrib + 3 * (size_t)s2;
    o0[0] = c0.x; o0[1] = c0.y; o0[2] = c0.z;
    o1[0] = c1.x; o1[1] = c1.y; o1[2] = c1.z;
    o2[0] = c2.x; o2[1] = c2.y; o2[2] = c2.z;
}

__global__ __launch_bounds__(256) void k_geom_vertices(GeomUpdateParams P) {
    const uint32_t vtx = blockIdx.x * 256 + threadIdx.x;
    if (vtx >= P.nverts) return;
    const uint32_t a0 = P.adjOffsets[vtx], a1 = P.adjOffsets[vtx + 1];
    F3 acc = f3(0.0f);
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t a = a0; a < a1; ++a) {
            const float* c = P.contrib + 3 * (size_t)a;
            acc = acc + f3(c[0], c[1], c[2]);
        }
    float* n = P.normals + 3 * (size_t)vtx;
    n[0] = acc.x; n[1] = acc.y; n[2] = acc.z;
    float* v = P.vertices + 3 * (size_t)vtx;
    if (P.prevVerts) {  // the position this update replaces, or keeps: the last build's (geometry motion)
        float* q = P.prevVerts + 3 * (size_t)vtx;
        q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
    }
    const uint32_t r = vtx - P.first;
    if (r < P.count) {
        const float* s = P.src + 3 * (size_t)r;
        v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
    }
}

// Geometry motion vectors: one thread per triangle record of the LBVH set just built, the three
// corners' displacement since the previous build.  The records are in the mesh's triangle order (the
// build gathers triangle g into record g and sorts leaf indices, not records), so record t's
// corners are indices[3t ..]; a vertex no update touched has prevVerts == vertices bit for bit and
// the difference is +0.  Per corner one index load and two 12-byte gathers behind it, per thread
// three 16-byte stores, consecutive threads' stores adjoining: memory-bound, no LDS, no atomics.
__global__ __launch_bounds__(256) void k_geom_displacement(GeomDispParams P) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P.triCountPadded) return;
    const uint32_t* ip = P.indices + 3 * (size_t)t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t i = ip[k];
        const float* c = P.vertices + 3 * (size_t)i;
        const float* q = P.prevVerts + 3 * (size_t)i;
        P.triDisp[3 * (size_t)t + k] = make_float4(c[0] - q[0], c[1] - q[1], c[2] - q[2], 0.0f);
    }
}

extern "C" hipError_t rtk_launch_geometry_update(const GeomUpdateParams* p, hipStream_t stream) {
    hipLaunchKernelGGL(k_geom_triangles, dim3((p->triCountPadded + 255) / 256), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(k_geom_vertices, dim3((p->nverts + 255) / 256), dim3(256), 0, stream, *p);
    return hipGetLastError();
}

extern "C" hipError_t rtk_launch_geometry_displacement(const GeomDispParams* p, hipStream_t stream) {
    hipLaunchKernelGGL(k_geom_displacement, dim3((p->triCountPadded + 255) / 256), dim3(256), 0, stream, *p);
    return hipGetLastError();
}
