// sdf.hip — signed distance queries (rt_set_signed_distance, rt_signed_distance_device, DESIGN.md
// §4.1.1c) for gfx950: the pseudo-normal table of an LBVH build and the sign pass behind a closest-point
// query.  sdf_kernels.h is the rule; these kernels only arrange its work.
//
// The table, behind each build on the build's stream (build_bvh), in geometry.hip's two-pass CSR shape:
//
//   k_sdf_triangles  one thread per (padded) triangle: the unit normal and the three corner angles once,
//                    stored with the two other corners' vertex ids at the corners' CSR slots.  A
//                    triangle that does not count (padding, degenerate) stores a record that says so.
//   k_sdf_gather     one thread per corner (t, k) of a triangle below triCount: it walks the slots of
//                    the corner's vertex in order and sums the vertex pseudo-normal (entry k) and the
//                    pseudo-normal of the edge from this corner to the next (entry 3 + k).  The walk is
//                    in ascending corner index from either end of an edge, so the two triangles of an
//                    edge store the same bits.
//
// The scattered side is the triangle pass's stores; the gather reads one contiguous run of 24-byte
// records per thread with no index load between the offsets and the values.  The same sums in the same
// order under -ffp-contract=off: no float atomics, deterministic.  A vertex's sum is recomputed by every
// corner that names it (about six times on a closed mesh); a vertex pass of its own would save those
// reads and add a launch and a dependent gather, and the whole table costs a fraction of the build.
//
// The sign pass (k_sdf_sign): one lane per point in a dense grid behind k_closest_points, in the shape of
// surface_rays.hip.  It reads the point, the two quads of its closest record, the named triangle's
// record of the LBVH set (the face's normal) or one table entry, and stores one quad.  No LDS, no
// atomics, no inline assembly, no s_setprio, no barrier.
#include "frame_kernels.h"
#include "sdf_kernels.h"

namespace {

constexpr int kSdfBlock = 256;

__global__ __launch_bounds__(kSdfBlock) void k_sdf_triangles(SdfTableParams P) {
    const uint32_t t = blockIdx.x * (uint32_t)kSdfBlock + threadIdx.x;
    if (t >= P.triCountPadded) return;
    const uint32_t id[3] = {P.indices[3 * (size_t)t], P.indices[3 * (size_t)t + 1], P.indices[3 * (size_t)t + 2]};
    SdfVec n;
    n.x = n.y = n.z = 0.0f;
    float angle[3] = {0.0f, 0.0f, 0.0f};
    bool valid = t < P.triCount && id[0] < P.nverts && id[1] < P.nverts && id[2] < P.nverts;
    if (valid) {
        const float* a = P.vertices + 3 * (size_t)id[0];
        const float* b = P.vertices + 3 * (size_t)id[1];
        const float* c = P.vertices + 3 * (size_t)id[2];
        const float v1[3] = {a[0], a[1], a[2]}, v2[3] = {b[0], b[1], b[2]}, v3[3] = {c[0], c[1], c[2]};
        valid = sdf_unit_normal(v1, v2, v3, n);
        if (valid) sdf_corner_angles(v1, v2, v3, angle);
    }
    const uint32_t slots = 3u * P.triCountPadded;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t s = P.cornerSlot[3 * (size_t)t + k];
        if (s >= slots) continue;  // no valid adjacency names such a slot
        P.slotNormal[s] = make_float4(n.x, n.y, n.z, angle[k]);
        P.slotOthers[s] = valid ? make_uint2(id[(k + 1) % 3], id[(k + 2) % 3]) : make_uint2(kSdfNoVertex, kSdfNoVertex);
    }
}

__global__ __launch_bounds__(kSdfBlock) void k_sdf_gather(SdfTableParams P) {
    const uint32_t c = blockIdx.x * (uint32_t)kSdfBlock + threadIdx.x;  // triCount < 2^30: 3 triCount fits
    if (c >= 3u * P.triCount) return;
    const uint32_t t = c / 3u, k = c - 3u * t;
    const uint32_t a = P.indices[c], b = P.indices[3 * (size_t)t + (k + 1u) % 3u];
    SdfVec vtx, edge;
    vtx.x = vtx.y = vtx.z = 0.0f;
    edge.x = edge.y = edge.z = 0.0f;
    if (a < P.nverts) {
        const uint32_t slots = 3u * P.triCountPadded;
        uint32_t s0 = P.adjOffsets[a], s1 = P.adjOffsets[a + 1];
        s1 = s1 < slots ? s1 : slots;
        for (uint32_t s = s0; s < s1; ++s) {
            const float4 r = P.slotNormal[s];
            const uint2 o = P.slotOthers[s];
            SdfVec n;
            n.x = r.x;
            n.y = r.y;
            n.z = r.z;
            sdf_walk_step(vtx, edge, !(o.x == kSdfNoVertex && o.y == kSdfNoVertex), n, r.w, o.x, o.y, b);
        }
    }
    float4* e = P.table + kSdfEntries * (size_t)t;
    e[k] = make_float4(vtx.x, vtx.y, vtx.z, 0.0f);
    e[3u + k] = make_float4(edge.x, edge.y, edge.z, 0.0f);
}

__global__ __launch_bounds__(kSdfBlock) void k_sdf_sign(SdfSignParams P) {
    const uint32_t i = blockIdx.x * (uint32_t)kSdfBlock + threadIdx.x;  // < 2^22 * 256 + 256
    if (i >= P.n) return;
    const float* pp = P.points + (size_t)i * P.stride;
    const float p[3] = {pp[0], pp[1], pp[2]};
    const uint4* rec = reinterpret_cast<const uint4*>(P.records) + 2 * (size_t)i;
    const uint4 q0 = rec[0], q1 = rec[1];
    const uint32_t w[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    float out[4];
    if (sdf_record_miss(w) || w[4] >= P.triCount) {
        sdf_miss_record(out);
    } else {
        const uint32_t tri = w[4];
        const uint32_t feature = w[7] & 0xFFFFu;  // <= 6 (sdf_record_miss)
        SdfVec N;
        if (feature == 0u) {
            const float4* tp = P.triPos + 4 * (size_t)tri;
            const float4 a = tp[0], b = tp[1], c = tp[2];
            const float v1[3] = {a.x, a.y, a.z}, v2[3] = {b.x, b.y, b.z}, v3[3] = {c.x, c.y, c.z};
            sdf_unit_normal(v1, v2, v3, N);
        } else {
            const float4 e = P.table[kSdfEntries * (size_t)tri + (feature - 1u)];
            N.x = e.x;
            N.y = e.y;
            N.z = e.z;
        }
        sdf_sign_record(p, w, N, out);
    }
    reinterpret_cast<float4*>(P.out)[i] = make_float4(out[0], out[1], out[2], out[3]);
}

}  // namespace

extern "C" hipError_t rtk_launch_sdf_table(const SdfTableParams* p, hipStream_t stream) {
    if (p->triCount == 0u || p->triCount > p->triCountPadded || p->triCountPadded > (1u << 30) || p->nverts == 0u ||
        !p->slotNormal || !p->slotOthers || !p->table)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sdf_triangles, dim3((p->triCountPadded + kSdfBlock - 1u) / kSdfBlock), dim3(kSdfBlock), 0, stream, *p);
    hipLaunchKernelGGL(k_sdf_gather, dim3((3u * p->triCount + kSdfBlock - 1u) / kSdfBlock), dim3(kSdfBlock), 0, stream, *p);
    return hipGetLastError();
}

extern "C" hipError_t rtk_launch_sdf_sign(const SdfSignParams* p, hipStream_t stream) {
    if (p->n == 0u || p->n > RT_QUERY_MAX_RAYS || p->stride < 3u || !p->table || !p->records || !p->out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sdf_sign, dim3((p->n + kSdfBlock - 1u) / kSdfBlock), dim3(kSdfBlock), 0, stream, *p);
    return hipGetLastError();
}
