// sdf_kernels.h — signed distance queries (rt_signed_distance_device): the rule that
// gives every vertex and edge of a build its angle-weighted pseudo-normal (Baerentzen and Aanaes,
// "Signed distance computation using the angle weighted pseudonormal", 2005) and the rule that turns a
// point and its closest-point record into a signed distance.  Shared by the host (rt_pseudo_normals,
// rt_signed_distance_rule, sdf.cpp) and the kernels (sdf.hip).
//
// Plain fp32, one rounding per operation (every translation unit is built with -ffp-contract=off),
// nothing fused; /, sqrtf and rt_acosf give the same bits on both sides (rtmath.h).  So the host
// functions, which compile these very functions, give the kernels' bits.  This header is the definition;
// include/rtx_amd.h restates it.
//
// Vertex identity is the index: the pseudo-normal of a vertex or an edge sums over the triangles that
// name the same vertex ids, so a mesh that repeats a position under two indices (unwelded), or winds
// neighbouring triangles inconsistently, gets per-index pseudo-normals that mean little.  Welding is
// the caller's job.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "closest_kernels.h"
#include "rtmath.h"

constexpr uint32_t kSdfEntries = 6;   // table entries per triangle: vertex 1 2 3, edge 12 23 31 (feature codes 1..6)
constexpr uint32_t kSdfNoVertex = 0xFFFFFFFFu;

struct SdfVec {
    float x, y, z;
};

// The unit normal of triangle (v1, v2, v3): n = ab x ac as closest_point_triangle's front bit computes
// it (each product rounded, then the difference), l2 = (nx nx + ny ny) + nz nz, n / sqrtf(l2) per
// component.  False, with n = (0, 0, 0), for a degenerate triangle: l2 > 0 is false or l2 is not finite.
RT_HD bool sdf_unit_normal(const float* v1, const float* v2, const float* v3, SdfVec& n) {
    const float abx = v2[0] - v1[0], aby = v2[1] - v1[1], abz = v2[2] - v1[2];
    const float acx = v3[0] - v1[0], acy = v3[1] - v1[1], acz = v3[2] - v1[2];
    const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    const float l2 = (nx * nx + ny * ny) + nz * nz;
    if (!(l2 > 0.0f) || !(l2 <= 3.402823466e+38f)) {
        n.x = n.y = n.z = 0.0f;
        return false;
    }
    const float l = __builtin_sqrtf(l2);
    n.x = nx / l;
    n.y = ny / l;
    n.z = nz / l;
    return true;
}

// The angle at vertex o between the edges to a and b: geometry.hip's corner_weight with the quotient
// clamped to [-1, 1]; a NaN stays a NaN
RT_HD float sdf_corner_angle(const float* o, const float* a, const float* b) {
    const float eax = a[0] - o[0], eay = a[1] - o[1], eaz = a[2] - o[2];
    const float ebx = b[0] - o[0], eby = b[1] - o[1], ebz = b[2] - o[2];
    const float la = closest_dot(eax, eay, eaz, eax, eay, eaz), lb = closest_dot(ebx, eby, ebz, ebx, eby, ebz);
    float q = closest_dot(eax, eay, eaz, ebx, eby, ebz) / __builtin_sqrtf(la * lb);
    q = q < -1.0f ? -1.0f : (q > 1.0f ? 1.0f : q);
    return rt_acosf(q);
}

// the three corner angles: corner 1 between v2 - v1 and v3 - v1, corner 2 between v3 - v2 and v1 - v2,
// corner 3 between v1 - v3 and v2 - v3
RT_HD void sdf_corner_angles(const float* v1, const float* v2, const float* v3, float* angle) {
    angle[0] = sdf_corner_angle(v1, v2, v3);
    angle[1] = sdf_corner_angle(v2, v3, v1);
    angle[2] = sdf_corner_angle(v3, v1, v2);
}

// One step of the walk over the slots of vertex a (adjacency order: ascending corner index), for the
// triangle t' that owns the slot's corner: `valid` (t' below the triangle count and not degenerate), its
// unit normal n, its angle at the corner, and the vertex ids at its two other corners.  The vertex sum
// takes angle * n (the product rounded first) unless the angle is a NaN; the sum of the edge (a, b) takes
// n when the triangle carries b at another corner.  Both start from +0.
RT_HD void sdf_walk_step(SdfVec& vtx, SdfVec& edge, bool valid, const SdfVec& n, float angle, uint32_t other1,
                         uint32_t other2, uint32_t b) {
    if (!valid) return;
    if (angle == angle) {
        vtx.x = vtx.x + angle * n.x;
        vtx.y = vtx.y + angle * n.y;
        vtx.z = vtx.z + angle * n.z;
    }
    if (other1 == b || other2 == b) {
        edge.x = edge.x + n.x;
        edge.y = edge.y + n.y;
        edge.z = edge.z + n.z;
    }
}

// The sign record of point p from its closest record (eight words, closest_kernels.h) and N: the table
// entry of (triangle, feature) for features 1..6, the triangle's own unit normal for the face.
// d = p - c per component with c the record's closest point; s = (Nx dx + Ny dy) + Nz dz;
// out = (N, sqrtf(d2)), .w negated when s < 0 (a zero or NaN s reads as outside), d2 the record's.  N is
// not normalised; an all-zero N says that no incident triangle counted.
RT_HD void sdf_sign_record(const float* p, const uint32_t* w, const SdfVec& N, float* out) {
    const float dx = p[0] - rtm::bits_to_float(w[0]), dy = p[1] - rtm::bits_to_float(w[1]),
                dz = p[2] - rtm::bits_to_float(w[2]);
    const float s = closest_dot(N.x, N.y, N.z, dx, dy, dz);
    const float dist = __builtin_sqrtf(rtm::bits_to_float(w[3]));
    out[0] = N.x;
    out[1] = N.y;
    out[2] = N.z;
    out[3] = s < 0.0f ? -dist : dist;
}

// A record that names no triangle: the found bit clear, index -1, or a feature code past 6
RT_HD bool sdf_record_miss(const uint32_t* w) {
    return (w[7] & kClosestFound) == 0u || w[4] == 0xFFFFFFFFu || (w[7] & 0xFFFFu) > 6u;
}

RT_HD void sdf_miss_record(float* out) {
    out[0] = out[1] = out[2] = 0.0f;
    out[3] = rtm::bits_to_float(0x7F800000u);
}
