// closest_kernels.h — closest-point queries (rt_closest_points_device): the rule that
// turns a point and a triangle into the triangle's closest point, shared by the host (rt_point_triangle,
// rt_closest_points_host, closest.cpp) and the kernel (closest_points.hip), the rule that picks a
// query's answer among the candidates, and the lower bound on the rule's d2 for everything inside a box
// that the kernel prunes by.
//
// The rule is plain fp32, one rounding per operation (every translation unit is built with
// -ffp-contract=off) and nothing that fuses; / is correctly rounded on both sides (rtmath.h).  So the
// host functions, which compile these very functions, give the kernel's bits.  This header is the
// definition; include/rtx_amd.h restates it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtmath.h"

constexpr uint32_t kClosestFloats = 8;         // RT_CLOSEST_FLOATS: one record
constexpr float kClosestRayMax = 10e10f;       // the miss position, the renderer's RayMax
constexpr uint32_t kClosestFront = 1u << 16;   // RT_CLOSEST_FRONT
constexpr uint32_t kClosestFound = 1u << 17;   // RT_CLOSEST_FOUND
// feature codes: 0 face, 1 2 3 vertex 1 2 3, 4 edge 12, 5 edge 23, 6 edge 31

struct ClosestTri {
    float cx, cy, cz;   // the closest point
    float d2;           // squared distance; NaN: the triangle is no candidate
    float u, v;         // the weights of v1 and v2 (a hit record's barycentrics)
    uint32_t feature;   // 0..6
    uint32_t front;     // 0 / 1
};

// (ax bx + ay by) + az bz
RT_HD float closest_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// The closest point of triangle (v1, v2, v3) to p: Ericson's Voronoi-region walk (Real-Time Collision
// Detection, 5.1.5) in its branch order: vertex 1, vertex 2, edge 12, vertex 3, edge 31, edge 23, face.
// With ab = v2 - v1, ac = v3 - v1 and d1..d6 the closest_dot products of (ab, ac) with p - v1, p - v2,
// p - v3, the weights (wa, wb, wc) of (v1, v2, v3) are
//   vertex k   1 at k, 0 elsewhere
//   edge 12    t = d1 / (d1 - d3):                  (1 - t, t, 0)
//   edge 31    t = d2 / (d2 - d6):                  (1 - t, 0, t)
//   edge 23    t = (d4 - d3) / ((d4 - d3) + (d5 - d6)):   (0, 1 - t, t)
//   face       r = 1 / ((va + vb) + vc), wb = vb r and wc = vc r, each clamped: wb to [0, 1], wc to
//              [0, 1 - wb]; wa = (1 - wb) - wc.  The clamps change nothing while va, vb, vc > 0, which is
//              how exact arithmetic reaches the face; they keep the point on the triangle when rounding
//              of a sliver's va, vb, vc reaches it otherwise (the pruning bound needs that, below).  A
//              NaN passes through them.
// The point is, per component, c = (v1 wa + v2 wb) + v3 wc; d = p - c; d2 = (dx dx + dy dy) + dz dz;
// u = wa, v = wb.  front = closest_dot(n, p - v1) > 0 with n = (aby acz - abz acy, abz acx - abx acz,
// abx acy - aby acx), each component the difference of its two rounded products.  A triangle of zero
// area that reaches the face divides 1 by 0 and gets a NaN d2: no candidate; one that a vertex or edge
// branch settles is a candidate like any other.
RT_HD ClosestTri closest_point_triangle(const float* p, const float* v1, const float* v2, const float* v3) {
    const float abx = v2[0] - v1[0], aby = v2[1] - v1[1], abz = v2[2] - v1[2];
    const float acx = v3[0] - v1[0], acy = v3[1] - v1[1], acz = v3[2] - v1[2];
    const float apx = p[0] - v1[0], apy = p[1] - v1[1], apz = p[2] - v1[2];
    float wa, wb, wc;
    uint32_t feature;
    const float d1 = closest_dot(abx, aby, abz, apx, apy, apz);
    const float d2 = closest_dot(acx, acy, acz, apx, apy, apz);
    const float bpx = p[0] - v2[0], bpy = p[1] - v2[1], bpz = p[2] - v2[2];
    const float d3 = closest_dot(abx, aby, abz, bpx, bpy, bpz);
    const float d4 = closest_dot(acx, acy, acz, bpx, bpy, bpz);
    const float cpx = p[0] - v3[0], cpy = p[1] - v3[1], cpz = p[2] - v3[2];
    const float d5 = closest_dot(abx, aby, abz, cpx, cpy, cpz);
    const float d6 = closest_dot(acx, acy, acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2;
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0f && d2 <= 0.0f) {
        wa = 1.0f; wb = 0.0f; wc = 0.0f; feature = 1u;
    } else if (d3 >= 0.0f && d4 <= d3) {
        wa = 0.0f; wb = 1.0f; wc = 0.0f; feature = 2u;
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float t = d1 / (d1 - d3);
        wa = 1.0f - t; wb = t; wc = 0.0f; feature = 4u;
    } else if (d6 >= 0.0f && d5 <= d6) {
        wa = 0.0f; wb = 0.0f; wc = 1.0f; feature = 3u;
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float t = d2 / (d2 - d6);
        wa = 1.0f - t; wb = 0.0f; wc = t; feature = 6u;
    } else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {
        const float t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        wa = 0.0f; wb = 1.0f - t; wc = t; feature = 5u;
    } else {
        const float r = 1.0f / ((va + vb) + vc);
        wb = vb * r;
        wb = wb < 0.0f ? 0.0f : (wb > 1.0f ? 1.0f : wb);
        const float rest = 1.0f - wb;
        wc = vc * r;
        wc = wc < 0.0f ? 0.0f : (wc > rest ? rest : wc);
        wa = rest - wc;
        feature = 0u;
    }
    ClosestTri o;
    o.cx = (v1[0] * wa + v2[0] * wb) + v3[0] * wc;
    o.cy = (v1[1] * wa + v2[1] * wb) + v3[1] * wc;
    o.cz = (v1[2] * wa + v2[2] * wb) + v3[2] * wc;
    const float dx = p[0] - o.cx, dy = p[1] - o.cy, dz = p[2] - o.cz;
    o.d2 = (dx * dx + dy * dy) + dz * dz;
    o.u = wa;
    o.v = wb;
    o.feature = feature;
    const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    o.front = closest_dot(nx, ny, nz, apx, apy, apz) > 0.0f ? 1u : 0u;
    return o;
}

// The answer of a query so far: the lexicographically smallest (d2, triangle index) among the
// candidates met whose d2 is no NaN and does not exceed the limit.  It starts as (limit, 0xFFFFFFFF),
// which no triangle index equals, so `tri == 0xFFFFFFFF` at the end is a miss.
struct ClosestBest {
    ClosestTri t;
    float d2;       // the pruning threshold: the best d2, or the limit before a candidate is met
    uint32_t tri;
};

// max_distance * max_distance in fp32; +inf stays +inf
RT_HD float closest_limit(float max_distance) { return max_distance * max_distance; }

RT_HD bool closest_point_finite(const float* p) {
    const float big = 3.402823466e+38f;
    return p[0] >= -big && p[0] <= big && p[1] >= -big && p[1] <= big && p[2] >= -big && p[2] <= big;
}

RT_HD void closest_begin(ClosestBest& b, float limit) {
    b.d2 = limit;
    b.tri = 0xFFFFFFFFu;
    b.t.cx = b.t.cy = b.t.cz = kClosestRayMax;
    b.t.d2 = limit;
    b.t.u = b.t.v = 0.0f;
    b.t.feature = 0u;
    b.t.front = 0u;
}

// one candidate: a NaN d2 fails both comparisons
RT_HD void closest_offer(ClosestBest& b, const ClosestTri& t, uint32_t tri) {
    if (t.d2 < b.d2 || (t.d2 == b.d2 && tri < b.tri)) {
        b.t = t;
        b.d2 = t.d2;
        b.tri = tri;
    }
}

// the 32-byte record as eight 32-bit words (floats as their bits)
RT_HD void closest_record(const ClosestBest& b, uint32_t* w) {
    const bool found = b.tri != 0xFFFFFFFFu;
    const float inf = rtm::bits_to_float(0x7F800000u);
    w[0] = rtm::float_to_bits(found ? b.t.cx : kClosestRayMax);
    w[1] = rtm::float_to_bits(found ? b.t.cy : kClosestRayMax);
    w[2] = rtm::float_to_bits(found ? b.t.cz : kClosestRayMax);
    w[3] = rtm::float_to_bits(found ? b.t.d2 : inf);
    w[4] = found ? b.tri : 0xFFFFFFFFu;
    w[5] = rtm::float_to_bits(found ? b.t.u : 0.0f);
    w[6] = rtm::float_to_bits(found ? b.t.v : 0.0f);
    w[7] = found ? (b.t.feature | (b.t.front ? kClosestFront : 0u) | kClosestFound) : 0u;
}

// A lower bound on the rule's d2 of every triangle whose vertices lie in the box [mn, mx] widened by
// the leaf boxes' own rounding (below), in the rule's arithmetic, not in real arithmetic.  With
// eps = 2^-24 and, per axis, M = max(|mn|, |mx|, |p|):
//   - the weights are >= 0 and sum to 1 within 2 eps, so the exact combination of the vertices lies
//     within 2 eps M of [mn, mx]; its three products and two sums round by at most 5 eps (1 + 2 eps) M;
//   - a leaf box's upper face is mn + max(mx - mn, 2^-23 mx), rounded twice: it can lie below a vertex
//     by at most 3 eps M (bvh_build.hip); inner boxes are exact min / max merges of leaf boxes;
//   - the gap g = max(mn - p, p - mx, 0) rounds once (gaps are at most 2 M: 2 eps M), gap - slack once
//     more (2 eps M), and the rule's d = p - c once (2 eps M).
// Together under 17 eps M; the slack is 32 eps M.  So l = max(g - slack, 0) <= |d| on every axis, and
// since the bound squares and adds in the rule's own order and fp32 multiplication and addition are
// monotone, (lx lx + ly ly) + lz lz <= d2, bit for bit.  (A triangle with a vertex that is not finite
// has a NaN d2 and is no candidate, so the argument needs no box of such a triangle to be right.)
RT_HD float closest_axis_bound(float p, float mn, float mx) {
    const float a = mn - p, b = p - mx;
    float g = a > b ? a : b;
    const float amn = mn < 0.0f ? -mn : mn, amx = mx < 0.0f ? -mx : mx, ap = p < 0.0f ? -p : p;
    float m = amn > amx ? amn : amx;
    m = m > ap ? m : ap;
    g = g - 1.9073486328125e-06f * m;  // 32 * 2^-24
    return g < 0.0f ? 0.0f : g;
}
RT_HD float closest_box_bound(const float* p, float mnx, float mny, float mnz, float mxx, float mxy, float mxz) {
    const float lx = closest_axis_bound(p[0], mnx, mxx), ly = closest_axis_bound(p[1], mny, mxy),
                lz = closest_axis_bound(p[2], mnz, mxz);
    return (lx * lx + ly * ly) + lz * lz;
}
