// closest.cpp — the closest-point rule on the host (rt_point_triangle, rt_closest_points_host) and the
// argument checks that rt_closest_points_device shares with them.  closest_kernels.h's functions are
// compiled here as the kernel compiles them (closest_points.hip), under the same -ffp-contract=off, so
// the two give the same bits.
#include <string.h>

#include "context.h"
#include "closest_kernels.h"

// max_distance is >= 0 or +inf (a NaN fails the comparison)
bool closest_distance_ok(float max_distance) { return max_distance >= 0.0f; }

extern "C" int rt_point_triangle(const float p[3], const float xyz[9], float out8[8]) {
    if (!p || !xyz || !out8) return RT_ERR_ARG;
    ClosestBest best;
    closest_begin(best, closest_limit(rtm::bits_to_float(0x7F800000u)));
    if (closest_point_finite(p)) closest_offer(best, closest_point_triangle(p, xyz, xyz + 3, xyz + 6), 0u);
    uint32_t w[8];
    closest_record(best, w);
    memcpy(out8, w, sizeof w);
    return RT_OK;
}

// The definition, exhaustively: every triangle is offered to every point.  closest_offer keeps the
// smallest (d2, id), so the order of the triangles does not matter.
extern "C" int rt_closest_points_host(const float* tris, const uint32_t* ids, uint32_t ntri, const float* points, uint32_t n,
                                      float max_distance, float* out) {
    if ((ntri > 0u && !tris) || (n > 0u && (!points || !out))) return RT_ERR_ARG;
    if (!closest_distance_ok(max_distance)) return RT_ERR_ARG;
    if (ids)
        for (uint32_t t = 0; t < ntri; ++t)
            if (ids[t] == 0xFFFFFFFFu) return RT_ERR_ARG;  // the miss record's index
    const float limit = closest_limit(max_distance);
    for (uint32_t i = 0; i < n; ++i) {
        const float* p = points + 3 * (size_t)i;
        ClosestBest best;
        closest_begin(best, limit);
        if (closest_point_finite(p))
            for (uint32_t t = 0; t < ntri; ++t) {
                const float* v = tris + 9 * (size_t)t;
                closest_offer(best, closest_point_triangle(p, v, v + 3, v + 6), ids ? ids[t] : t);
            }
        uint32_t w[8];
        closest_record(best, w);
        memcpy(out + kClosestFloats * (size_t)i, w, sizeof w);
    }
    return RT_OK;
}
