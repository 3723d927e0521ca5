// sdf.cpp — the signed distance rule on the host (rt_pseudo_normals, rt_signed_distance_rule): no
// context, no device.  sdf_kernels.h's functions are compiled here as the kernels compile them (sdf.hip),
// under the same -ffp-contract=off, so the two give the same bits.
#include <string.h>

#include <vector>

#include "rtx_amd.h"
#include "sdf_kernels.h"

// The table of a mesh: per triangle the six entries vertex 1 2 3, edge 12 23 31, four floats each
// (.w = 0).  The adjacency is rt_mesh_adjacency's over the given triangles; every walk is the kernels'.
extern "C" int rt_pseudo_normals(const float* xyz, uint32_t vertex_count, const uint32_t* indices, uint32_t triangle_count,
                                 float* out) {
    if (!xyz || !indices || !out || vertex_count == 0u || triangle_count == 0u) return RT_ERR_ARG;
    const size_t corners = (size_t)triangle_count * 3;
    std::vector<uint32_t> off((size_t)vertex_count + 1), adj(corners);
    if (rt_mesh_adjacency(indices, triangle_count, vertex_count, off.data(), adj.data(), nullptr) != RT_OK)
        return RT_ERR_ARG;  // an index at or past vertex_count
    std::vector<SdfVec> unit(triangle_count);
    std::vector<float> angle(corners);
    std::vector<uint8_t> valid(triangle_count);
    for (uint32_t t = 0; t < triangle_count; ++t) {
        const uint32_t* id = indices + 3 * (size_t)t;
        const float *v1 = xyz + 3 * (size_t)id[0], *v2 = xyz + 3 * (size_t)id[1], *v3 = xyz + 3 * (size_t)id[2];
        valid[t] = sdf_unit_normal(v1, v2, v3, unit[t]) ? 1 : 0;
        float* a = angle.data() + 3 * (size_t)t;
        a[0] = a[1] = a[2] = 0.0f;
        if (valid[t]) sdf_corner_angles(v1, v2, v3, a);
    }
    for (size_t c = 0; c < corners; ++c) {
        const size_t t = c / 3, k = c - 3 * t;
        const uint32_t a = indices[c], b = indices[3 * t + (k + 1) % 3];
        SdfVec vtx = {0.0f, 0.0f, 0.0f}, edge = {0.0f, 0.0f, 0.0f};
        for (uint32_t s = off[a]; s < off[a + 1]; ++s) {
            const size_t c2 = adj[s], t2 = c2 / 3, k2 = c2 - 3 * t2;
            sdf_walk_step(vtx, edge, valid[t2] != 0, unit[t2], angle[c2], indices[3 * t2 + (k2 + 1) % 3],
                          indices[3 * t2 + (k2 + 2) % 3], b);
        }
        float* e = out + 24 * t;
        e[4 * k] = vtx.x; e[4 * k + 1] = vtx.y; e[4 * k + 2] = vtx.z; e[4 * k + 3] = 0.0f;
        e[12 + 4 * k] = edge.x; e[12 + 4 * k + 1] = edge.y; e[12 + 4 * k + 2] = edge.z; e[12 + 4 * k + 3] = 0.0f;
    }
    return RT_OK;
}

// One point's sign record from its closest record, the named triangle's positions and its six entries
extern "C" int rt_signed_distance_rule(const float p[3], const float rec8[8], const float xyz9[9], const float pn24[24],
                                       float out4[4]) {
    if (!p || !rec8 || !xyz9 || !pn24 || !out4) return RT_ERR_ARG;
    uint32_t w[8];
    memcpy(w, rec8, sizeof w);
    if (sdf_record_miss(w)) {
        sdf_miss_record(out4);
        return RT_OK;
    }
    const uint32_t feature = w[7] & 0xFFFFu;
    SdfVec N;
    if (feature == 0u) {
        sdf_unit_normal(xyz9, xyz9 + 3, xyz9 + 6, N);
    } else {
        const float* e = pn24 + 4 * (feature - 1u);
        N.x = e[0];
        N.y = e[1];
        N.z = e[2];
    }
    sdf_sign_record(p, w, N, out4);
    return RT_OK;
}
