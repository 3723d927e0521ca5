// adjacency.cpp — the vertex -> corner adjacency on the host (rt_mesh_adjacency): no context, no device.
// A translation unit of its own, so that a host-only program (tools/sdf_host_check.cpp) compiles the very
// function the library and rt_pseudo_normals use.
#include <vector>

#include "rtx_amd.h"

extern "C" {

// rt_init's vertex -> corner CSR (kernel.cu:313-327 walks it in triangle order) and its inverse; the
// definition the device kernels of a mesh set reproduce (mesh.hip)
int rt_mesh_adjacency(const uint32_t* indices, uint32_t padded_triangles, uint32_t vertex_count, uint32_t* adj_offsets,
                      uint32_t* adj_corners, uint32_t* corner_slots) {
    if (!indices || !adj_offsets || vertex_count == 0) return RT_ERR_ARG;
    const size_t n = (size_t)padded_triangles * 3;
    for (size_t c = 0; c < n; ++c)
        if (indices[c] >= vertex_count) return RT_ERR_ARG;
    for (size_t v = 0; v <= vertex_count; ++v) adj_offsets[v] = 0;
    for (size_t c = 0; c < n; ++c) adj_offsets[(size_t)indices[c] + 1]++;
    for (size_t v = 0; v < vertex_count; ++v) adj_offsets[v + 1] += adj_offsets[v];
    if (!adj_corners && !corner_slots) return RT_OK;
    std::vector<uint32_t> fill(adj_offsets, adj_offsets + vertex_count);
    for (size_t c = 0; c < n; ++c) {
        const uint32_t slot = fill[indices[c]]++;
        if (corner_slots) corner_slots[c] = slot;
        if (adj_corners) adj_corners[slot] = (uint32_t)c;
    }
    return RT_OK;
}

}  // extern "C"
