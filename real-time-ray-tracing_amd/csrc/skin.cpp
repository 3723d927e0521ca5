// skin.cpp — the skinning rule on the host (rt_skin_vertices) and the checks of a caller's skin that
// rt_set_skin shares with it.  skin_kernels.h's functions are compiled here as the kernel compiles them
// (skin.hip), under the same -ffp-contract=off, so the two give the same bits.
#include "context.h"
#include "skin_kernels.h"

// what is wrong with a skin's sizes or pointers, or null
const char* skin_shape_fault(const rt_skin* s) {
    if (!s->rest_xyz || !s->joints || !s->weights) return "rest_xyz, joints and weights must not be NULL";
    if (s->vertex_count == 0u) return "a skin has at least 1 vertex";
    if (s->joint_count == 0u || s->joint_count > kSkinJointsMax) return "joint_count must be 1..RT_SKIN_JOINTS_MAX";
    return nullptr;
}

// ... or with its contents: every joint index names a joint, slots of weight 0 included; every weight
// is finite and not negative
const char* skin_content_fault(const rt_skin* s, uint32_t& vertex) {
    for (uint32_t v = 0; v < s->vertex_count; ++v)
        for (uint32_t k = 0; k < kSkinInfluences; ++k) {
            const float w = s->weights[(size_t)v * kSkinInfluences + k];
            vertex = v;
            if (s->joints[(size_t)v * kSkinInfluences + k] >= s->joint_count) return "a joint index is not below joint_count";
            if (!(w >= 0.0f) || w > 3.402823466e+38f) return "a weight is negative or not finite";
        }
    return nullptr;
}

extern "C" int rt_skin_vertices(const rt_skin* s, const float* matrices, float* xyz_out) {
    if (!s || !matrices || !xyz_out) return RT_ERR_ARG;
    uint32_t at = 0;
    if (skin_shape_fault(s) || skin_content_fault(s, at)) return RT_ERR_ARG;
    for (uint32_t v = 0; v < s->vertex_count; ++v)
        skin_vertex(s->rest_xyz + 3 * (size_t)v, s->joints + kSkinInfluences * (size_t)v, s->weights + kSkinInfluences * (size_t)v,
                    matrices, xyz_out + 3 * (size_t)v);
    return RT_OK;
}
