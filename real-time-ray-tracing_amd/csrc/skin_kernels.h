// skin_kernels.h — linear-blend skinning (rt_set_skin / rt_pose_skin*): the rule that
// turns a rest position, four joint indices, four weights and a table of 3 x 4 joint matrices into a
// posed position, shared by the host (rt_skin_vertices, skin.cpp) and the kernel (skin.hip), and the
// kernel's launch interface.
//
// The rule is plain fp32, one rounding per operation (every translation unit is built with
// -ffp-contract=off) and nothing that fuses, so the host function, which compiles these very functions,
// gives the kernel's bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtmath.h"

constexpr uint32_t kSkinInfluences = 4;     // RT_SKIN_INFLUENCES
constexpr uint32_t kSkinJointsMax = 4096;   // RT_SKIN_JOINTS_MAX
constexpr uint32_t kSkinMatrixFloats = 12;  // one joint: row-major 3 x 4, translation in column 3

// row r of matrix m applied to the point (px, py, pz, 1): ((m0 px + m1 py) + m2 pz) + m3
RT_HD float skin_row(float m0, float m1, float m2, float m3, float px, float py, float pz) {
    return ((m0 * px + m1 * py) + m2 * pz) + m3;
}

// One vertex.  acc starts at +0 and takes w[k] * (M[j[k]] p) for k = 0..3 in this order; an influence of
// weight 0 is skipped and its matrix is not read, so a NaN in a joint no non-zero weight names reaches
// no vertex.  Weights are used as given (not normalised).  Under the identity a -0 component of p comes
// out as +0 (+0 + -0), every other value as it is.
RT_HD void skin_vertex(const float* p, const uint16_t* j, const float* w, const float* matrices, float* out) {
    const float px = p[0], py = p[1], pz = p[2];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (uint32_t k = 0; k < kSkinInfluences; ++k) {
        const float wk = w[k];
        if (wk == 0.0f) continue;
        const float* m = matrices + (size_t)j[k] * kSkinMatrixFloats;
        a0 = a0 + wk * skin_row(m[0], m[1], m[2], m[3], px, py, pz);
        a1 = a1 + wk * skin_row(m[4], m[5], m[6], m[7], px, py, pz);
        a2 = a2 + wk * skin_row(m[8], m[9], m[10], m[11], px, py, pz);
    }
    out[0] = a0;
    out[1] = a1;
    out[2] = a2;
}

// One pose (skin.hip): vertex v of [0, nverts) from rest / joints / weights under `matrices` into `out`.
// Every array is device memory; matrices is 16-byte aligned and holds every joint the skin names.
struct SkinParams {
    const float* rest;        // [nverts * 3]
    const uint16_t* joints;   // [nverts * 4], 8-byte aligned
    const float* weights;     // [nverts * 4], 16-byte aligned
    const float* matrices;    // [jointCount * 12], 16-byte aligned
    float* out;               // [nverts * 3]
    uint32_t nverts;
};
extern "C" hipError_t rtk_launch_skin(const SkinParams* p, hipStream_t stream);
