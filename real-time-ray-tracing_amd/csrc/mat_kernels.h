// mat_kernels.h — launch interface of the material-table kernels (materials.hip) and the device's
// statement of the class rule, shared with the host so that a test can pin it to rt_material_classes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rtx_amd.h"

// The kernel class of one material id as k_mat_set computes it, branch-free: the restatement of
// rt_material_classes (context.cpp), which is the rule.  Glossy: 1, 5 and every id >= 10;
// microfacet: 4.  rt_material_class_rule exposes this very function to the host
// (tests/test_materials_device_api.py compares the two over all 256 ids).
__host__ __device__ inline uint32_t mat_class_of(uint32_t id) {
    const uint32_t glossy = (uint32_t)(id == 1u) | (uint32_t)(id == 5u) | (uint32_t)(id >= 10u);
    const uint32_t micro = (uint32_t)(id == 4u);
    return glossy * RT_MAT_CLASS_GLOSSY | micro * RT_MAT_CLASS_MICROFACET;
}

constexpr uint32_t kMatDefaultId = 3u;  // the reference's table: material 3 for every triangle

// One device material set (materials.hip): dst = prev (or 3 everywhere) with [first, first + count)
// replaced by src, an id of an undeclared class stored as 3 and counted, every byte from triCount up
// to capBytes 3, and the census of the ids below triCount.
struct MatSetParams {
    const uint8_t* prev;   // the previous table, [capBytes], 16-byte aligned; null: 3 everywhere
    const uint8_t* src;    // [count] the caller's ids (device memory, any alignment)
    uint8_t* dst;          // [capBytes], 16-byte aligned; another buffer than prev
    uint32_t* census;      // [256] triangles per id of dst over [0, triCount) (zeroed by the launcher)
    uint32_t* badCount;    // device word, zero between sets: the ids of undeclared classes
    uint32_t* status;      // pinned host words (kStatusMatUndeclared)
    uint32_t first, count, triCount;
    uint32_t capBytes;     // a multiple of 16
    uint32_t classes;      // RT_MAT_CLASS_* bits the caller declared
};
extern "C" hipError_t rtk_launch_mat_set(const MatSetParams* p, hipStream_t stream);
