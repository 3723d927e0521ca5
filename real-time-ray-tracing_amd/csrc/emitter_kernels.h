// emitter_kernels.h — emitter sampling (rt_set_emitter_sampling): the two rules the
// kernels and the host share, and the launch interface of the list build (emitters.hip).
//
// The rules are plain fp32, one rounding per operation (every translation unit is built with
// -ffp-contract=off, and sqrtf is correctly rounded on both sides), so rt_emitter_weight and
// rt_emitter_select, which compile these very functions for the host, give the kernels' bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// (v1 - v0) x (v2 - v0) of the triangle xyz = v0 | v1 | v2: twice the area in length, the plane's normal
// in direction.  The list build takes the area from it and the sampler area and normal.
__host__ __device__ inline void emitter_cross(const float* xyz, float* c) {
    const float ax = xyz[3] - xyz[0], ay = xyz[4] - xyz[1], az = xyz[5] - xyz[2];
    const float bx = xyz[6] - xyz[0], by = xyz[7] - xyz[1], bz = xyz[8] - xyz[2];
    c[0] = ay * bz - az * by;
    c[1] = az * bx - ax * bz;
    c[2] = ax * by - ay * bx;
}

// 0.5 |c|
__host__ __device__ inline float emitter_area(const float* c) {
    return 0.5f * __builtin_sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
}

// The weight of an emitting triangle: area x luminance of its entry's emission (Rec. 709).
__host__ __device__ inline float emitter_weight(const float* xyz, const float* emission) {
    float c[3];
    emitter_cross(xyz, c);
    const float lum = 0.2126f * emission[0] + 0.7152f * emission[1] + 0.0722f * emission[2];
    return emitter_area(c) * lum;
}

// The slot a random number r in [0, 1) selects from the inclusive CDF of `count` >= 1 weights: the first
// whose CDF value is >= r * total, total = cdf[count - 1]; the search ends inside [0, count - 1] for any
// r.  prob: the share the CDF gives that slot, (cdf[k] - cdf[k - 1]) / total.  (The reference's
// BinarySearch(..) + 1 over the sky CDF never returns entry 0; a list with one emitter has only that.)
__host__ __device__ inline uint32_t emitter_select(const float* cdf, uint32_t count, float r, float& prob) {
    const float total = cdf[count - 1u];
    const float target = r * total;
    uint32_t lo = 0u, hi = count - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2u;
        if (cdf[mid] >= target) hi = mid;
        else lo = mid + 1u;
    }
    const float below = lo > 0u ? cdf[lo - 1u] : 0.0f;
    prob = (cdf[lo] - below) / total;
    return lo;
}

constexpr uint32_t kEmScanBlock = 256;       // the reference Scan's block (rtk_launch_scan)
constexpr uint32_t kEmMaxTris = 1u << 20;    // a queue entry's light index has 24 bits; the scan 8192 blocks
// header words of a list (EmitterListParams::header)
enum EmHeader : int { kEmCount = 0, kEmTotal = 1, kEmHeaderWords = 4 };

// the CDF's length for a build of triCount triangles: the power of two >= max(triCount, kEmScanBlock)
inline uint32_t emitter_cdf_len(uint32_t triCount) {
    uint32_t p = kEmScanBlock;
    while (p < triCount) p <<= 1;
    return p;
}

// One list build (emitters.hip), behind the LBVH build whose triangle records it reads.
struct EmitterListParams {
    const float4* triPos;      // the build's triangle records (traverse.h): triangle t at triPos + 4 t
    const uint8_t* triMat;     // material id per triangle, or null: 3 everywhere
    const float4* matTable;    // [256 * kMatRecVecs] the custom material table
    int materialOverride;      // >= 0: that id for every triangle
    uint32_t triCount;         // <= kEmMaxTris
    uint32_t cdfLen;           // emitter_cdf_len(triCount)
    float* triWeight;          // scratch [cdfLen]: every triangle's weight, 0 for one that is no emitter
    uint32_t* blockCount;      // scratch [cdfLen / 256 + 1]: emitters per 256 triangles, then their offsets
    uint32_t* tris;            // out [triCount]: the emitters' triangle indices, ascending
    float* weights;            // out [cdfLen]: weights[slot], 0 from the count up
    float* cdf;                // out [cdfLen]: the inclusive scan of weights
    float* scanSums;           // scratch [cdfLen / 256]
    uint32_t* header;          // out [kEmHeaderWords]: count, bits of cdf[count - 1] (0 for an empty list)
};
extern "C" hipError_t rtk_launch_emitter_list(const EmitterListParams* p, hipStream_t stream);
