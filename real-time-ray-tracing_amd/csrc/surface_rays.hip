// surface_rays.hip — the surface pass of device ray queries (rt_trace_surfaces_device, DESIGN.md
// §4.1.1a) for gfx950: hit position, ray offset, geometric and shading normal, material id and the
// hit point's displacement, from a ray and its 16-B hit record.
//
// The record is a pure function of (origin, direction, t, triangle, u, v) and the LBVH set: the one
// input of finalize_hit (traverse.h) that a hit record does not carry, hitErrT, is
// err_gamma(16) * fabsf(t) (watertight), restated here.  So the pass calls finalize_hit as it stands,
// on the records of any tracer, and is a dense kernel of its own: one thread per ray, no LDS, no
// atomics, no loop.  A persistent tracer variant would have carried 12..16 more output registers and
// the normals' gathers through the traversal loop, whose occupancy the registers set.
//
// Memory: per ray 40 B of contiguous input (two xyz triples at the caller's strides, three dword
// loads each as k_trace_rays, and the record as one 16-B load) and 48 B (64 B with motion) of
// output, each quad one 16-B store; a wave's three (four) stores together cover whole lines.  Per
// hit the gathers: the 48 B of the triangle record, 48 B of normals, one id byte, with motion 48 B
// of displacements, all in 16-B loads.  A record whose index lies outside [0, triCountPadded) reads
// nothing from the set and is finished as a miss.
//
// No s_setprio: the pass runs behind the query's tracer, a guest beside the frames like it.
#include "frame_kernels.h"
#include "traverse.h"

using namespace rtd;

namespace {

constexpr int kSurfaceBlock = 256;

template <bool kMotion>
__global__ __launch_bounds__(kSurfaceBlock) void k_ray_surface(RaySurfaceParams P) {
    const uint32_t i = blockIdx.x * (uint32_t)kSurfaceBlock + threadIdx.x;  // < 2^22 * 256 + 256
    if (i >= P.n) return;
    const SceneView sc = scene_view(P.nodes, P.tlasNodes, P.triPos, P.triNrm);
    const float* o = P.org + (size_t)i * P.orgStride;
    const float* d = P.dir + (size_t)i * P.dirStride;
    const F3 org = f3(o[0], o[1], o[2]), dir = f3(d[0], d[1], d[2]);
    const float4 rec = P.hits[i];
    float t = rec.x;
    int idx = (int)__float_as_uint(rec.y);
    if ((uint32_t)idx >= P.triCountPadded) {  // -1, or anything else that is no record of the set
        t = kRayMax;
        idx = -1;
    }
    HitInfo h;
    finalize_hit(sc, org, dir, t, idx, rec.z, rec.w, err_gamma(16) * fabsf(t), h);
    uint32_t word = 0u;
    F3 disp = f3(0.0f);
    if (h.hit && idx >= 0) {
        // the id the path tracer reads for this triangle (update_material, pathtrace.hip)
        const int id = P.materialOverride >= 0 ? P.materialOverride
                       : (uint32_t)idx < P.triCount ? (P.triMat ? (int)P.triMat[idx] : 3) : 6;
        word = ((uint32_t)id & 0xFFFFu) | (h.into ? 1u << 16 : 0u) | 1u << 17;
        if (kMotion && P.triDisp) {  // interpolated as k_pt_geom_motion interpolates it
            const F3 d1 = f3_of(P.triDisp[3 * idx]), d2 = f3_of(P.triDisp[3 * idx + 1]), d3 = f3_of(P.triDisp[3 * idx + 2]);
            disp = d3 * (1.0f - rec.z - rec.w) + d1 * rec.z + d2 * rec.w;
        }
    }
    float4* out = P.surface + (size_t)i * (kMotion ? 4u : 3u);
    out[0] = make_float4(h.pos.x, h.pos.y, h.pos.z, h.offset);
    out[1] = make_float4(h.normal.x, h.normal.y, h.normal.z, h.ndr);
    out[2] = make_float4(h.fakeNormal.x, h.fakeNormal.y, h.fakeNormal.z, __uint_as_float(word));
    if (kMotion) out[3] = make_float4(disp.x, disp.y, disp.z, 0.0f);
}

}  // namespace

extern "C" hipError_t rtk_launch_ray_surface(const RaySurfaceParams* p, int motion, hipStream_t stream) {
    if (p->n == 0u || p->n > RT_QUERY_MAX_RAYS) return hipErrorInvalidValue;
    const dim3 grid((p->n + kSurfaceBlock - 1u) / kSurfaceBlock);
    void (*k)(RaySurfaceParams) = motion ? k_ray_surface<true> : k_ray_surface<false>;
    hipLaunchKernelGGL(k, grid, dim3(kSurfaceBlock), 0, stream, *p);
    return hipGetLastError();
}
