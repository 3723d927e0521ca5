// trace_rays.hip — device ray queries (rt_trace_rays_device) for gfx950: the
// persistent dynamic-fetch tracer for caller memory.  It uses the queue tracers' loop (queue_trace.h).
//
// A lane loads its ray straight from the caller's origin and direction arrays (any stride of at
// least three floats, three dword loads each: no 16-B alignment is assumed) and writes its record
// as one 16-B store into the caller's hit array.  Nothing of the path tracer's workspace is touched:
// no queue-3 staging, no hitErr, no statistics atomics, no shading list; the fetch counters are a
// block of the query's own (RayQueryParams::fetch, zeroed on the stream ahead of the launch).
//
// The loop is k_trace_queue's own (queue_trace: refill rule, two steps per trip, tail mode, 1024-
// iteration cap), so a closest-hit record and its iteration count are k_trace_queue<3>'s for the
// same ray, bit for bit.  kAnyHit: a ray ends at the iteration in which the traversal first records
// a hit (an occlusion ray's exit, trav_done), and the record is that hit.
//
// Block shape: 256 threads with a 17-slot LDS stack column per thread (34,816 B per workgroup), as
// k_trace_queue: four workgroups fit a CU's 160 KiB of LDS, and the grid stays at the queue tracers'
// tracePerCu below that, so a query leaves the CUs room for the frames' waves beside it.
//
// No s_setprio: the query is a guest beside the frames, whose tracers raise their own priority.
// Whether a raised priority would help a query that runs alone or beside a frame has not been
// measured.
#include "queue_trace.h"

using namespace rtd;

namespace {

constexpr int kQueryBlock = 256;

template <bool kAnyHit, bool kIters>
__global__ __launch_bounds__(kQueryBlock) void k_trace_rays(RayQueryParams P) {
    __shared__ uint2 stk[17 * kQueryBlock];  // 16 entries + the dead slot trav_step stores above the top
    const int tid = threadIdx.x;
    const int lane = (int)__lane_id();
    const uint32_t n = P.n;
    const SceneView sc = scene_view(P.nodes, P.tlasNodes, P.triPos, nullptr);

    const uint32_t wavesPerBlock = kQueryBlock / 64;
    Fetch f;
    fetch_init(f, n, gridDim.x * wavesPerBlock, blockIdx.x * wavesPerBlock + (uint32_t)(tid >> 6));

    queue_trace<false, true, true>(
        sc, f, stk + tid, kQueryBlock,
        [&] { fetch_topup(f, n, P.fetch, lane); },
        [&] { return fetch_drained(f); },
        [&](uint32_t idx, TravRay& r) {  // idx < n <= RT_QUERY_MAX_RAYS
            const float* o = P.org + (size_t)idx * P.orgStride;
            const float* d = P.dir + (size_t)idx * P.dirStride;
            trav_setup(sc, f3(o[0], o[1], o[2]), f3(d[0], d[1], d[2]), r);
            return kAnyHit;
        },
        [&](uint32_t idx, const TravState& s) {
            P.hits[idx] = hit_record(s);
            if (kIters) P.iters[idx] = s.iters;
        },
        [](bool, bool, uint32_t, const TravState&) {});
}

}  // namespace

extern "C" hipError_t rtk_launch_trace_rays(const RayQueryParams* p, uint32_t maxBlocks, int anyHit, hipStream_t stream) {
    if (p->n == 0u || maxBlocks < 1u) return hipErrorInvalidValue;
    const uint32_t want = (p->n + kQueryBlock - 1u) / kQueryBlock;
    const dim3 grid(want < maxBlocks ? want : maxBlocks);
    const bool iters = p->iters != nullptr;
    void (*k)(RayQueryParams) = anyHit ? (iters ? k_trace_rays<true, true> : k_trace_rays<true, false>)
                                       : (iters ? k_trace_rays<false, true> : k_trace_rays<false, false>);
    hipLaunchKernelGGL(k, grid, dim3(kQueryBlock), 0, stream, *p);
    return hipGetLastError();
}
