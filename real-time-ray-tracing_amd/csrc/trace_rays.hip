// trace_rays.hip — device ray queries (rt_trace_rays_device) for gfx950: the
// persistent dynamic-fetch tracer of trace_queue.hip restated for caller memory.
//
// A lane loads its ray straight from the caller's origin and direction arrays (any stride of at
// least three floats, three dword loads each: no 16-B alignment is assumed) and writes its record
// as one 16-B store into the caller's hit array.  Nothing of the path tracer's workspace is touched:
// no queue-3 staging, no hitErr, no statistics atomics, no shading list; the fetch counters are a
// block of the query's own (RayQueryParams::fetch, zeroed on the stream ahead of the launch).
//
// The traversal is traverse.h's, one TraverseBvh iteration per trav_step call, with the refill rule
// (kRefillMin), the two-steps-per-trip loop, the tail mode and the 1024-iteration cap of
// k_trace_queue: a closest-hit record and its iteration count are k_trace_queue<3>'s for the same
// ray, bit for bit.  kAnyHit: a ray ends at the iteration in which the traversal first records a hit
// (k_trace_queue's `occlusion && s.hitIdx >= 0` exit), and the record is that hit.
//
// Block shape: 256 threads with a 17-slot LDS stack column per thread (34,816 B per workgroup), as
// k_trace_queue: four workgroups fit a CU's 160 KiB of LDS, and the grid stays at the queue tracers'
// tracePerCu below that, so a query leaves the CUs room for the frames' waves beside it.
//
// No s_setprio: the query is a guest beside the frames, whose tracers raise their own priority.
// Whether a raised priority would help a query that runs alone or beside a frame has not been
// measured.
#include "frame_kernels.h"
#include "queue_fetch.h"
#include "traverse.h"

using namespace rtd;

namespace {

constexpr int kQueryBlock = 256;
#ifndef RTX_LEAF_BATCH
#define RTX_LEAF_BATCH 1
#endif
constexpr bool kLeafBatch = RTX_LEAF_BATCH != 0;  // ablation: -DRTX_LEAF_BATCH=0, as trace_queue.hip

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

    bool active = false, exhausted = false;
    uint32_t idx = 0;
    TravRay r;
    TravState s;
    TravRec rec;  // the record the lane's next iteration processes
    r.org = f3(0.0f);
    trav_init(s, sc.root);
#pragma unroll 1
    while (true) {
        const unsigned long long need = __ballot(!active && !exhausted);
        const unsigned long long busy = __ballot(active);
        if (need != 0ull && (__popcll(need) >= kRefillMin || busy == 0ull)) {
            const uint32_t k = (uint32_t)__popcll(need);
            fetch_topup(f, n, P.fetch, lane);
            const uint32_t avail = f.resHi - f.resLo;
            const bool none = avail == 0u && f.drained == (1u << kParts) - 1u;
            if (!active && !exhausted) {
                const uint32_t rank = (uint32_t)__popcll(need & ((1ull << lane) - 1ull));
                if (rank < avail) {
                    idx = f.resLo + rank;  // < n <= RT_QUERY_MAX_RAYS
                    const float* o = P.org + (size_t)idx * P.orgStride;
                    const float* d = P.dir + (size_t)idx * P.dirStride;
                    trav_setup(sc, f3(o[0], o[1], o[2]), f3(d[0], d[1], d[2]), r);
                    trav_init(s, sc.root);
                    rec = trav_first_rec(sc);
                    active = true;
                } else if (none) {
                    exhausted = true;
                }
            }
            f.resLo += k < avail ? k : avail;
        }
        if (__ballot(active) == 0ull) break;
        // Tail: this wave's reserve is empty and every part drained, so no lane can be refilled; the
        // remaining rays run in a plain per-lane loop (trace_queue.hip).  Each ray's steps are unchanged.
        const bool tail = f.resLo == f.resHi && f.drained == (1u << kParts) - 1u;
        if (tail || !kLeafBatch ? active : trav_lane_steps(active, s)) {
            bool done;
            do {  // two steps per trip
                done = trav_step<16, true, false>(sc, r, s, rec, stk + tid, kQueryBlock, nullptr) || s.iters >= 1024u ||
                       (kAnyHit && s.hitIdx >= 0);
                if (!done && (tail || !kLeafBatch || trav_lane_steps(true, s)))
                    done = trav_step<16, true, false>(sc, r, s, rec, stk + tid, kQueryBlock, nullptr) || s.iters >= 1024u ||
                           (kAnyHit && s.hitIdx >= 0);
            } while (tail && !done);
            if (done) {
                P.hits[idx] = make_float4(s.t, __uint_as_float((uint32_t)s.hitIdx), s.hitU, s.hitV);
                if (kIters) P.iters[idx] = s.iters;
                active = false;
            }
        }
    }
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
