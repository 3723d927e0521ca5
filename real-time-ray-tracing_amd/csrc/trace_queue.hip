// trace_queue.hip — persistent tracer of a deferred-ray queue (wavefront path tracing,
// DESIGN.md §4) for gfx950.
//
// The bounce and shadow rays leaving a surface are incoherent: inside one wave64 their
// traversals differ in length by an order of magnitude, and the single-kernel path tracer
// kept every lane of a wave waiting for its longest ray at 2 waves/SIMD.  Here a lean kernel
// (traversal state only) runs at 5 waves/SIMD, and each wave refills its idle lanes from the
// queue (one atomic per 64 rays, see Fetch) so lanes stay busy until the queue is drained
// (Aila & Laine 2009, persistent threads with dynamic fetch).
//
// The loop is queue_trace.h's; this file supplies where a queue entry's ray comes from, where its
// record goes and the shading list of queue 3.  Each lane runs TraverseBvh (traverse.h:107-253)
// one iteration per trav_step call, so the reference semantics — 16-entry LDS stack with dropped
// overflow pushes, nearer child first, 1024-iteration cap — hold per ray exactly as in the inline
// traversal.
#include "queue_trace.h"

using namespace rtd;

namespace {

constexpr int kTraceBlock = 256;
constexpr uint32_t kTrace3Short = 1u << 20;  // queue-3 length below which trace3ShortBlocks apply

// A wave's pending entries of the shading list (PtWorkspace::shade3) go out n <= 64 at a time: one
// atomic per flush, and the wave waits for its return once per ~64 listed entries.  (One atomic per
// loop trip that finished a listed ray, ~47 k on one address with every wave waiting for each of
// its own, stretched trace<3> 248 -> 380 us in the pipeline.)  Wave-uniform call; the wave's LDS
// accesses execute in order, the fences keep the compiler from reordering them.
RT_DEV void flush_shade_list(const PathTraceParams& P, uint32_t* shl, uint32_t n, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    uint32_t base = 0u;
    if (lane == 0) base = atomicAdd(&P.ws.counters[kCntShade3], n);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if ((uint32_t)lane < n) P.ws.shade3[base + (uint32_t)lane] = shl[lane];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// kStats: the launch keeps per-pixel statistics (P.statsOut), so the traversal counts visits and tests
// kClosest (queue 4 under a custom material table with an emitter, PtWorkspace::closest4): a bounce
// ray's traversal runs to its closest hit, since which triangle it lands on decides the sample's colour
// kNee (emitter sampling, PathTraceParams::emHeader): a shadow ray that samples an emitter (kQEmitterFlag)
// runs to its closest hit too, in both queues: the first hit of a BVH-ordered traversal may be the light
// behind an occluder, or an occluder behind the light
template <int kStep, bool kStats, bool kClosest = false, bool kNee = false>
__global__ __launch_bounds__(kTraceBlock) void k_trace_queue(PathTraceParams P) {
    __shared__ uint2 stk[17 * kTraceBlock];  // 16 entries + the dead slot trav_step stores above the top
    __shared__ uint32_t shadeList[kStep == 3 ? kTraceBlock : 1];  // per wave: 64 pending shading-list entries
    // The tracers' waves issue at the denoise kernels' priority (DN_PRIO), above the next frame's
    // camera waves: in a pipelined frame the context stream binds (bench.py binding_stream), and its
    // queue tracers' time is their longest rays' dependent iterations, which stretch when the SIMD
    // arbiter serves the camera waves first.  Measured (tools/ab.sh, three repeats): frame
    // 0.803-0.811 -> 0.782-0.792 ms, trace<3> 0.287 -> 0.244 ms, trace<4> 0.203 -> 0.166 ms, terrain
    // 3.20-3.24 -> 3.16-3.21 ms; trace<4> alone at 3: 0.785-0.790; both at 2: 0.799-0.802; the resume
    // kernels at 3 on top: no better (profiles/r05_ab/queue_prio/).  (Round 4, with the shade kernel
    // at 2 waves per SIMD and the post stream binding, the same measured slower.)
    __builtin_amdgcn_s_setprio(3);
    const int tid = threadIdx.x;
    const int lane = (int)__lane_id();
    const PtQueue& q = kStep == 3 ? P.ws.q3 : P.ws.q4;
    const uint32_t n = P.ws.counters[kStep == 3 ? kCntQ3 : kCntQ4];
    uint32_t* fetchCounters = P.ws.fetch + (kStep == 3 ? 0 : kParts * 16);
    const SceneView sc = scene_of(P);

    // a short queue 3 runs on the first trace3ShortBlocks workgroups only (frame.cpp); the others
    // leave before taking any work, and the static first batches are cut over the ones that stay
    uint32_t blocks = gridDim.x;
    if (kStep == 3 && P.ws.trace3ShortBlocks != 0u && n < kTrace3Short && P.ws.trace3ShortBlocks < blocks)
        blocks = P.ws.trace3ShortBlocks;
    if (blockIdx.x >= blocks) return;
    const uint32_t wavesPerBlock = kTraceBlock / 64;
    Fetch f;
    fetch_init(f, n, blocks * wavesPerBlock, blockIdx.x * wavesPerBlock + (uint32_t)(tid >> 6));

    uint32_t accV = 0, accT = 0;
    uint32_t* const shl = shadeList + (kStep == 3 ? (tid & ~63) : 0);  // this wave's
    uint32_t nList = 0;  // wave-uniform
    queue_trace<kStats, true, true>(
        sc, f, stk + tid, kTraceBlock,
        [&] { fetch_topup(f, n, fetchCounters, lane); },
        [&] { return fetch_drained(f); },
        [&](uint32_t idx, TravRay& r) {
            const float4 o = q.rayO[idx], d = q.rayD[idx];
            trav_setup(sc, f3(o.x, o.y, o.z), f3(d.x, d.y, d.z), r);
            bool occlusion = (kStep == 4 && !kClosest) || (__float_as_uint(d.w) & kQShadowFlag) != 0u;
            if constexpr (kNee) occlusion = occlusion && (__float_as_uint(d.w) & kQEmitterFlag) == 0u;
            return occlusion;
        },
        [&](uint32_t idx, const TravState& s) {
            (kStep == 3 ? P.ws.hitRec : P.ws.hitRec4)[idx] = hit_record(s);
            (kStep == 3 ? P.ws.hitErr : P.ws.hitErr4)[idx] = s.hitErrT;
            if (P.ws.itersOut) P.ws.itersOut[idx] = s.iters;
            if (P.statsOut) {
                const uint32_t p = __float_as_uint(q.rayO[idx].w);
                atomicAdd(&P.statsOut[p].y, s.visits);
                atomicAdd(&P.statsOut[p].z, s.tests);
                atomicMax(&P.ws.counters[kStep == 3 ? kCntMaxIter3 : kCntMaxIter4], s.iters);
                accV += s.visits;
                accT += s.tests;
            }
        },
        // the entries whose resume may shade go to the shading list (split resume<3>); wave-uniform flow
        [&](bool fin, bool occlusion, uint32_t idx, const TravState& s) {
            if (kStep == 3 && P.ws.shade3) {
                const unsigned long long m = __ballot(fin && q3_shades(occlusion ? kQShadowFlag : 0u, (uint32_t)s.hitIdx));
                if (m != 0ull) {
                    const uint32_t k = (uint32_t)__popcll(m);
                    if (nList + k > 64u) {
                        flush_shade_list(P, shl, nList, lane);
                        nList = 0u;
                    }
                    if ((m >> lane) & 1ull) shl[nList + lane_rank(m)] = idx;
                    nList += k;
                }
            }
        });
    if (kStep == 3 && P.ws.shade3 && nList) flush_shade_list(P, shl, nList, lane);
    if (P.statsOut) {  // every lane left the loop together
        wave_add(accV, &P.ws.counters[kStep == 3 ? kCntVisQ3 : kCntVisQ4]);
        wave_add(accT, &P.ws.counters[kStep == 3 ? kCntTstQ3 : kCntTstQ4]);
    }
}

}  // namespace

extern "C" int rtk_trace_queue_blocks_per_cu() {
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_trace_queue<3, false>, kTraceBlock, 0) != hipSuccess) return 0;
    return b;
}

extern "C" hipError_t rtk_launch_trace_queue(const PathTraceParams* p, int step, hipStream_t stream) {
    const uint32_t blocks = step == 3 ? p->ws.traceBlocks : p->ws.trace4Blocks;
    if (blocks < 1) return hipErrorInvalidValue;
    const dim3 grid(blocks);
    const bool stats = p->statsOut != nullptr;
    void (*k)(PathTraceParams) = step == 3 ? (stats ? k_trace_queue<3, true> : k_trace_queue<3, false>)
                                           : (stats ? k_trace_queue<4, true> : k_trace_queue<4, false>);
    if (step == 4 && p->ws.closest4) k = stats ? k_trace_queue<4, true, true> : k_trace_queue<4, false, true>;
    if (p->emHeader) {  // emitter sampling: with a custom table that emits, so queue 4 is a closest-hit queue already
        if (!p->ws.closest4) return hipErrorInvalidValue;
        k = step == 3 ? (stats ? k_trace_queue<3, true, false, true> : k_trace_queue<3, false, false, true>)
                      : (stats ? k_trace_queue<4, true, true, true> : k_trace_queue<4, false, true, true>);
    }
    hipLaunchKernelGGL(k, grid, dim3(kTraceBlock), 0, stream, *p);
    return hipGetLastError();
}
