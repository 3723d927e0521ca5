// queue_trace.h — the persistent tracers' work distribution (Fetch) and their one refilling
// traversal loop (queue_trace), DESIGN.md §4.1.  Users: k_trace_queue (trace_queue.hip), the ray
// queries' k_trace_rays (trace_rays.hip) and phase 1 of the fused bounce chain (pathtrace.hip).
#pragma once
#include "frame_kernels.h"
#include "traverse.h"

namespace rtd {

#ifndef RTX_REFILL_MIN
#define RTX_REFILL_MIN 16
#endif
constexpr int kRefillMin = RTX_REFILL_MIN;  // idle lanes that trigger a refill (ablation: -DRTX_REFILL_MIN)
#ifndef RTX_LEAF_BATCH
#define RTX_LEAF_BATCH 1
#endif
constexpr bool kLeafBatch = RTX_LEAF_BATCH != 0;  // trav_lane_steps in the loop (ablation: -DRTX_LEAF_BATCH=0)
constexpr int kParts = 8;       // fetch counters (one per XCD by blockIdx % 8): spreads the atomics

RT_DEV SceneView scene_of(const PathTraceParams& P) { return scene_view(P.nodes, P.tlasNodes, P.triPos, P.triNrm); }

// Work distribution.  Wave g first takes items [64 g, 64 g + 64) with no atomic: a short queue
// (a sky-dominated frame) costs no atomics at all.  The rest, [64 * waves, n), is cut into
// kParts contiguous parts; a wave tops up a 64-item reserve from its home part (one atomic per
// 64 items), moving on to the next part when its home part is drained.  A same-address
// device-scope atomic serialises at the memory side, so both the static first batch and the
// per-part counters keep the queue of atomics on any one address short.
struct Fetch {
    uint32_t resLo, resHi;  // wave-uniform reserve [resLo, resHi)
    uint32_t dynBase, partLen;
    uint32_t drained;       // bit x: part x has no items left
    int home;
};

// staticFirst = false: no static first batch, every item is fetched (a workgroup dispatched
// late, behind other kernels' waves, then holds back no items)
RT_DEV void fetch_init(Fetch& f, uint32_t n, uint32_t wavesTotal, uint32_t gw, bool staticFirst = true) {
    const uint32_t s0 = staticFirst ? gw * 64u : 0u;
    f.resLo = staticFirst && s0 < n ? s0 : n;
    f.resHi = staticFirst ? (s0 + 64u < n ? s0 + 64u : n) : n;
    f.dynBase = staticFirst ? wavesTotal * 64u : 0u;
    const uint32_t dyn = n > f.dynBase ? n - f.dynBase : 0u;
    f.partLen = (dyn + kParts - 1) / kParts;
    f.drained = dyn == 0u ? (1u << kParts) - 1u : 0u;
    f.home = (int)(blockIdx.x % kParts);
}

// every part has no items left: an empty reserve stays empty
RT_DEV bool fetch_drained(const Fetch& f) { return f.drained == (1u << kParts) - 1u; }

// refill an empty reserve from the first part that still has items (wave-uniform call)
RT_DEV void fetch_topup(Fetch& f, uint32_t n, uint32_t* counters, int lane) {
    while (f.resLo == f.resHi && !fetch_drained(f)) {
        int part = f.home;
        while (f.drained & (1u << part)) part = (part + 1) % kParts;
        uint32_t got = 0u;
        if (lane == 0) got = atomicAdd(&counters[part * 16], 64u);  // counters 64 B apart
        got = __shfl(got, 0);
        const uint32_t lo = f.dynBase + part * f.partLen + got;
        uint32_t hi = f.dynBase + part * f.partLen + (got + 64u < f.partLen ? got + 64u : f.partLen);
        if (hi > n) hi = n;
        if (got >= f.partLen || lo >= hi) {
            f.drained |= 1u << part;
            continue;
        }
        f.resLo = lo;
        f.resHi = hi;
    }
}

// The refilling traversal loop: every lane of the wave runs its own ray, one TraverseBvh iteration
// per trav_step call, and once kRefillMin lanes are idle (or all are) the idle lanes take the next
// items of the wave's reserve, in lane order.  A lane becomes `exhausted` once the reserve is empty
// and stuck() says it stays so; the wave returns when no lane holds a ray, which every wave reaches
// because the fetch counters only grow and every ray ends within 1024 iterations.  Wave-uniform
// call; stk is the thread's column of a 17-slot LDS stack (16 entries + the dead slot trav_step
// stores above the top), `stride` columns wide.
//
// What differs between the users comes in as callables:
//   topup()                   wave-uniform: refill f's reserve if it is empty and may be refilled
//   stuck()                   wave-uniform: an empty reserve can no longer be refilled
//   load(idx, r)              set the ray of item idx up (trav_setup); returns whether it stops at its first hit
//   finish(idx, s)            the stores of item idx's finished traversal
//   trip(fin, firstHit, idx, s)  wave-uniform, once per loop trip; fin: the lane finished item idx in this trip
// kCarry: trav_step's (the next record is carried between iterations: 14 more registers).
// kTwoSteps: two steps per trip, so the refill and exec-mask bookkeeping runs once per two.
//
// Tail: once the reserve is empty and stuck, no lane can be refilled.  The remaining rays then run
// in a plain per-lane loop, without the refill ballots and the leaf batching (a wave in the tail
// has few lanes left, and its iteration latency is the kernel's tail).  Each ray's steps are the
// same in either mode, and so are its record, counters and 1024-iteration cap.
template <bool kStats, bool kCarry, bool kTwoSteps, class Topup, class Stuck, class Load, class Finish, class Trip>
RT_DEV void queue_trace(const SceneView& sc, Fetch& f, uint2* stk, int stride, Topup topup, Stuck stuck, Load load,
                        Finish finish, Trip trip) {
    bool active = false, exhausted = false, firstHit = false;
    uint32_t idx = 0;
    TravRay r;
    TravState s;
    TravRec rec;  // kCarry: the record the lane's next iteration processes; else trav_step's scratch
    r.org = f3(0.0f);
    trav_init(s, sc.root);
    const auto step = [&] { return trav_done(trav_step<16, kCarry, kStats>(sc, r, s, rec, stk, stride, nullptr), s, firstHit); };
#pragma unroll 1
    while (true) {
        const unsigned long long need = __ballot(!active && !exhausted);
        const unsigned long long busy = __ballot(active);
        if (need != 0ull && (__popcll(need) >= kRefillMin || busy == 0ull)) {
            const uint32_t k = (uint32_t)__popcll(need);
            topup();
            const uint32_t avail = f.resHi - f.resLo;
            const bool none = avail == 0u && stuck();
            if (!active && !exhausted) {
                const uint32_t rank = lane_rank(need);
                if (rank < avail) {
                    idx = f.resLo + rank;
                    firstHit = load(idx, r);
                    trav_init(s, sc.root);
                    if (kCarry) rec = trav_first_rec(sc);
                    active = true;
                } else if (none) {
                    exhausted = true;
                }
            }
            f.resLo += k < avail ? k : avail;
        }
        if (__ballot(active) == 0ull) break;
        const bool tail = f.resLo == f.resHi && stuck();
        bool fin = false;
        if (tail || !kLeafBatch ? active : trav_lane_steps(active, s)) {
            bool done;
            do {
                done = step();
                if constexpr (kTwoSteps)
                    if (!done && (tail || !kLeafBatch || trav_lane_steps(true, s))) done = step();
            } while (tail && !done);
            if (done) {
                finish(idx, s);
                active = false;
                fin = true;
            }
        }
        trip(fin, firstHit, idx, s);
    }
}

}  // namespace rtd
