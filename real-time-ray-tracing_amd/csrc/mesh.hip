// mesh.hip — run-time mesh replacement for gfx950 (rt_set_mesh / rt_set_mesh_device): the caller's
// index array into the context's, and the vertex -> corner adjacency the normals kernels
// (geometry.hip, trace_primary.hip) read, built on the device.  rt_mesh_adjacency (context.cpp) is
// the definition: corner c gets slot  adjOff[idx[c]] + #{c' < c : idx[c'] == idx[c]}.
//
//   k_mesh_ingest   one thread per padded corner: copy, pad with 0, an index >= nverts read as 0
//                   and counted (one integer atomic per wave that saw one)
//   k_mesh_report   one thread: the count, if any, to the host's status word, and the counter re-armed
//   per 8-bit digit of the vertex id, lowest first (a stable LSD radix sort of the corners, which
//   start in ascending order, by vertex):
//     k_mesh_hist     a workgroup per tile: the tile's count of each digit (LDS integer atomics:
//                     only their totals are used) into table[digit][tile]
//     k_mesh_scan     a workgroup per digit: its row's exclusive prefix sums over the tiles in
//                     place, and the row's total into totals[digit]
//     k_mesh_scatter  a workgroup per tile, 512 keys a round.  It scans the 256 totals itself, so
//                     that totals'[d] + table[d][tile] is where the tile's first key of digit d
//                     goes; a key's place is that running offset of its digit, plus the counts of
//                     the waves before its own in this round (through LDS, in wave order), plus
//                     its rank among its wave's lanes of that digit (ballots); the last pass also
//                     writes the inverse, corner -> slot
//   k_mesh_offsets  one thread per vertex: adjOff[v] = the first slot whose sorted key is >= v, a
//                   binary search (empty runs and the end, adjOff[nverts] = 3 NP, fall out of it)
//
// Every step is a launch of its own on one stream: no workgroup waits for another, nothing spins.
// No result depends on the order atomics land in, there is no float arithmetic, and the work per
// key does not depend on the keys: a fan of a million triangles around one vertex costs what any
// mesh of that size costs.  The passes cover the bits of nverts - 1 only.
#include "bvh_kernels.h"
#include "rt_device.h"

using namespace rtd;

namespace {

constexpr uint32_t kThr = kMeshSortThreads, kWaves = kThr / 64, kDigits = 256;

struct SortPass {
    const uint32_t* keysIn;
    const uint32_t* valsIn;  // null: the key's own position (the first pass: corner c at c)
    uint32_t* keysOut;
    uint32_t* valsOut;
    uint32_t* slotOut;       // optional: slotOut[val] = the key's place (the last pass)
    uint32_t* table;         // [kDigits][tiles]
    uint32_t* totals;        // [kDigits] keys of each digit
    uint32_t n, tileLen, tiles, shift;
};

RT_DEV uint32_t digit_of(uint32_t key, uint32_t shift) { return (key >> shift) & (kDigits - 1u); }

// s[0 .. 256) in LDS to its inclusive prefix sums, in place; called by every thread of the workgroup
RT_DEV void scan256(uint32_t* s, uint32_t t) {
    for (uint32_t d = 1u; d < kDigits; d <<= 1) {
        const uint32_t v = (t < kDigits && t >= d) ? s[t - d] : 0u;
        __syncthreads();
        if (t < kDigits) s[t] += v;
        __syncthreads();
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_mesh_ingest(MeshSetParams P) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    const uint32_t n = 3u * P.triCountPadded;
    uint32_t v = c < 3u * P.triCount ? P.srcIndices[c] : 0u;
    const bool bad = v >= P.nverts;  // nverts >= 1: the padding's 0 is never bad
    if (bad) v = 0u;
    if (c < n) P.indices[c] = v;
    const unsigned long long b = __ballot(bad);
    if ((threadIdx.x & 63u) == 0u && b != 0ull) atomicAdd(P.badCount, (uint32_t)__popcll(b));
}

__global__ void k_mesh_report(uint32_t* badCount, uint32_t* status) {
    const uint32_t c = *badCount;
    if (c) {
        report_status(status, kStatusMeshBadIndices, c);
        *badCount = 0u;
    }
}

__global__ __launch_bounds__(kMeshSortThreads) void k_mesh_hist(SortPass P) {
    __shared__ uint32_t h[kDigits];
    const uint32_t t = threadIdx.x, tile = blockIdx.x;
    if (t < kDigits) h[t] = 0u;
    __syncthreads();
    const uint32_t begin = tile * P.tileLen, end = begin + P.tileLen < P.n ? begin + P.tileLen : P.n;
    for (uint32_t i = begin + t; i < end; i += kThr) atomicAdd(&h[digit_of(P.keysIn[i], P.shift)], 1u);
    __syncthreads();
    if (t < kDigits) P.table[t * P.tiles + tile] = h[t];
}

// digit blockIdx.x's row of the table (tiles <= 256 = the workgroup's threads, one tile each)
__global__ __launch_bounds__(256) void k_mesh_scan(uint32_t* table, uint32_t tiles, uint32_t* totals) {
    __shared__ uint32_t s[kDigits];
    const uint32_t t = threadIdx.x, d = blockIdx.x;
    const uint32_t v = t < tiles ? table[d * tiles + t] : 0u;
    s[t] = v;
    __syncthreads();
    scan256(s, t);
    if (t < tiles) table[d * tiles + t] = s[t] - v;
    if (t == kDigits - 1u) totals[d] = s[t];
}

__global__ __launch_bounds__(kMeshSortThreads) void k_mesh_scatter(SortPass P) {
    __shared__ uint32_t running[kDigits];      // where the tile's next key of each digit goes
    __shared__ uint32_t cnt[kWaves][kDigits];  // this round's keys of each digit per wave; zero between rounds
    const uint32_t t = threadIdx.x, w = t >> 6, lane = t & 63u, tile = blockIdx.x;
    const uint32_t total = t < kDigits ? P.totals[t] : 0u;
    if (t < kDigits) running[t] = total;
    for (uint32_t k = t; k < kWaves * kDigits; k += kThr) (&cnt[0][0])[k] = 0u;
    __syncthreads();
    scan256(running, t);  // the keys of the digits up to t; each thread then rewrites its own word
    if (t < kDigits) running[t] = running[t] - total + P.table[t * P.tiles + tile];
    __syncthreads();
    const uint32_t begin = tile * P.tileLen, end = begin + P.tileLen < P.n ? begin + P.tileLen : P.n;
    for (uint32_t base = begin; base < end; base += kThr) {  // uniform over the workgroup
        const uint32_t i = base + t;
        const bool valid = i < end;
        const uint32_t key = valid ? P.keysIn[i] : 0u;
        const uint32_t val = valid ? (P.valsIn ? P.valsIn[i] : i) : 0u;
        const uint32_t d = digit_of(key, P.shift);
        // the valid lanes of this wave with this lane's digit
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (uint32_t b = 0; b < 8u; ++b) {
            const bool bit = ((d >> b) & 1u) != 0u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) cnt[w][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = running[d] + rank;
            for (uint32_t k = 0; k < w; ++k) pos += cnt[k][d];
            if (pos < P.n) {  // always, the table being these keys' counts
                P.keysOut[pos] = key;
                P.valsOut[pos] = val;
                if (P.slotOut) P.slotOut[val] = pos;
            }
        }
        __syncthreads();
        if (t < kDigits) {
            uint32_t sum = 0u;
#pragma unroll
            for (uint32_t k = 0; k < kWaves; ++k) {
                sum += cnt[k][t];
                cnt[k][t] = 0u;
            }
            running[t] += sum;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_mesh_offsets(const uint32_t* sortedKeys, uint32_t n, uint32_t nverts,
                                                      uint32_t* adjOffsets) {
    const uint32_t v = blockIdx.x * 256 + threadIdx.x;
    if (v > nverts) return;
    uint32_t lo = 0u, hi = n;  // the first slot in [0, n] whose key is >= v
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (sortedKeys[mid] < v) lo = mid + 1u;
        else hi = mid;
    }
    adjOffsets[v] = lo;
}

extern "C" hipError_t rtk_launch_mesh_set(const MeshSetParams* p, hipStream_t stream, hipEvent_t afterIngest) {
    const uint32_t n = 3u * p->triCountPadded;
    if (n == 0u || p->nverts == 0u || p->triCount > p->triCountPadded) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mesh_ingest, dim3((n + 255u) / 256u), dim3(256), 0, stream, *p);
    hipLaunchKernelGGL(k_mesh_report, dim3(1), dim3(1), 0, stream, p->badCount, p->status);
    if (afterIngest) {
        const hipError_t e = hipEventRecord(afterIngest, stream);
        if (e != hipSuccess) return e;
    }
    uint32_t bits = 0u;
    while (bits < 32u && ((uint64_t)1 << bits) < (uint64_t)p->nverts) ++bits;  // of the ids 0 .. nverts - 1
    const uint32_t passes = bits <= 8u ? 1u : (bits + 7u) / 8u;
    SortPass s;
    s.table = p->table;
    s.totals = p->table + kDigits * kMeshTilesMax;
    s.n = n;
    s.tileLen = mesh_tile_len(n);
    s.tiles = (n + s.tileLen - 1u) / s.tileLen;
    for (uint32_t k = 0; k < passes; ++k) {
        const bool last = k + 1u == passes;
        s.keysIn = k == 0u ? p->indices : p->keys[(k - 1u) & 1u];
        s.valsIn = k == 0u ? nullptr : p->vals[(k - 1u) & 1u];
        s.keysOut = p->keys[k & 1u];
        s.valsOut = last ? p->adjCorner : p->vals[k & 1u];
        s.slotOut = last ? p->cornerSlot : nullptr;
        s.shift = 8u * k;
        hipLaunchKernelGGL(k_mesh_hist, dim3(s.tiles), dim3(kThr), 0, stream, s);
        hipLaunchKernelGGL(k_mesh_scan, dim3(kDigits), dim3(256), 0, stream, s.table, s.tiles, s.totals);
        hipLaunchKernelGGL(k_mesh_scatter, dim3(s.tiles), dim3(kThr), 0, stream, s);
    }
    hipLaunchKernelGGL(k_mesh_offsets, dim3(p->nverts / 256u + 1u), dim3(256), 0, stream,
                       p->keys[(passes - 1u) & 1u], n, p->nverts, p->adjOffsets);
    return hipGetLastError();
}
