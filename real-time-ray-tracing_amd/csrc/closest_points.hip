// closest_points.hip — closest-point queries (rt_closest_points_device) for gfx950:
// for each caller point the triangle of the LBVH set that closest_kernels.h's rule puts nearest, by a
// best-first descent of the two-level tree.
//
// One lane per point in a dense grid.  A lane walks the record arena the ray tracers read (trav_load,
// SceneView): at a node it bounds the rule's d2 from below for both child boxes (closest_box_bound),
// descends into the child with the smaller bound (a tie goes left) and pushes the other one with its
// bound, each only while the bound does not exceed the best d2 so far; at a TLAS leaf it switches to
// the batch's BLAS root; at a BLAS leaf it offers the triangle, unless it is one of the build's
// padding triangles.  A pop skips entries whose bound has come to exceed the best.  Every comparison
// prunes on `bound > best` alone: an equal bound may hide an equal d2 under a lower index, and a NaN
// bound prunes nothing.  Since the bound never exceeds the rule's d2 of any triangle beneath the box,
// and the answer is the smallest (d2, index) over the candidates, the order of the walk does not show
// in the result: it is rt_closest_points_host's over the tree's leaves, bit for bit.
//
// The stack holds (traversal word, bound bits) pairs in LDS as [entry][thread] columns, as
// traverse.h's: 32 entries x 128 threads x 8 B = 32 KB, five workgroups to a CU.  Its depth follows the
// tree's, which equal Morton keys can make a chain of 1023 nodes.  So a push onto a full stack ends
// the walk, and the lane starts over on the build's leaf list (reorder) and offers every leaf: exact
// whatever the tree's shape, slow, and met only by such chains or under [debug] closestStack.
//
// No s_setprio: the query is a guest beside the frames, like the ray query.  No atomics, no inline
// assembly, no barrier (a lane of a partial last workgroup simply returns).
#include "closest_kernels.h"
#include "frame_kernels.h"
#include "traverse.h"

using namespace rtd;

namespace {

constexpr int kClosestBlock = 128;
static_assert(kClosestStackMax * kClosestBlock * 8 <= 32768, "the stack columns fit 32 KB of LDS");

RT_DEV void offer_triangle(ClosestBest& best, const float* p, float4 a, float4 b, float4 c, uint32_t tri) {
    const float v1[3] = {a.x, a.y, a.z}, v2[3] = {b.x, b.y, b.z}, v3[3] = {c.x, c.y, c.z};
    closest_offer(best, closest_point_triangle(p, v1, v2, v3), tri);
}

__global__ __launch_bounds__(kClosestBlock) void k_closest_points(ClosestParams P) {
    __shared__ uint2 stack[kClosestStackMax * kClosestBlock];
    const uint32_t i = blockIdx.x * (uint32_t)kClosestBlock + threadIdx.x;  // < 2^22 * 128 + 128
    if (i >= P.n) return;
    uint2* stk = stack + threadIdx.x;
    const float* pp = P.points + (size_t)i * P.stride;
    const float p[3] = {pp[0], pp[1], pp[2]};
    ClosestBest best;
    closest_begin(best, P.limit);
    if (closest_point_finite(p)) {
        const SceneView sc = scene_view(P.nodes, P.tlasNodes, P.triPos, nullptr);
        const int cap = (int)P.stackCap;
        // the first triangle of a last batch that has one leaf, or no triangle's index
        const uint32_t oneLeaf = P.triCount - (P.batchCount - 1u) * 1024u == 1u ? P.triCount - 1u : 0xFFFFFFFFu;
        int top = 0;  // entries on the stack
        bool full = false;
        uint32_t cur = sc.root;
        // a walk reads each record of the tree once at most; a count beyond that (no valid tree) ends it
        // as a full stack does
        uint32_t steps = 4096u * P.batchCount + 64u;
        for (;;) {
            if (steps-- == 0u) {
                full = true;
                break;
            }
            const TravRec rec = trav_load(sc, cur);
            bool pop = true;
            if (!(cur & kLeafBit)) {
                const float bl = closest_box_bound(p, rec.a.x, rec.a.y, rec.a.z, rec.a.w, rec.b.x, rec.b.y);
                const float br = closest_box_bound(p, rec.b.z, rec.b.w, rec.c.x, rec.c.y, rec.c.z, rec.c.w);
                const bool goLeft = !(br < bl);
                const uint32_t nearW = goLeft ? rec.d.x : rec.d.y, farW = goLeft ? rec.d.y : rec.d.x;
                const float nearB = goLeft ? bl : br, farB = goLeft ? br : bl;
                if (!(farB > best.d2)) {
                    if (top >= cap) {
                        full = true;
                        break;
                    }
                    stk[top * kClosestBlock] = make_uint2(farW, __float_as_uint(farB));
                    ++top;
                }
                if (!(nearB > best.d2)) {
                    cur = nearW;
                    pop = false;
                }
            } else if (!(cur & kBlasBit)) {  // a TLAS leaf: its word indexes the batch's BLAS root
                cur = (cur & kIdxMask) | kBlasBit;
                pop = false;
            } else {
                const uint32_t tri = (cur & kIdxMask) - sc.triBase;
                // A last batch of one leaf stores its element 0 as that leaf whatever sorted first
                // (bvh_build.hip refit, n == 1), while the leaf list names the element that did: when
                // that is a padding triangle, the list, which is the definition, holds nothing of the batch.
                bool listed = tri < P.triCount;
                if (listed && tri == oneLeaf) listed = P.reorder[oneLeaf] == 0u;
                if (listed) offer_triangle(best, p, rec.a, rec.b, rec.c, tri);
            }
            if (pop) {
                bool got = false;
                while (top > 0) {
                    --top;
                    const uint2 e = stk[top * kClosestBlock];
                    if (!(__uint_as_float(e.y) > best.d2)) {
                        cur = e.x;
                        got = true;
                        break;
                    }
                }
                if (!got) break;
            }
        }
        if (full) {  // the leaf list: batch b's leaves are b * 1024 + reorder[b * 1024 + k], k < its count
            closest_begin(best, P.limit);
            for (uint32_t b = 0; b < P.batchCount; ++b) {
                const uint32_t cnt = b + 1u < P.batchCount ? 1024u : P.triCount - (P.batchCount - 1u) * 1024u;
                for (uint32_t k = 0; k < cnt; ++k) {
                    const uint32_t tri = b * 1024u + P.reorder[b * 1024u + k];
                    if (tri >= P.triCount) continue;
                    const float4* tp = sc.tris + 4 * (size_t)tri;
                    offer_triangle(best, p, tp[0], tp[1], tp[2], tri);
                }
            }
        }
    }
    uint32_t w[8];
    closest_record(best, w);
    uint4* out = reinterpret_cast<uint4*>(P.out) + 2 * (size_t)i;
    out[0] = make_uint4(w[0], w[1], w[2], w[3]);
    out[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

}  // namespace

extern "C" hipError_t rtk_launch_closest_points(const ClosestParams* p, hipStream_t stream) {
    if (p->n == 0u || p->n > RT_QUERY_MAX_RAYS || p->stackCap < 2u || p->stackCap > (uint32_t)kClosestStackMax ||
        p->batchCount == 0u)
        return hipErrorInvalidValue;
    const dim3 grid((p->n + kClosestBlock - 1u) / kClosestBlock);
    hipLaunchKernelGGL(k_closest_points, grid, dim3(kClosestBlock), 0, stream, *p);
    return hipGetLastError();
}
