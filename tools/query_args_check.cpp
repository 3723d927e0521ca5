// query_args_check.cpp — stand-alone host check of rt_trace_rays_device's argument and state checks
// (frame.cpp), for a sanitizer build of the host code; needs no GPU: the context is created, never
// inited, so every call returns before it touches the device.
//
// Build and run (host objects with ASan + UBSan, the kernels' objects as the product builds them):
//   make
//   F="-O1 -g -std=c++17 -fPIC -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer \
//      -D__HIP_PLATFORM_AMD__ -Iinclude -Ireal-time-ray-tracing_amd/csrc -I/opt/rocm/include"
//   for f in real-time-ray-tracing_amd/csrc/*.cpp tools/query_args_check.cpp; do
//       hipcc $F -x c++ -c $f -o /tmp/qa_$(basename $f).o; done
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/query_args_check /tmp/qa_*.o \
//       real-time-ray-tracing_amd/lib/obj/*.hip.o -ldl && /tmp/query_args_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rtx_amd.h"

static int failures = 0;
#define EXPECT(call, want)                                                                  \
    do {                                                                                    \
        const int rc__ = (call);                                                            \
        if (rc__ != (want)) { printf("FAIL %s: %d, expected %d\n", #call, rc__, (want)); ++failures; } \
    } while (0)

int main() {
    rt_context* ctx = nullptr;
    if (rt_create(64, 64, nullptr, &ctx) != RT_OK || !ctx) { printf("rt_create failed\n"); return 2; }
    std::vector<float> org(64 * 3), dir(64 * 3, 1.0f), raw(64 * 4 + 8);
    std::vector<uint32_t> iters(64);
    float* hits = raw.data();
    while ((uintptr_t)hits & 15u) ++hits;
    const rt_ray_query good = {org.data(), 3, dir.data(), 3, 64, hits, iters.data(), 0, nullptr, nullptr};
    rt_ray_query q;

    EXPECT(rt_trace_rays_device(nullptr, &good), RT_ERR_ARG);
    EXPECT(rt_trace_rays_device(ctx, nullptr), RT_ERR_ARG);
    EXPECT(rt_trace_rays_device(ctx, &good), RT_ERR_STATE);
    if (!strstr(rt_last_error(ctx), "before rt_init")) { printf("FAIL message: %s\n", rt_last_error(ctx)); ++failures; }
#define BAD(stmt) q = good; stmt; EXPECT(rt_trace_rays_device(ctx, &q), RT_ERR_ARG)
    BAD(q.org = nullptr);
    BAD(q.dir = nullptr);
    BAD(q.hits = nullptr);
    BAD(q.org_stride = 2);
    BAD(q.dir_stride = 0);
    BAD(q.n = RT_QUERY_MAX_RAYS + 1u);
    BAD(q.n = 0xFFFFFFFFu);
    BAD(q.flags = 2u);
    BAD(q.flags = 0x80000001u);
    BAD(q.hits = hits + 1);
    BAD(q.hits = hits + 2);
    BAD(q.org = (const float*)((const char*)org.data() + 2));
    BAD(q.dir = (const float*)((const char*)dir.data() + 1));
    BAD(q.iters = (uint32_t*)((char*)iters.data() + 2));
    q = good; q.n = 0; q.org = q.dir = nullptr; q.hits = nullptr; q.iters = nullptr;
    EXPECT(rt_trace_rays_device(ctx, &q), RT_ERR_STATE);
    q = good; q.n = RT_QUERY_MAX_RAYS; q.flags = RT_QUERY_ANY_HIT; q.iters = nullptr;
    EXPECT(rt_trace_rays_device(ctx, &q), RT_ERR_STATE);
    rt_destroy(ctx);
    printf(failures ? "%d check(s) failed\n" : "rt_trace_rays_device argument checks ok\n", failures);
    return failures ? 1 : 0;
}
