// sdf_host_check.cpp — a stand-alone run of the signed distance host rule (rt_pseudo_normals,
// rt_signed_distance_rule, csrc/sdf.cpp) for a memory and undefined-behaviour check on the CPU, without
// Python and without a device.  It compiles the three sources it calls as the library does (adjacency.cpp is
// rt_mesh_adjacency, which rt_pseudo_normals calls), so nothing else of the library is needed:
//
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined \
//         -fno-sanitize-recover=undefined -Iinclude -Ireal-time-ray-tracing_amd/csrc -I/opt/rocm/include \
//         tools/sdf_host_check.cpp real-time-ray-tracing_amd/csrc/sdf.cpp real-time-ray-tracing_amd/csrc/closest.cpp \
//         real-time-ray-tracing_amd/csrc/adjacency.cpp \
//         -o sdf_host_check && ./sdf_host_check
//
// Scenes: the fin (one edge of three triangles) and the open fan with a zero-area and a NaN triangle of
// tests/sdf_scenes.py, every array allocated at its exact size so that a read or write past it shows.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rtx_amd.h"

static int fails = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)

static void run(const char* name, const std::vector<float>& xyz, const std::vector<uint32_t>& idx) {
    const uint32_t nv = (uint32_t)(xyz.size() / 3), nt = (uint32_t)(idx.size() / 3);
    std::vector<float> table((size_t)nt * 24, -1.0f);
    CHECK(rt_pseudo_normals(xyz.data(), nv, idx.data(), nt, table.data()) == RT_OK);
    std::vector<float> tris((size_t)nt * 9);
    for (size_t c = 0; c < (size_t)nt * 3; ++c) memcpy(&tris[3 * c], &xyz[3 * (size_t)idx[c]], 12);
    const int side = 9;
    std::vector<float> pts;
    for (int i = 0; i < side * side * side; ++i) {
        pts.push_back(-1.6f + 0.4f * (float)(i % side));
        pts.push_back(-1.6f + 0.4f * (float)((i / side) % side));
        pts.push_back(-1.6f + 0.4f * (float)(i / (side * side)));
    }
    const uint32_t n = (uint32_t)(pts.size() / 3);
    std::vector<float> rec((size_t)n * 8), out((size_t)n * 4);
    for (float md : {INFINITY, 0.5f}) {
        CHECK(rt_closest_points_host(tris.data(), nullptr, nt, pts.data(), n, md, rec.data()) == RT_OK);
        uint32_t inside = 0, miss = 0;
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t w[8];
            memcpy(w, &rec[8 * (size_t)i], 32);
            const uint32_t t = w[4] < nt ? w[4] : 0u;
            CHECK(rt_signed_distance_rule(&pts[3 * (size_t)i], &rec[8 * (size_t)i], &tris[9 * (size_t)t],
                                          &table[24 * (size_t)t], &out[4 * (size_t)i]) == RT_OK);
            inside += out[4 * (size_t)i + 3] < 0.0f;
            miss += isinf(out[4 * (size_t)i + 3]) != 0;
        }
        printf("%s: %u triangles, %u points within %g: %u behind their feature, %u misses\n", name, nt, n, md, inside, miss);
    }
    CHECK(rt_pseudo_normals(nullptr, nv, idx.data(), nt, table.data()) == RT_ERR_ARG);
    CHECK(rt_pseudo_normals(xyz.data(), nv, idx.data(), 0, table.data()) == RT_ERR_ARG);
    std::vector<uint32_t> bad(idx);
    bad.back() = nv;
    CHECK(rt_pseudo_normals(xyz.data(), nv, bad.data(), nt, table.data()) == RT_ERR_ARG);
}

int main() {
    run("fin", {0, 0, 0, 0, 0, 1, 1, 0, 0.5f, -0.5f, 0.8f, 0.5f, -0.5f, -0.8f, 0.5f}, {0, 1, 2, 0, 1, 3, 1, 0, 4});
    std::vector<float> v = {0, 0.5f, 0};
    std::vector<uint32_t> idx;
    for (int k = 0; k <= 9; ++k) {
        const float a = (float)k * (6.2831853f / 9.0f);
        v.push_back(cosf(a)); v.push_back(0.3f * sinf(5.0f * a)); v.push_back(sinf(a));
    }
    for (uint32_t k = 0; k < 9; ++k) { idx.push_back(0); idx.push_back(k + 1); idx.push_back(k + 2); }
    memcpy(&v[3 * 5], &v[3 * 4], 12);          // triangle 3: zero area
    v[3 * 10] = v[3 * 10 + 1] = v[3 * 10 + 2] = NAN;  // triangle 8: a NaN vertex
    run("bad_fan", v, idx);
    printf(fails ? "%d check(s) failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
