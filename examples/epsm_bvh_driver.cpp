// epsm_bvh_driver.cpp -- a C++ host builds the scene's acceleration structure through the C ABI alone (no Python in the
// process): epsm_bvh_build on a deterministic triangle soup of mixed scales, a structural check of the tree on the host,
// then the vertices move, epsm_bvh_refit, and the boxes are checked again.  Prints OK and exits 0 when every check holds.
//   make -C examples && examples/build/epsm_bvh_driver [T]
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "epsm_trace.h"

#define HIP_OK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); }  \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static double uniform01() {                       // splitmix64: the same soup on every run
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (double) ((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0);
}
static double uniform(double a, double b) { return a + (b - a) * uniform01(); }

// a teapot in a stadium: clusters at several scales, triangle sizes over six decades
static void soup(int64_t T, std::vector<float> &pos, std::vector<uint32_t> &tri) {
    double cl[12][3];
    for (auto &c : cl) {
        const double s = pow(10.0, uniform(-2, 2));
        for (double &x : c) x = uniform(-1, 1) * s;
    }
    pos.resize(9 * T);
    tri.resize(3 * T);
    for (int64_t t = 0; t < T; ++t) {
        const double *c = cl[(int) (uniform01() * 12) % 12];
        const double spread = pow(10.0, uniform(-4, 1)), size = pow(10.0, uniform(-5, 1));
        double centre[3];
        for (int k = 0; k < 3; ++k) centre[k] = c[k] + uniform(-1, 1) * spread;
        for (int v = 0; v < 3; ++v) {
            for (int k = 0; k < 3; ++k) pos[9 * t + 3 * v + k] = (float) (centre[k] + uniform(-1, 1) * size);
            tri[3 * t + v] = (uint32_t) (3 * t + v);
        }
    }
}

static int g_fail = 0;
#define CHECK(cond, ...)                                           \
    do {                                                           \
        if (!(cond)) {                                             \
            if (g_fail++ < 10) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
        }                                                          \
    } while (0)

static bool inside(float lo, float hi, float plo, float phi) { return lo >= plo && hi <= phi; }

// every triangle in exactly one leaf, every box holds its triangles and its child's boxes, at most 16 wide levels
static void check_tree(const std::vector<EpsmBvhNode> &nodes, const std::vector<uint32_t> &prim, const std::vector<float> &pos,
                       const std::vector<uint32_t> &tri, int64_t T, const char *when) {
    std::vector<int> seen(T, 0);
    struct Item { int node, depth; float lo[3], hi[3]; };
    std::vector<Item> stack;
    const float inf = INFINITY;
    stack.push_back({0, 0, {-inf, -inf, -inf}, {inf, inf, inf}});
    int max_depth = 0;
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        if (it.depth > max_depth) max_depth = it.depth;
        CHECK(it.node >= 0 && it.node < (int) nodes.size(), "%s: node index %d out of range", when, it.node);
        if (it.node < 0 || it.node >= (int) nodes.size()) continue;
        const EpsmBvhNode &n = nodes[it.node];
        for (int s = 0; s < 4; ++s) {
            const int c = n.c[s];
            if (c == 0x7fffffff) continue;
            const float lo[3] = {n.lox[s], n.loy[s], n.loz[s]}, hi[3] = {n.hix[s], n.hiy[s], n.hiz[s]};
            for (int k = 0; k < 3; ++k)
                CHECK(inside(lo[k], hi[k], it.lo[k], it.hi[k]), "%s: node %d slot %d outside its parent's box", when, it.node, s);
            if (c < 0) {
                const int first = (~c) >> 3, count = (~c) & 7;
                CHECK(count >= 1 && count <= 6 && count == n.n[s], "%s: node %d slot %d bad leaf count", when, it.node, s);
                for (int q = first; q < first + count && q < T; ++q) {
                    ++seen[q];
                    const uint32_t t = prim[q];
                    for (int v = 0; v < 3; ++v)
                        for (int k = 0; k < 3; ++k) {
                            const float p = pos[3 * tri[3 * t + v] + k];
                            CHECK(p >= lo[k] && p <= hi[k], "%s: triangle %u outside its leaf box", when, t);
                        }
                }
            } else {
                stack.push_back({c, it.depth + 1, {lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}});
            }
        }
    }
    for (int64_t q = 0; q < T; ++q) CHECK(seen[q] == 1, "%s: leaf entry %lld referenced %d times", when, (long long) q, seen[q]);
    std::vector<int> hit(T, 0);
    for (int64_t q = 0; q < T; ++q) if (prim[q] < (uint32_t) T) ++hit[prim[q]];
    for (int64_t t = 0; t < T; ++t) CHECK(hit[t] == 1, "%s: triangle %lld in %d leaves", when, (long long) t, hit[t]);
    CHECK(max_depth + 1 <= 16, "%s: %d wide levels", when, max_depth + 1);
    printf("%s: %zu nodes, %d wide levels, %lld triangles in leaves\n", when, nodes.size(), max_depth + 1, (long long) T);
}

int main(int argc, char **argv) {
    const int64_t T = argc > 1 ? atoll(argv[1]) : 20000;
    const int64_t V = 3 * T;
    std::vector<float> pos;
    std::vector<uint32_t> tri;
    soup(T, pos, tri);

    float *d_pos, *d_tv;
    uint32_t *d_tri, *d_prim;
    EpsmBvhNode *d_nodes;
    void *d_ws;
    const int64_t cap = epsm_bvh_max_nodes(T);
    const size_t ws_bytes = epsm_bvh_workspace_bytes(T);
    HIP_OK(hipMalloc(&d_pos, sizeof(float) * 3 * V));
    HIP_OK(hipMalloc(&d_tri, sizeof(uint32_t) * 3 * T));
    HIP_OK(hipMalloc(&d_prim, sizeof(uint32_t) * T));
    HIP_OK(hipMalloc(&d_tv, sizeof(float) * 9 * T));
    HIP_OK(hipMalloc(&d_nodes, sizeof(EpsmBvhNode) * cap));
    HIP_OK(hipMalloc(&d_ws, ws_bytes));
    HIP_OK(hipMemcpy(d_pos, pos.data(), sizeof(float) * 3 * V, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_tri, tri.data(), sizeof(uint32_t) * 3 * T, hipMemcpyHostToDevice));

    int32_t n_nodes = 0, n_levels = 0, level_begin[17];
    int rc = epsm_bvh_build(d_pos, V, d_tri, T, d_nodes, d_prim, d_tv, &n_nodes, level_begin, &n_levels, d_ws, ws_bytes, nullptr);
    if (rc != EPSM_OK) { fprintf(stderr, "epsm_bvh_build: %d %s\n", rc, epsm_last_error()); return 1; }
    std::vector<EpsmBvhNode> nodes(n_nodes);
    std::vector<uint32_t> prim(T);
    HIP_OK(hipMemcpy(nodes.data(), d_nodes, sizeof(EpsmBvhNode) * n_nodes, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(prim.data(), d_prim, sizeof(uint32_t) * T, hipMemcpyDeviceToHost));
    CHECK(n_levels >= 1 && n_levels <= 16 && level_begin[0] == 0 && level_begin[n_levels] == n_nodes, "bad level table");
    check_tree(nodes, prim, pos, tri, T, "build");

    // move the vertices (a shear and a lift that grows with the index), refit, check the boxes again
    for (int64_t i = 0; i < V; ++i) {
        pos[3 * i + 0] += 0.25f * pos[3 * i + 2];
        pos[3 * i + 2] += 1e-5f * (float) (i % 1000);
    }
    HIP_OK(hipMemcpy(d_pos, pos.data(), sizeof(float) * 3 * V, hipMemcpyHostToDevice));
    rc = epsm_bvh_refit(d_pos, V, d_tri, d_prim, T, d_nodes, n_nodes, level_begin, n_levels, d_tv, nullptr);
    if (rc != EPSM_OK) { fprintf(stderr, "epsm_bvh_refit: %d %s\n", rc, epsm_last_error()); return 1; }
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(nodes.data(), d_nodes, sizeof(EpsmBvhNode) * n_nodes, hipMemcpyDeviceToHost));
    check_tree(nodes, prim, pos, tri, T, "refit");

    HIP_OK(hipFree(d_pos)); HIP_OK(hipFree(d_tri)); HIP_OK(hipFree(d_prim));
    HIP_OK(hipFree(d_tv)); HIP_OK(hipFree(d_nodes)); HIP_OK(hipFree(d_ws));
    if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    printf("OK\n");
    return 0;
}
