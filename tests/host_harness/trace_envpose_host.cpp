// TEST HARNESS ONLY: the host build of the tracer and the texel, roughness and material adjoints (trace_material_host.cpp) plus
// the envmap pose adjoint and its transpose, epsm_trace_paths_envpose_backward / epsm_trace_paths_envpose_forward
// (include/epsm_trace.h) on host pointers: the same per-path code (epsm_trace_envpose.h) and the same reduction -- one float row
// per 128 paths, the rows added in float64 in a fixed order -- and one test-only export, epsm_test_envpose_items: the items
// (coefficient, world direction) the same observer forms, path by path.  Built into its own library by tests/_envpose_host.py.
// Not shipped, not a fallback.
#include "trace_material_host.cpp"
#include "../../epsm_mitsuba3_amd/csrc/epsm_trace_envpose.h"

namespace {
struct HostEnvPoseSink {
    ep::EnvPoseSums sums;
    void item(const ep::Item &it) { sums.item(it); }
    void finish() {}
};
// the items of one path: rows of [coef (3), d (3)], at most `cap` of them kept, all of them counted
struct HostItemLog {
    float *rows;
    int cap, n;
    void item(const ep::Item &it) {
        if (!it.on) return;
        if (n < cap) {
            float *r = rows + 6 * n;
            r[0] = it.coef.x; r[1] = it.coef.y; r[2] = it.coef.z; r[3] = it.d.x; r[4] = it.d.y; r[5] = it.d.z;
        }
        ++n;
    }
    void finish() {}
};
}  // namespace

extern "C" size_t epsm_trace_envpose_workspace_bytes(int64_t N) { return ep::workspace_bytes(N); }

extern "C" int epsm_trace_paths_envpose_backward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                 int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                 const float *adj_radiance, float *grad_pose, void *workspace, size_t workspace_bytes,
                                                 void *) {
    ep::EnvPoseArgs T;
    if (ep::envpose_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance)) return -22;
    if (N == 0) return 0;
    if (!adj_radiance || !grad_pose) return -22;
    if (!workspace || (((uintptr_t) workspace) & 15) || workspace_bytes < ep::workspace_bytes(N)) return -22;
    T.adj = adj_radiance; T.partial = (float *) workspace;
    const int64_t rows = ep::partial_rows(N);
#pragma omp parallel for schedule(dynamic, 2)
    for (int64_t r = 0; r < rows; ++r) {
        float row[ep::kRow] = {};
        for_each_path(T.A, r * ep::kBlock, (r + 1) * ep::kBlock < N ? (r + 1) * ep::kBlock : N,
                      [&](int64_t i, PathState &s, const TriHit &th0, const BvhStack &st) {
            HostEnvPoseSink sink;
            sink.sums.adj = ld3(adj_radiance + 3 * i);
            sink.sums.clear();
            ep::envpose_replay(T, i, true, s, th0, st, sink);
            for (int k = 0; k < ep::kRow; ++k) row[k] += sink.sums.acc[k];
        });
        for (int k = 0; k < ep::kRow; ++k) T.partial[r * ep::kRow + k] = row[k];
    }
    for (int k = 0; k < ep::kRow; ++k) {
        double acc = 0.0;
        for (int64_t r = 0; r < rows; ++r) acc += (double) T.partial[r * ep::kRow + k];
        grad_pose[k] += (float) acc;
    }
    return 0;
}

extern "C" int epsm_trace_paths_envpose_forward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                const float *tangent_pose, float *d_radiance, void *) {
    ep::EnvPoseArgs T;
    if (ep::envpose_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance)) return -22;
    if (N == 0) return 0;
    if (!tangent_pose || !d_radiance) return -22;
    T.tangent = tangent_pose; T.d_radiance = d_radiance;
    for_each_path(T.A, [&](int64_t i, PathState &s, const TriHit &th0, const BvhStack &st) {
        ep::EnvPoseTangentSink sink{T, i, true, zero3<float>()};
        ep::envpose_replay(T, i, true, s, th0, st, sink);
    });
    return 0;
}

// TEST ONLY: items (N, cap, 6) = [coef (3), d (3)] of every path (rows past a path's count are left as they were), count (N).
extern "C" int epsm_test_envpose_items(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                       int rr_depth, int64_t path_offset, int64_t N, const float *radiance, int cap, float *items,
                                       int32_t *count) {
    ep::EnvPoseArgs T;
    if (ep::envpose_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance)) return -22;
    if (N == 0) return 0;
    if (cap < 1 || !items || !count) return -22;
    for_each_path(T.A, [&](int64_t i, PathState &s, const TriHit &th0, const BvhStack &st) {
        HostItemLog sink{items + 6 * (int64_t) cap * i, cap, 0};
        ep::envpose_replay(T, i, true, s, th0, st, sink);
        count[i] = sink.n;
    });
    return 0;
}
