// TEST HARNESS ONLY: the host build of the tracer and the texel adjoint (trace_tex_host.cpp) plus the roughness adjoint and its
// transpose, epsm_trace_paths_bsdf_backward / epsm_trace_paths_bsdf_forward (include/epsm_trace.h) on host pointers: the same
// per-path code (epsm_trace_bsdf.h) and the same reduction -- one float row per 128 paths, the rows added in float64 in a fixed
// order.  Built into its own library by tests/_bsdf_host.py.  Not shipped, not a fallback.
#include "trace_tex_host.cpp"
#include "../../epsm_mitsuba3_amd/csrc/epsm_trace_bsdf.h"

namespace {
struct HostSlotSink {
    ba::SlotSums sums;
    void item(const ba::Item &it) { sums.item(it); }
    void finish() {}
};
}  // namespace

extern "C" size_t epsm_trace_bsdf_workspace_bytes(int64_t N) { return ba::workspace_bytes(N); }

extern "C" int epsm_trace_paths_bsdf_backward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                              int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                              const float *adj_radiance, float *grad_alpha, int B, void *workspace,
                                              size_t workspace_bytes, void *) {
    ba::BsdfArgs T;
    if (ba::bsdf_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, B)) return -22;
    if (N == 0) return 0;
    if (!adj_radiance || (B > 0 && !grad_alpha)) return -22;
    if (B == 0) return 0;
    if (!workspace || workspace_bytes < ba::workspace_bytes(N)) return -22;
    T.adj = adj_radiance; T.partial = (float *) workspace;
    const int64_t rows = ba::partial_rows(N);
#pragma omp parallel for schedule(dynamic, 2)
    for (int64_t r = 0; r < rows; ++r) {
        float row[ba::kMaxSlots] = {};
        for_each_path(T.A, r * ba::kBlock, (r + 1) * ba::kBlock < N ? (r + 1) * ba::kBlock : N,
                      [&](int64_t i, PathState &s, const TriHit &th0, const BvhStack &st) {
            HostSlotSink sink;
            sink.sums.adj = ld3(adj_radiance + 3 * i);
            sink.sums.clear();
            ba::bsdf_replay(T, i, true, s, th0, st, sink);
            for (int k = 0; k < B; ++k) row[k] += sink.sums.acc[k];
        });
        for (int k = 0; k < ba::kMaxSlots; ++k) T.partial[r * ba::kMaxSlots + k] = row[k];
    }
    for (int k = 0; k < B; ++k) {
        double acc = 0.0;
        for (int64_t r = 0; r < rows; ++r) acc += (double) T.partial[r * ba::kMaxSlots + k];
        grad_alpha[k] += (float) acc;
    }
    return 0;
}

extern "C" int epsm_trace_paths_bsdf_forward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                             int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                             const float *tangent_alpha, int B, float *d_radiance, void *) {
    ba::BsdfArgs T;
    if (ba::bsdf_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, B)) return -22;
    if (N == 0) return 0;
    if (!d_radiance || (B > 0 && !tangent_alpha)) return -22;
    T.tangent = tangent_alpha; T.d_radiance = d_radiance;
    for_each_path(T.A, [&](int64_t i, PathState &s, const TriHit &th0, const BvhStack &st) {
        ba::TangentSink sink{T, i, true, zero3<float>()};
        ba::bsdf_replay(T, i, true, s, th0, st, sink);
    });
    return 0;
}
