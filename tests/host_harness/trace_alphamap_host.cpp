// TEST HARNESS ONLY: the host build of the tracer, the texel, roughness and conductor material adjoints
// (trace_material_host.cpp) plus the roughness-map adjoint and its transpose, epsm_trace_paths_alpha_texture_backward /
// epsm_trace_paths_alpha_texture_forward (include/epsm_trace.h) on host pointers: the same per-path code
// (epsm_trace_alphamap.h), plain atomic adds and no merge.  Built into its own library by tests/_alphamap_host.py.  Not shipped,
// not a fallback.
#include "trace_material_host.cpp"
#include "../../epsm_mitsuba3_amd/csrc/epsm_trace_alphamap.h"

namespace {
struct HostAlphaMapScatterSink {
    const am::AlphaMapArgs &T;
    F3 adj;
    void item(const tx::Item &it) {
        if (!it.on) return;
        const float g = dot(adj, it.coef);
        float *p = T.buf[it.b];
        for (int k = 0; k < 4; ++k) {
            const float v = g * it.w[k];
            if (v == 0.f || !(fabsf(v) < INFINITY)) continue;
            float *t = p + it.off[k];
#pragma omp atomic
            *t += v;
        }
    }
    void item(const am::NoItem &) {}
    void finish() {}
};
}  // namespace

extern "C" int epsm_trace_paths_alpha_texture_backward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp,
                                                       int max_depth, int rr_depth, int64_t path_offset, int64_t N,
                                                       const float *radiance, const float *adj_radiance, float *const *grad_tex,
                                                       void *) {
    am::AlphaMapArgs T;
    if (am::alphamap_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, grad_tex)) return -22;
    if (N == 0) return 0;
    if (!adj_radiance) return -22;
    if (T.n_buf == 0) return 0;
    T.adj = adj_radiance;
    for_each_path(T.A, [&](int64_t i, PathState &s, const TriHit &th0, const BvhStack &st) {
        HostAlphaMapScatterSink sink{T, ld3(adj_radiance + 3 * i)};
        am::alphamap_replay(T, i, true, s, th0, st, sink);
    });
    return 0;
}

extern "C" int epsm_trace_paths_alpha_texture_forward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp,
                                                      int max_depth, int rr_depth, int64_t path_offset, int64_t N,
                                                      const float *radiance, const float *const *tan_tex, float *d_radiance, void *) {
    am::AlphaMapArgs T;
    if (am::alphamap_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, (float *const *) tan_tex))
        return -22;
    if (N == 0) return 0;
    if (!d_radiance) return -22;
    T.d_radiance = d_radiance;
    for_each_path(T.A, [&](int64_t i, PathState &s, const TriHit &th0, const BvhStack &st) {
        am::GatherSink sink{T, i, true, zero3<float>()};
        am::alphamap_replay(T, i, true, s, th0, st, sink);
    });
    return 0;
}
