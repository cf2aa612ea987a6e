// TEST HARNESS ONLY: the host build of the tracer (trace_host.cpp, trace_fwd_host.cpp) plus the texel adjoint and its transpose,
// epsm_trace_paths_texture_backward / epsm_trace_paths_texture_forward (include/epsm_trace.h) on host pointers: the same
// per-path code (epsm_trace_texture.h), plain atomic adds and no merge.  Built into its own library by tests/_texture_host.py.
// Not shipped, not a fallback.
#include "trace_fwd_host.cpp"           // (trace_host.cpp and the reparameterised forward pass: texels next to geometry)
#include "../../epsm_mitsuba3_amd/csrc/epsm_trace_texture.h"

namespace {
struct HostScatterSink {
    const tx::TexArgs &T;
    F3 adj;
    void item(const tx::Item &it) {
        if (!it.on) return;
        const F3 g = mul3(adj, it.coef);
        float *p = T.buf[it.b];
        for (int k = 0; k < 4; ++k) {
            const float v[3] = {g.x * it.w[k], g.y * it.w[k], g.z * it.w[k]};
            for (int c = 0; c < 3; ++c) {
                if (v[c] == 0.f || !(fabsf(v[c]) < INFINITY)) continue;
                float *t = p + 3 * (int64_t) it.off[k] + c;
#pragma omp atomic
                *t += v[c];
            }
        }
    }
    void finish() {}
};
}  // namespace

extern "C" int epsm_trace_paths_texture_backward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                 int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                 const float *adj_radiance, float *const *grad_tex, float *grad_env, void *) {
    tx::TexArgs T;
    if (tx::tex_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, grad_tex, grad_env)) return -22;
    if (N == 0) return 0;
    if (!adj_radiance) return -22;
    T.adj = adj_radiance;
    for_each_path(T.A, [&](int64_t i, PathState &s, const TriHit &th0, const BvhStack &st) {
        HostScatterSink sink{T, ld3(adj_radiance + 3 * i)};
        tx::texture_replay(T, i, true, s, th0, st, sink);
    });
    return 0;
}

extern "C" int epsm_trace_paths_texture_forward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                const float *const *tan_tex, const float *tan_env, float *d_radiance, void *) {
    tx::TexArgs T;
    if (tx::tex_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, (float *const *) tan_tex,
                          (float *) tan_env))
        return -22;
    if (N == 0) return 0;
    if (!d_radiance) return -22;
    T.d_radiance = d_radiance;
    for_each_path(T.A, [&](int64_t i, PathState &s, const TriHit &th0, const BvhStack &st) {
        tx::GatherSink sink{T, i, true, zero3<float>()};
        tx::texture_replay(T, i, true, s, th0, st, sink);
    });
    return 0;
}
