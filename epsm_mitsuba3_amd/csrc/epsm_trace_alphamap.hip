// epsm_trace_alphamap.hip -- kernels + C ABI of the roughness-map adjoint and its transpose (include/epsm_trace.h,
// epsm_trace_paths_alpha_texture_backward / epsm_trace_paths_alpha_texture_forward; per-path code: epsm_trace_alphamap.h; the
// device frame: epsm_trace_adjoint.h).
#include "epsm_trace_adjoint.h"
#include "epsm_trace_alphamap.h"

using namespace epsm;
using epsm_host::fail;

namespace {

// Backward: four values per item, one float per texel of the footprint -- a roughness has one channel (FootprintScatter).
struct AlphaMapPass {
    using Args = am::AlphaMapArgs;
    using Backward = FootprintScatter<1, AlphaMapPass>;
    using Forward = am::GatherSink;
    template <class Sink> __device__ __forceinline__ static void replay(const Args &T, int64_t i, bool has, PathState &s,
                                                                        const TriHit &th0, const BvhStack &st, Sink &sink) {
        am::alphamap_replay(T, i, has, s, th0, st, sink);
    }
    __device__ __forceinline__ static void value(F3 adj, F3 coef, float (&g)[1]) { g[0] = dot(adj, coef); }
};

// Two waves per SIMD (resource figures: DESIGN 5m).
template <bool BACKWARD>
__global__ __launch_bounds__(128, 2) void epsm_alphamap_kernel(am::AlphaMapArgs T) {
    __shared__ uint32_t s_stack[kLaneStackLds * 128];
    AlphaMapPass::Backward sink{T};
    replay_lane<AlphaMapPass, BACKWARD>(T, s_stack, sink);
}

}  // namespace

extern "C" int epsm_trace_paths_alpha_texture_backward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp,
                                                       int max_depth, int rr_depth, int64_t path_offset, int64_t N,
                                                       const float *radiance, const float *adj_radiance, float *const *grad_tex,
                                                       void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_trace_paths_alpha_texture_backward";
    am::AlphaMapArgs T;
    if (const char *why = am::alphamap_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, grad_tex))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    if (!adj_radiance) return fail(EPSM_EINVAL, what, "NULL adj_radiance");
    if (T.n_buf == 0) return EPSM_OK;
    T.adj = adj_radiance;
    return launch_checked(what, epsm_alphamap_kernel<true>, (N + 127) / 128, 128, stream, T);
}

extern "C" int epsm_trace_paths_alpha_texture_forward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp,
                                                      int max_depth, int rr_depth, int64_t path_offset, int64_t N,
                                                      const float *radiance, const float *const *tan_tex, float *d_radiance,
                                                      void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_trace_paths_alpha_texture_forward";
    am::AlphaMapArgs T;
    // (the tangents are only read: they share the argument block's buffer slots with the backward pass's gradients)
    if (const char *why = am::alphamap_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance,
                                                 (float *const *) tan_tex))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    if (!d_radiance) return fail(EPSM_EINVAL, what, "NULL d_radiance");
    T.d_radiance = d_radiance;
    return launch_checked(what, epsm_alphamap_kernel<false>, (N + 127) / 128, 128, stream, T);
}
