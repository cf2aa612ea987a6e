// epsm_trace_texture.hip -- kernels + C ABI of the texel adjoint and its transpose (include/epsm_trace.h,
// epsm_trace_paths_texture_backward / epsm_trace_paths_texture_forward; per-path code: epsm_trace_texture.h; the device frame:
// epsm_trace_adjoint.h).
#include "epsm_trace_adjoint.h"
#include "epsm_trace_texture.h"

using namespace epsm;
using epsm_host::fail;

namespace {

// Backward: twelve values per item, the footprint's four texels x rgb (FootprintScatter).
struct TexturePass {
    using Args = tx::TexArgs;
    using Backward = FootprintScatter<3, TexturePass>;
    using Forward = tx::GatherSink;
    template <class Sink> __device__ __forceinline__ static void replay(const Args &T, int64_t i, bool has, PathState &s,
                                                                        const TriHit &th0, const BvhStack &st, Sink &sink) {
        tx::texture_replay(T, i, has, s, th0, st, sink);
    }
    __device__ __forceinline__ static void value(F3 adj, F3 coef, float (&g)[3]) {
        const F3 v = mul3(adj, coef);
        g[0] = v.x; g[1] = v.y; g[2] = v.z;
    }
};

// Two waves per SIMD: at four (128 registers) the two items and the observer's state spill 376 B per lane to scratch, at two
// 220-228 registers and 36 B.
template <bool BACKWARD>
__global__ __launch_bounds__(128, 2) void epsm_texture_kernel(tx::TexArgs T) {
    __shared__ uint32_t s_stack[kLaneStackLds * 128];
    TexturePass::Backward sink{T};
    replay_lane<TexturePass, BACKWARD>(T, s_stack, sink);
}

}  // namespace

extern "C" int epsm_trace_paths_texture_backward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                 int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                 const float *adj_radiance, float *const *grad_tex, float *grad_env, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_trace_paths_texture_backward";
    tx::TexArgs T;
    if (const char *why = tx::tex_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, grad_tex, grad_env))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    if (!adj_radiance) return fail(EPSM_EINVAL, what, "NULL adj_radiance");
    if (T.n_buf == 0 && !grad_env) return EPSM_OK;
    T.adj = adj_radiance;
    return launch_checked(what, epsm_texture_kernel<true>, (N + 127) / 128, 128, stream, T);
}

extern "C" int epsm_trace_paths_texture_forward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                const float *const *tan_tex, const float *tan_env, float *d_radiance, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_trace_paths_texture_forward";
    tx::TexArgs T;
    // (the tangents are only read: they share the argument block's buffer slots with the backward pass's gradients)
    if (const char *why = tx::tex_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance,
                                            (float *const *) tan_tex, (float *) tan_env))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    if (!d_radiance) return fail(EPSM_EINVAL, what, "NULL d_radiance");
    T.d_radiance = d_radiance;
    return launch_checked(what, epsm_texture_kernel<false>, (N + 127) / 128, 128, stream, T);
}
