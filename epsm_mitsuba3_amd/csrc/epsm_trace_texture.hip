// epsm_trace_texture.hip -- kernels + C ABI of the texel adjoint and its transpose (include/epsm_trace.h,
// epsm_trace_paths_texture_backward / epsm_trace_paths_texture_forward; per-path code: epsm_trace_texture.h).
#include <stdio.h>
#include <string.h>

#include "epsm_common.h"
#include "epsm_trace_texture.h"
#include "epsm_trace_packet.h"
#include "epsm_wave_scatter.h"           // make_runs / seg_sum: the merge before the atomics

using namespace epsm;
using epsm_host::fail;

namespace {

// Backward: the items of a bounce go to the texels.  Lanes of a primary-ray wave are samples of one pixel: at the
// first vertex, and where the environment is seen directly, most of them share a footprint.  Adjacent lanes with the same
// (buffer, i0, j0) are summed first -- twelve segmented shuffle scans, one per texel and channel -- and the run's last lane
// issues the adds; a wave whose footprints are all distinct skips the scans (the test is one ballot).
struct ScatterSink {
    const tx::TexArgs &T;
    F3 adj;
    __device__ __forceinline__ void item(const tx::Item &it) {
        const unsigned long long on = __ballot(it.on);
        if (on == 0ull) return;                                           // (wave-uniform)
        const F3 g = mul3(adj, it.coef);
        float v[12];
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[3 * k] = g.x * it.w[k]; v[3 * k + 1] = g.y * it.w[k]; v[3 * k + 2] = g.z * it.w[k]; }
        bool issue = it.on;
        const Runs r = make_runs(it.on, it.b, it.i0, it.j0);
        if (__ballot(r.tail) != on) {                                     // some footprint is shared: merge (wave-uniform branch)
#pragma unroll
            for (int q = 0; q < 12; ++q) v[q] = seg_sum(v[q], r.head);
            issue = r.tail;
        }
        if (!issue) return;
        float *p = T.buf[it.b];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float *t = p + 3 * (int64_t) it.off[k];
            if (adds_something(v[3 * k])) atomicAdd(t, v[3 * k]);
            if (adds_something(v[3 * k + 1])) atomicAdd(t + 1, v[3 * k + 1]);
            if (adds_something(v[3 * k + 2])) atomicAdd(t + 2, v[3 * k + 2]);
        }
    }
    __device__ __forceinline__ void finish() {}
};

// One lane = one path, as epsm_trace_kernel traces it (the primary rays walked by the wave, the same LDS stacks); lanes past N
// ride along without a path so that the whole wave reaches the merge.  Two waves per SIMD: at four (128 registers) the two items
// and the observer's state spill 376 B per lane to scratch, at two 220-228 registers and 36 B.
template <bool BACKWARD>
__global__ __launch_bounds__(128, 2) void epsm_texture_kernel(tx::TexArgs T) {
    __shared__ uint32_t s_stack[kLaneStackLds * 128];
    uint32_t deep[kBvhStack - kLaneStackLds];
    const int64_t i = (int64_t) blockIdx.x * 128 + threadIdx.x;
    const BvhStack st = lane_stack(s_stack, deep, 128);
    const bool has = i < T.A.N;
    if (__ballot(has) == 0ull) return;
    PrimaryHit p = primary_hit(T.A, i, has, false, s_stack);
    if (BACKWARD) {
        ScatterSink sink{T, p.has ? ld3(T.adj + 3 * i) : zero3<float>()};
        tx::texture_replay(T, p.i, p.has, p.s, p.th0, st, sink);
    } else {
        tx::GatherSink sink{T, p.i, p.has, zero3<float>()};
        tx::texture_replay(T, p.i, p.has, p.s, p.th0, st, sink);
    }
}

int launch(const char *what, const tx::TexArgs &T, bool backward, void *stream) {
    const unsigned blocks = (unsigned) ((T.A.N + 127) / 128);
    if (backward) hipLaunchKernelGGL(epsm_texture_kernel<true>, dim3(blocks), dim3(128), 0, (hipStream_t) stream, T);
    else hipLaunchKernelGGL(epsm_texture_kernel<false>, dim3(blocks), dim3(128), 0, (hipStream_t) stream, T);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return epsm_host::hip_fail(what, e);
    return EPSM_OK;
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
    return launch(what, T, true, stream);
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
    return launch(what, T, false, stream);
}
