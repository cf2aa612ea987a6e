// epsm_trace_alphamap.hip -- kernels + C ABI of the roughness-map adjoint and its transpose (include/epsm_trace.h,
// epsm_trace_paths_alpha_texture_backward / epsm_trace_paths_alpha_texture_forward; per-path code: epsm_trace_alphamap.h).
#include <stdio.h>
#include <string.h>

#include "epsm_common.h"
#include "epsm_trace_alphamap.h"
#include "epsm_trace_packet.h"
#include "epsm_wave_scatter.h"           // make_runs / seg_sum: the merge before the atomics

using namespace epsm;
using epsm_host::fail;

namespace {

// Backward: the item of a bounce goes to the texels of its footprint, one float each.  Lanes of a primary-ray wave are samples
// of one pixel: on a rough plate seen directly most of them share a footprint.  Adjacent lanes with the same
// (buffer, i0, j0) are summed first -- four segmented shuffle scans, one per texel: the texel adjoint's twelve carry three
// channels, a roughness has one -- and the run's last lane issues the adds; a wave whose footprints are all distinct skips the
// scans (the test is one ballot).
struct ScatterSink {
    const am::AlphaMapArgs &T;
    F3 adj;
    __device__ __forceinline__ void item(const tx::Item &it) {
        const unsigned long long on = __ballot(it.on);
        if (on == 0ull) return;                                           // (wave-uniform)
        const float g = dot(adj, it.coef);
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = g * it.w[k];
        bool issue = it.on;
        const Runs r = make_runs(it.on, it.b, it.i0, it.j0);
        if (__ballot(r.tail) != on) {                                     // some footprint is shared: merge (wave-uniform branch)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = seg_sum(v[k], r.head);
            issue = r.tail;
        }
        if (!issue) return;
        float *p = T.buf[it.b];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (adds_something(v[k])) atomicAdd(p + it.off[k], v[k]);      // (nearest: w[1..3] = 0, one add)
    }
    __device__ __forceinline__ void item(const am::NoItem &) {}
    __device__ __forceinline__ void finish() {}
};

// One lane = one path, as epsm_texture_kernel replays it (the primary rays walked by the wave, the same LDS stacks); lanes past N
// ride along without a path so that the whole wave reaches the merge.  Two waves per SIMD (resource figures: DESIGN 5m).
template <bool BACKWARD>
__global__ __launch_bounds__(128, 2) void epsm_alphamap_kernel(am::AlphaMapArgs T) {
    __shared__ uint32_t s_stack[kLaneStackLds * 128];
    uint32_t deep[kBvhStack - kLaneStackLds];
    const int64_t i = (int64_t) blockIdx.x * 128 + threadIdx.x;
    const BvhStack st = lane_stack(s_stack, deep, 128);
    const bool has = i < T.A.N;
    if (__ballot(has) == 0ull) return;
    PrimaryHit p = primary_hit(T.A, i, has, false, s_stack);
    if (BACKWARD) {
        ScatterSink sink{T, p.has ? ld3(T.adj + 3 * i) : zero3<float>()};
        am::alphamap_replay(T, p.i, p.has, p.s, p.th0, st, sink);
    } else {
        am::GatherSink sink{T, p.i, p.has, zero3<float>()};
        am::alphamap_replay(T, p.i, p.has, p.s, p.th0, st, sink);
    }
}

int launch(const char *what, const am::AlphaMapArgs &T, bool backward, void *stream) {
    const unsigned blocks = (unsigned) ((T.A.N + 127) / 128);
    if (backward) hipLaunchKernelGGL(epsm_alphamap_kernel<true>, dim3(blocks), dim3(128), 0, (hipStream_t) stream, T);
    else hipLaunchKernelGGL(epsm_alphamap_kernel<false>, dim3(blocks), dim3(128), 0, (hipStream_t) stream, T);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return epsm_host::hip_fail(what, e);
    return EPSM_OK;
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
    return launch(what, T, true, stream);
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
    return launch(what, T, false, stream);
}
