// epsm_trace_material.hip -- kernels + C ABI of the conductor material adjoint and its transpose (include/epsm_trace.h,
// epsm_trace_paths_material_backward / epsm_trace_paths_material_forward; per-path code: epsm_trace_material.h).
#include <stdio.h>
#include <string.h>

#include "epsm_common.h"
#include "epsm_trace_material.h"
#include "epsm_trace_packet.h"

using namespace epsm;
using epsm_host::fail;

namespace {

struct BackwardSink {
    ma::MaterialSums sums;
    __device__ __forceinline__ void item(const ma::Item &it) { sums.item(it); }
    __device__ __forceinline__ void finish() {}
};

// the sum of v over the 64 lanes of the wave, in every lane (a butterfly: the same order of additions in every launch)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One lane = one path, as epsm_bsdf_kernel replays it (the primary rays walked by the wave, the same LDS stacks); lanes past N
// ride along without a path so that both waves reach the reduction.  Backward: 9 numbers per slot to reduce, so no atomics -- a
// butterfly over each wave, the workgroup's two waves through LDS, one row of ma::kRow partial sums per workgroup;
// epsm_material_sum_kernel adds the rows up.
template <bool BACKWARD>
__global__ __launch_bounds__(128, 2) void epsm_material_kernel(ma::MaterialArgs T) {
    __shared__ uint32_t s_stack[kLaneStackLds * 128];
    __shared__ float s_part[2][ma::kRow];
    uint32_t deep[kBvhStack - kLaneStackLds];
    const int64_t i = (int64_t) blockIdx.x * 128 + threadIdx.x;
    const BvhStack st = lane_stack(s_stack, deep, 128);
    PrimaryHit p = primary_hit(T.A, i, false, s_stack);           // (no early exit: an idle wave still owes the reduction its zeros)
    if (BACKWARD) {
        BackwardSink sink;
        sink.sums.adj = p.has ? ld3(T.adj + 3 * i) : zero3<float>();
        sink.sums.clear();
        ma::material_replay(T, p.i, p.has, p.s, p.th0, st, sink);
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
        for (int k = 0; k < ma::kRow; ++k) {
            const float v = k < ma::kPerSlot * T.n_slots ? wave_sum(sink.sums.acc[k]) : 0.f;      // (wave-uniform condition)
            if (lane == 0) s_part[wave][k] = v;
        }
        __syncthreads();
        if (threadIdx.x < ma::kRow)
            T.partial[(int64_t) blockIdx.x * ma::kRow + threadIdx.x] = s_part[0][threadIdx.x] + s_part[1][threadIdx.x];
    } else {
        ma::MaterialTangentSink sink{T, p.i, p.has, zero3<float>()};
        ma::material_replay(T, p.i, p.has, p.s, p.th0, st, sink);
    }
}

// grad_material[j] += sum over the rows of partial[row][j], j = 9 slot + 3 parameter + channel, in float64 and in a fixed order:
// thread t sums rows t, t + 256, ..., then a tree over the 256 threads.  One workgroup per number.
__global__ __launch_bounds__(256) void epsm_material_sum_kernel(const float *partial, int64_t rows, float *grad_material) {
    __shared__ double s_sum[256];
    const int j = blockIdx.x;
    double acc = 0.0;
    for (int64_t r = threadIdx.x; r < rows; r += 256) acc += (double) partial[r * ma::kRow + j];
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int) threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) grad_material[j] += (float) s_sum[0];
}

}  // namespace

extern "C" size_t epsm_trace_material_workspace_bytes(int64_t N) { return ma::workspace_bytes(N); }

extern "C" int epsm_trace_paths_material_backward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                  int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                  const float *adj_radiance, float *grad_material, int M, void *workspace,
                                                  size_t workspace_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_trace_paths_material_backward";
    ma::MaterialArgs T;
    if (const char *why = ma::material_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, M))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    if (!adj_radiance) return fail(EPSM_EINVAL, what, "NULL adj_radiance");
    if (M > 0 && !grad_material) return fail(EPSM_EINVAL, what, "NULL grad_material");
    if (M == 0) return EPSM_OK;
    if (!workspace || workspace_bytes < ma::workspace_bytes(N) || ((uintptr_t) workspace & 15u))
        return fail(EPSM_EINVAL, what, "workspace NULL, misaligned or smaller than epsm_trace_material_workspace_bytes(N)");
    T.adj = adj_radiance; T.partial = (float *) workspace;
    const int64_t rows = ma::partial_rows(N);
    hipLaunchKernelGGL(epsm_material_kernel<true>, dim3((unsigned) rows), dim3(128), 0, (hipStream_t) stream, T);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return epsm_host::hip_fail(what, e);
    hipLaunchKernelGGL(epsm_material_sum_kernel, dim3((unsigned) (ma::kPerSlot * M)), dim3(256), 0, (hipStream_t) stream,
                       (const float *) T.partial, rows, grad_material);
    e = hipGetLastError();
    if (e != hipSuccess) return epsm_host::hip_fail(what, e);
    return EPSM_OK;
}

extern "C" int epsm_trace_paths_material_forward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                 int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                 const float *tangent_material, int M, float *d_radiance, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_trace_paths_material_forward";
    ma::MaterialArgs T;
    if (const char *why = ma::material_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, M))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    if (!d_radiance) return fail(EPSM_EINVAL, what, "NULL d_radiance");
    if (M > 0 && !tangent_material) return fail(EPSM_EINVAL, what, "NULL tangent_material");
    T.tangent = tangent_material; T.d_radiance = d_radiance;
    hipLaunchKernelGGL(epsm_material_kernel<false>, dim3((unsigned) ma::partial_rows(N)), dim3(128), 0, (hipStream_t) stream, T);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return epsm_host::hip_fail(what, e);
    return EPSM_OK;
}
