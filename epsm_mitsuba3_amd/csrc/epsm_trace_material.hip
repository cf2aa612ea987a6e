// epsm_trace_material.hip -- kernels + C ABI of the conductor material adjoint and its transpose (include/epsm_trace.h,
// epsm_trace_paths_material_backward / epsm_trace_paths_material_forward; per-path code: epsm_trace_material.h; the device
// frame: epsm_trace_adjoint.h).
#include "epsm_trace_adjoint.h"
#include "epsm_trace_material.h"

using namespace epsm;
using epsm_host::fail;

namespace {

// Backward: 9 numbers per slot to reduce, so no atomics -- one row of ma::kRow partial sums per workgroup (block_row_reduce),
// epsm_rows_sum_kernel adds the rows up: grad_material[9 slot + 3 parameter + channel].
struct MaterialPass {
    using Args = ma::MaterialArgs;
    using Backward = SumSink<ma::MaterialSums>;
    using Forward = ma::MaterialTangentSink;
    template <class Sink> __device__ __forceinline__ static void replay(const Args &T, int64_t i, bool has, PathState &s,
                                                                        const TriHit &th0, const BvhStack &st, Sink &sink) {
        ma::material_replay(T, i, has, s, th0, st, sink);
    }
};

template <bool BACKWARD>
__global__ __launch_bounds__(128, 2) void epsm_material_kernel(ma::MaterialArgs T) {
    __shared__ uint32_t s_stack[kLaneStackLds * 128];
    __shared__ float s_part[2][ma::kRow];
    MaterialPass::Backward sink;
    replay_lane<MaterialPass, BACKWARD>(T, s_stack, sink);
    if (BACKWARD) block_row_reduce(sink.sums.acc, ma::kPerSlot * T.n_slots, s_part, T.partial + (int64_t) blockIdx.x * ma::kRow);
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
    if (!workspace_ok(workspace, workspace_bytes, ma::workspace_bytes(N)))
        return fail(EPSM_EINVAL, what, "workspace NULL, misaligned or smaller than epsm_trace_material_workspace_bytes(N)");
    T.adj = adj_radiance; T.partial = (float *) workspace;
    return launch_reduced<ma::kRow>(what, epsm_material_kernel<true>, T, ma::partial_rows(N), ma::kPerSlot * M, grad_material, stream);
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
    return launch_checked(what, epsm_material_kernel<false>, ma::partial_rows(N), 128, stream, T);
}
