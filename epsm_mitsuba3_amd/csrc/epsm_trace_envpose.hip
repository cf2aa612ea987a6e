// epsm_trace_envpose.hip -- kernels + C ABI of the envmap pose adjoint and its transpose (include/epsm_trace.h,
// epsm_trace_paths_envpose_backward / epsm_trace_paths_envpose_forward; per-path code: epsm_trace_envpose.h; the device
// frame: epsm_trace_adjoint.h).
#include "epsm_trace_adjoint.h"
#include "epsm_trace_envpose.h"

using namespace epsm;
using epsm_host::fail;

namespace {

// Backward: 4 numbers to reduce, so no atomics -- one row of ep::kRow partial sums per workgroup (block_row_reduce),
// epsm_rows_sum_kernel adds the rows up: grad_pose[omega.x, omega.y, omega.z, ln(scale)].
struct EnvPosePass {
    using Args = ep::EnvPoseArgs;
    using Backward = SumSink<ep::EnvPoseSums>;
    using Forward = ep::EnvPoseTangentSink;
    template <class Sink> __device__ __forceinline__ static void replay(const Args &T, int64_t i, bool has, PathState &s,
                                                                        const TriHit &th0, const BvhStack &st, Sink &sink) {
        ep::envpose_replay(T, i, has, s, th0, st, sink);
    }
};

template <bool BACKWARD>
__global__ __launch_bounds__(128, 2) void epsm_envpose_kernel(ep::EnvPoseArgs T) {
    __shared__ uint32_t s_stack[kLaneStackLds * 128];
    __shared__ float s_part[2][ep::kRow];
    EnvPosePass::Backward sink;
    replay_lane<EnvPosePass, BACKWARD>(T, s_stack, sink);
    if (BACKWARD) block_row_reduce(sink.sums.acc, ep::kRow, s_part, T.partial + (int64_t) blockIdx.x * ep::kRow);
}

}  // namespace

extern "C" size_t epsm_trace_envpose_workspace_bytes(int64_t N) { return ep::workspace_bytes(N); }

extern "C" int epsm_trace_paths_envpose_backward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                 int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                 const float *adj_radiance, float *grad_pose, void *workspace, size_t workspace_bytes,
                                                 void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_trace_paths_envpose_backward";
    ep::EnvPoseArgs T;
    if (const char *why = ep::envpose_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    if (!adj_radiance) return fail(EPSM_EINVAL, what, "NULL adj_radiance");
    if (!grad_pose) return fail(EPSM_EINVAL, what, "NULL grad_pose");
    if (!workspace_ok(workspace, workspace_bytes, ep::workspace_bytes(N)))
        return fail(EPSM_EINVAL, what, "workspace NULL, misaligned or smaller than epsm_trace_envpose_workspace_bytes(N)");
    T.adj = adj_radiance; T.partial = (float *) workspace;
    return launch_reduced<ep::kRow>(what, epsm_envpose_kernel<true>, T, ep::partial_rows(N), ep::kRow, grad_pose, stream);
}

extern "C" int epsm_trace_paths_envpose_forward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                const float *tangent_pose, float *d_radiance, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_trace_paths_envpose_forward";
    ep::EnvPoseArgs T;
    if (const char *why = ep::envpose_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    if (!tangent_pose) return fail(EPSM_EINVAL, what, "NULL tangent_pose");
    if (!d_radiance) return fail(EPSM_EINVAL, what, "NULL d_radiance");
    T.tangent = tangent_pose; T.d_radiance = d_radiance;
    return launch_checked(what, epsm_envpose_kernel<false>, ep::partial_rows(N), 128, stream, T);
}
