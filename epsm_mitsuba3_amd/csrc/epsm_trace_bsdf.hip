// epsm_trace_bsdf.hip -- kernels + C ABI of the roughness adjoint and its transpose (include/epsm_trace.h,
// epsm_trace_paths_bsdf_backward / epsm_trace_paths_bsdf_forward; per-path code: epsm_trace_bsdf.h; the device frame:
// epsm_trace_adjoint.h).
#include "epsm_trace_adjoint.h"
#include "epsm_trace_bsdf.h"

using namespace epsm;
using epsm_host::fail;

namespace {

// Backward: at most kMaxSlots numbers to reduce, so no atomics -- one row of kMaxSlots partial sums per workgroup
// (block_row_reduce), epsm_rows_sum_kernel adds the rows up.
struct BsdfPass {
    using Args = ba::BsdfArgs;
    using Backward = SumSink<ba::SlotSums>;
    using Forward = ba::TangentSink;
    template <class Sink> __device__ __forceinline__ static void replay(const Args &T, int64_t i, bool has, PathState &s,
                                                                        const TriHit &th0, const BvhStack &st, Sink &sink) {
        ba::bsdf_replay(T, i, has, s, th0, st, sink);
    }
};

template <bool BACKWARD>
__global__ __launch_bounds__(128, 2) void epsm_bsdf_kernel(ba::BsdfArgs T) {
    __shared__ uint32_t s_stack[kLaneStackLds * 128];
    __shared__ float s_part[2][ba::kMaxSlots];
    BsdfPass::Backward sink;
    replay_lane<BsdfPass, BACKWARD>(T, s_stack, sink);
    if (BACKWARD) block_row_reduce(sink.sums.acc, T.n_slots, s_part, T.partial + (int64_t) blockIdx.x * ba::kMaxSlots);
}

}  // namespace

extern "C" size_t epsm_trace_bsdf_workspace_bytes(int64_t N) { return ba::workspace_bytes(N); }

extern "C" int epsm_trace_paths_bsdf_backward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                              int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                              const float *adj_radiance, float *grad_alpha, int B, void *workspace,
                                              size_t workspace_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_trace_paths_bsdf_backward";
    ba::BsdfArgs T;
    if (const char *why = ba::bsdf_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, B))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    if (!adj_radiance) return fail(EPSM_EINVAL, what, "NULL adj_radiance");
    if (B > 0 && !grad_alpha) return fail(EPSM_EINVAL, what, "NULL grad_alpha");
    if (B == 0) return EPSM_OK;
    if (!workspace_ok(workspace, workspace_bytes, ba::workspace_bytes(N)))
        return fail(EPSM_EINVAL, what, "workspace NULL, misaligned or smaller than epsm_trace_bsdf_workspace_bytes(N)");
    T.adj = adj_radiance; T.partial = (float *) workspace;
    return launch_reduced<ba::kMaxSlots>(what, epsm_bsdf_kernel<true>, T, ba::partial_rows(N), B, grad_alpha, stream);
}

extern "C" int epsm_trace_paths_bsdf_forward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                             int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                             const float *tangent_alpha, int B, float *d_radiance, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_trace_paths_bsdf_forward";
    ba::BsdfArgs T;
    if (const char *why = ba::bsdf_args_fill(T, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, radiance, B))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    if (!d_radiance) return fail(EPSM_EINVAL, what, "NULL d_radiance");
    if (B > 0 && !tangent_alpha) return fail(EPSM_EINVAL, what, "NULL tangent_alpha");
    T.tangent = tangent_alpha; T.d_radiance = d_radiance;
    return launch_checked(what, epsm_bsdf_kernel<false>, ba::partial_rows(N), 128, stream, T);
}
