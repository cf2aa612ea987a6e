// epsm_trace_probe.hip -- epsm_probe (include/epsm_trace.h): the tracer's per-path functions on plain numbers, on the device;
// epsm_probe_rays: its BVH traversal on caller-given rays, on the stacks its kernels use.
#include "epsm_common.h"
#include "../../include/epsm_trace.h"
#include "epsm_probe_core.h"
#include "epsm_trace_wavefront.h"        // wf_stack, kWfStackLds
#include "epsm_trace_packet.h"           // lane_stack, packet_intersect

using namespace epsm;
using epsm_host::fail;

namespace {
__global__ __launch_bounds__(256) void epsm_probe_kernel(int what, int64_t n, const float *in, float *out, EpsmBsdf bsdf, EpsmSensor sensor) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i < n) probe_row(what, in + i * EPSM_PROBE_IN, out + i * EPSM_PROBE_OUT, &bsdf, &sensor);
}

// ---- epsm_probe_rays: one ray per lane, 128 lanes per workgroup as the tracer's traversal kernels ----
constexpr int kRayThreads = 128;
// the one-launch kernels' stack (epsm_trace_kernel, epsm_trace.hip): 32 entries per lane in LDS, the rest private
template <bool ANY_HIT>
__global__ __launch_bounds__(kRayThreads) void epsm_probe_rays_lane_kernel(EpsmScene S, int64_t n, const float *rays, uint32_t *out) {
    __shared__ uint32_t s_stack[kLaneStackLds * kRayThreads];
    uint32_t deep[kBvhStack - kLaneStackLds];
    const int64_t i = (int64_t) blockIdx.x * kRayThreads + threadIdx.x;
    const BvhStack st = lane_stack(s_stack, deep, kRayThreads);
    if (i < n) probe_ray_row<ANY_HIT>(S, rays + i * EPSM_RAYS_IN, out + i * EPSM_RAYS_OUT, st);
}
// the wavefront kernels' stack (epsm_wf_extend_kernel): 16 entries per lane in LDS, the rest at ovf + i with stride n
template <bool ANY_HIT>
__global__ __launch_bounds__(kRayThreads) void epsm_probe_rays_wavefront_kernel(EpsmScene S, int64_t n, const float *rays, uint32_t *out,
                                                                                uint32_t *ovf) {
    __shared__ uint32_t s_stack[kWfStackLds * kRayThreads];
    const int64_t i = (int64_t) blockIdx.x * kRayThreads + threadIdx.x;
    if (i >= n) return;
    WfState W = {};
    W.stack_ovf = ovf; W.N = n;
    probe_ray_row<ANY_HIT>(S, rays + i * EPSM_RAYS_IN, out + i * EPSM_RAYS_OUT, wf_stack(W, i, s_stack + threadIdx.x, kRayThreads));
}
// the wave-packet walk (epsm_wf_extend_packet_kernel): rows 64 w .. 64 w + 63 are one wave, all of whose lanes call it
__global__ __launch_bounds__(kRayThreads) void epsm_probe_rays_packet_kernel(EpsmScene S, int64_t n, const float *rays, uint32_t *out) {
    __shared__ uint32_t s_stack[kPacketStack * (kRayThreads / 64)];
    const int wv = threadIdx.x >> 6;
    const int64_t i = (int64_t) blockIdx.x * kRayThreads + threadIdx.x;
    Ray r; r.o = zero3<float>(); r.d = f3(0.f, 0.f, 1.f); r.maxt = 0.f;
    const bool has = i < n && probe_ray_load(rays + i * EPSM_RAYS_IN, r);
    const TriHit th = packet_intersect(S, r, has, s_stack + wv * kPacketStack);
    if (i < n) probe_ray_store(out + i * EPSM_RAYS_OUT, th);
}
}  // namespace

extern "C" size_t epsm_probe_rays_workspace_bytes(int form, int64_t n) {
    return probe_rays_wavefront_form(form) && n > 0 ? (size_t) n * 4 * kWfStackOvf : 0;
}
extern "C" int epsm_probe_rays(const EpsmScene *scene, int form, int64_t n, const float *rays, uint32_t *out, void *workspace,
                               size_t workspace_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (const char *why = probe_rays_refusal(scene, form, n, rays, out, workspace, workspace_bytes, epsm_probe_rays_workspace_bytes(form, n)))
        return fail(EPSM_EINVAL, why);
    if (n == 0) return EPSM_OK;
    const dim3 grid((unsigned) ((n + kRayThreads - 1) / kRayThreads)), block(kRayThreads);
    hipStream_t s = (hipStream_t) stream;
    switch (form) {
        case EPSM_RAYS_LANE: hipLaunchKernelGGL(epsm_probe_rays_lane_kernel<false>, grid, block, 0, s, *scene, n, rays, out); break;
        case EPSM_RAYS_LANE_ANY: hipLaunchKernelGGL(epsm_probe_rays_lane_kernel<true>, grid, block, 0, s, *scene, n, rays, out); break;
        case EPSM_RAYS_WAVEFRONT:
            hipLaunchKernelGGL(epsm_probe_rays_wavefront_kernel<false>, grid, block, 0, s, *scene, n, rays, out, (uint32_t *) workspace); break;
        case EPSM_RAYS_WAVEFRONT_ANY:
            hipLaunchKernelGGL(epsm_probe_rays_wavefront_kernel<true>, grid, block, 0, s, *scene, n, rays, out, (uint32_t *) workspace); break;
        default: hipLaunchKernelGGL(epsm_probe_rays_packet_kernel, grid, block, 0, s, *scene, n, rays, out); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return epsm_host::hip_fail("epsm_probe_rays", e);
    return EPSM_OK;
}

extern "C" int epsm_probe(int what, int64_t n, const float *in, float *out, const void *cfg, void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (what < 0 || what >= EPSM_PROBE_COUNT) return fail(EPSM_EINVAL, "epsm_probe: unknown function");
    if (n == 0) return EPSM_OK;
    if (n < 0 || !in || !out) return fail(EPSM_EINVAL, "epsm_probe: bad argument");
    if ((probe_needs_bsdf(what) || probe_needs_sensor(what)) && !cfg) return fail(EPSM_EINVAL, "epsm_probe: this function needs cfg");
    EpsmBsdf bsdf = {};
    EpsmSensor sensor = {};
    if (probe_needs_bsdf(what)) bsdf = *(const EpsmBsdf *) cfg;
    if (probe_needs_sensor(what)) sensor = *(const EpsmSensor *) cfg;
    hipLaunchKernelGGL(epsm_probe_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, (hipStream_t) stream, what, n, in, out,
                       bsdf, sensor);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return epsm_host::hip_fail("epsm_probe", e);
    return EPSM_OK;
}
