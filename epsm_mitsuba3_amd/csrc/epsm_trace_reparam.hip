// epsm_trace_reparam.hip -- kernels + C ABI of the reparameterised backward pass and of its transpose, the forward pass
// (include/epsm_trace.h, epsm_trace_paths_reparam / epsm_trace_paths_reparam_forward; per-path code: epsm_trace_reparam.h).
#include <stdio.h>
#include <string.h>
#include <type_traits>

#include "epsm_common.h"
#include "epsm_trace_reparam.h"
#include "epsm_trace_replay.h"
#include "epsm_trace_packet.h"
#include "epsm_trace_launch.h"

using namespace epsm;
using epsm_host::fail;

namespace {

#ifndef EPSM_RP_THREADS
#define EPSM_RP_THREADS 64
#endif
#ifndef EPSM_RP_OCC
#define EPSM_RP_OCC 2                   // 256 registers: 3.4 KB of scratch per lane instead of 4.0 at four waves; render_backward 47.4 -> 44.9 ms (3: 46.5, 1: 45.2)
#endif
// What a lane of the three path kernels starts with: its path i of the tile and its traversal stack (an LDS column, the rest
// private); lanes past N leave.  body(i, st).
template <class Body>
__device__ __forceinline__ void path_lane(int64_t N, Body body) {
    __shared__ uint32_t s_stack[kLaneStackLds * EPSM_RP_THREADS];
    uint32_t deep[kBvhStack - kLaneStackLds];
    const int64_t i = (int64_t) blockIdx.x * EPSM_RP_THREADS + threadIdx.x;
    const BvhStack st = lane_stack(s_stack, deep, EPSM_RP_THREADS);
    if (i >= N) return;
    body(i, st);
}

// Stage 1: one lane = one path, replayed; every vertex differentiated (dual numbers, scratch: three vertex records);
// its warps are left as requests.  (First version, auxiliary rays traced by the same lane: 182 ms per render_backward
// at 4.26 M paths / 128 k triangles / 16 rays with one wave per SIMD, 99 ms with four.)
__global__ __launch_bounds__(EPSM_RP_THREADS, EPSM_RP_OCC) void epsm_reparam_path_kernel(rp::ReparamArgs R, rp::WarpReq *req, int *count) {
    path_lane(R.A.N, [&](int64_t i, const BvhStack &st) {
        rp::QueueSink sink{{req, R.A.N, i, 0}};
        // (the camera rays of a wave walked together first, as the tracers do: 41.6 -> 42.3 ms per call; not kept)
        rp::reparam_one_path(R, i, st, sink);
        count[i] = sink.n;
    });
}

// Stage 2: one lane = one auxiliary ray, a group of G lanes (G = 16, 32 or 64 >= reparam_rays) = one request.  The rays of a wave
// walk the tree TOGETHER (epsm_trace_packet.h; round 5): 46.3 -> 42.5 ms per call at 4.26 M paths / 16 rays, 26.5 -> 22.0 ms at
// 1.08 M paths / 64 rays against every lane its own walk.  A workgroup
// serves the requests of 256 consecutive paths: it lists the ones that exist -- (call n, path), n-major, so that neighbouring
// groups hold the same call of neighbouring paths: rays that start next to each other and point the same way -- and works
// through the list 256 / G requests at a time.  (Round 3 launched one group per (n, path) slot and let the empty ones leave:
// 29 % of the slots exist -- 2.06 requests per path of 7 at max_depth 3 -- and the waves that held any were 75 % full.)
// Z, dZ and the origin's adjoint are reduced over the group with xor shuffles: masks 1, 2, .., G / 2 in that order -- the order of
// the additions is part of what the passes compute.
template <int G> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v += __shfl_xor(v, m);
    return v;
}
template <int G> __device__ __forceinline__ F3 group_sum(F3 v) { return f3(group_sum<G>(v.x), group_sum<G>(v.y), group_sum<G>(v.z)); }
template <int G> __device__ __forceinline__ uint32_t group_min(uint32_t t) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) { const uint32_t u = (uint32_t) __shfl_xor((int) t, m); t = u < t ? u : t; }
    return t;
}
struct WarpLds {
    uint32_t pstack[kPacketStack * 4];                                     // one column per wave (epsm_trace_packet.h)
    uint16_t list[256 * rp::kMaxReq];                                      // (n << 8) | path of the block
    int off[rp::kMaxReq * 4 + 1];
};
// One request as its group of G lanes holds it once the auxiliary rays are walked: lane r's ray `A` (mine: the lane has one),
// Z and dZ summed over the group.
struct WarpGroup {
    bool live, mine;                   // the group has a request; this lane one of its rays
    int r, n;                          // lane of the group; the request is call n ...
    int64_t i;                         // ... of path i
    rp::WarpReq q;
    F3 d;
    rp::Aux A;
    float iZ; F3 dZ;
};
// What both stage-2 kernels do with a workgroup's requests before they part ways: list them, then, 256 / G at a time, draw each
// lane's auxiliary ray, walk the wave's rays together and reduce Z, dZ; body(g) is the backward or the forward tail.
template <int G, class Args, class Body>
__device__ __forceinline__ void for_each_warp_group(const Args &R, const rp::WarpReq *req, const int *count, int n_max, WarpLds &lds,
                                                    Body body) {
    constexpr int kGroups = 256 / G;
    const int64_t N = R.A.N, p0 = (int64_t) blockIdx.x * 256;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    int c = p0 + tid < N ? count[p0 + tid] : 0;
    c = c < n_max ? c : n_max;
    int rank[rp::kMaxReq];
#pragma unroll
    for (int n = 0; n < rp::kMaxReq; ++n) {
        const unsigned long long m = __ballot(c > n);
        rank[n] = __builtin_amdgcn_mbcnt_hi((unsigned) (m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) m, 0u));
        if (lane == 0) lds.off[n * 4 + wv] = __popcll(m);
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int e = 0; e < rp::kMaxReq * 4; ++e) { const int v = lds.off[e]; lds.off[e] = run; run += v; }
        lds.off[rp::kMaxReq * 4] = run;
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < rp::kMaxReq; ++n)
        if (c > n) lds.list[lds.off[n * 4 + wv] + rank[n]] = (uint16_t) ((n << 8) | tid);
    __syncthreads();
    const int total = lds.off[rp::kMaxReq * 4];
    WarpGroup g;
    g.r = tid % G;
    for (int b0 = 0; b0 < total; b0 += kGroups) {                          // (uniform over the workgroup: the wave walks its rays together)
        const int b = b0 + tid / G;
        g.live = b < total;
        const int e = lds.list[g.live ? b : 0];
        g.n = e >> 8;
        g.i = p0 + (e & 255);
        g.q = rp::request_slot(req, N, g.n, g.i);
        const F3 o = f3(g.q.o[0], g.q.o[1], g.q.o[2]);
        g.d = f3(g.q.d[0], g.q.d[1], g.q.d[2]);
        F3 fs, ft;
        coordinate_system(g.d, fs, ft);
        g.A.w = 0.f; g.A.dw = zero3<float>(); g.A.v = g.d; g.A.tri = kNoIndex; g.A.b1 = g.A.b2 = g.A.inv_dist = 0.f;
        g.mine = g.live && g.r < R.cfg.rays;
        // the rays of a request leave one point within a fraction of a degree, the requests of a wave are the same call of
        // neighbouring paths: the wave walks the tree once for all of them
        rp::AuxDraw D; D.ray.o = o; D.ray.d = g.d; D.ray.maxt = 0.f; D.tangent = zero3<float>(); D.sy_ = 0.f;
        if (g.mine) D = rp::aux_begin(R.cfg, rp::WarpId{0xffffffffu ^ R.A.seed, (uint32_t) (R.A.path_offset + g.i), g.n}, g.r, o, g.d, fs, ft);
        const TriHit ath = packet_intersect(R.A.S, D.ray, g.mine, lds.pstack + wv * kPacketStack);
        if (g.mine) g.A = rp::aux_finish(R.A.S, R.cfg, D, ath, o, g.d);
        g.dZ = group_sum<G>(g.A.dw);
        g.iZ = 1.f / fmaxf(group_sum<G>(g.A.w), 1e-8f);
        body(g);
    }
}

template <int G>
__global__ __launch_bounds__(256) void epsm_reparam_warp_kernel(rp::ReparamArgs R, const rp::WarpReq *req, const int *count, int n_max) {
    __shared__ WarpLds lds;
    for_each_warp_group<G>(R, req, count, n_max, lds, [&](const WarpGroup &g) {
        const rp::WarpReq &q = g.q;
        const rp::Aux &A = g.A;
        const F3 d = g.d, dZ = g.dZ, g_dir = f3(q.gdir[0], q.gdir[1], q.gdir[2]);
        const float iZ = g.iZ;
        const bool live = g.live, mine = g.mine;
        const int r = g.r;
        // the adjoint of reparam.py:269-327 at V = 0 (warp_backward, one auxiliary ray per lane)
        const F3 g_V = (g_dir - d * dot(d, g_dir)) * iZ - dZ * (q.gdiv * iZ * iZ);
        const F3 g_v = mine ? g_V * A.w + A.dw * (q.gdiv * iZ) : zero3<float>();
        F3 g_o = zero3<float>(), g_d = zero3<float>(), g_p = zero3<float>();
        uint32_t pending = 0xFFFFFFFFu;                                    // the triangle this lane still owes its share to
        if (mine) {
            if (A.tri == kNoIndex) g_d = g_v;
            else {
                g_p = (g_v - A.v * dot(A.v, g_v)) * A.inv_dist;
                g_o = -g_p;
                if (R.A.S.meshes[R.A.S.tri_mesh[A.tri]].flags & EPSM_MESH_POS_ATTACHED) pending = A.tri;
            }
        }
        // The rays of a warp mostly hit the same one or two triangles: their shares are summed over the group first, triangle
        // by triangle, and added by one lane.  (One float atomic per ray loses the small ones: a vertex's sum over 10^7 rays
        // is 10^5 times a single share, which then falls under half an ulp of it -- 2 % of a four-vertex wall's gradient at
        // 256 spp.)
        for (int round = 0; round < G; ++round) {
            const uint32_t t = group_min<G>(pending);
            if (t == 0xFFFFFFFFu) break;                                   // (uniform over the group)
            const bool sel = pending == t;
            const float b1 = sel ? A.b1 : 0.f, b2 = sel ? A.b2 : 0.f, b0 = sel ? 1.f - A.b1 - A.b2 : 0.f;
            const F3 acc0 = group_sum<G>(g_p * b0), acc1 = group_sum<G>(g_p * b1), acc2 = group_sum<G>(g_p * b2);
            if (r == 0) {
                const uint32_t *iv = R.A.S.tri + 3 * (int64_t) t;
                rp::add_vertex(R.G.pos, iv[0], acc0); rp::add_vertex(R.G.pos, iv[1], acc1); rp::add_vertex(R.G.pos, iv[2], acc2);
            }
            if (sel) pending = 0xFFFFFFFFu;
        }
        g_o = group_sum<G>(g_o); g_d = group_sum<G>(g_d);
        if (live && r == 0 && q.ftri != kNoIndex) {
            if (q.em_inv_dist != 0.f) g_o = g_o - (g_d - d * dot(d, g_d)) * q.em_inv_dist;
            rp::add_follow_point(R.A.S, R.G, q.ftri, q.fb1, q.fb2, g_o);
        }
    });
}

// ---------------------------------------------------------------------------
// the forward pass (epsm_trace_paths_reparam_forward): three launches on the backward's request layout
// ---------------------------------------------------------------------------
// Stages 1 and 3: one lane = one path, replayed.  Stage 1 (RecordSink) writes the warp requests and evaluates nothing; stage 3
// (ReadSink) reads each request's tangents back, does the dual evaluations and writes the path's d_radiance / d_film.
template <class Sink>
__global__ __launch_bounds__(EPSM_RP_THREADS, EPSM_RP_OCC) void epsm_reparam_fwd_path_kernel(rp::ReparamFwdArgs R, rp::WarpReq *req, int *count) {
    path_lane(R.A.N, [&](int64_t i, const BvhStack &st) {
        Sink sink{{req, R.A.N, i, 0}};
        rp::reparam_forward_one_path(R, i, st, sink);
        if (!Sink::kEval) count[i] = sink.n;
    });
}

// Stage 2: one lane = one auxiliary ray, a group of G lanes = one request, listed and walked as in epsm_reparam_warp_kernel (the
// same rays).  Each lane gathers the motion of its hit and of the request's glued origin; the group reduces Z, dZ and then
// sum w_i v_i', sum (dw_i - w_i dZ / Z) . v_i' (warp_forward); lane 0 writes d' and div' into the request's gdir / gdiv.
template <int G>
__global__ __launch_bounds__(256) void epsm_reparam_fwd_warp_kernel(rp::ReparamFwdArgs R, rp::WarpReq *req, const int *count, int n_max) {
    __shared__ WarpLds lds;
    for_each_warp_group<G>(R, req, count, n_max, lds, [&](const WarpGroup &g) {
        const rp::WarpReq &q = g.q;
        const F3 d = g.d;
        F3 wv3 = zero3<float>();
        float dv = 0.f;
        if (g.mine) {
            const F3 t_o = q.ftri != kNoIndex ? rp::follow_tangent(R.A.S, R.T, q.ftri, q.fb1, q.fb2) : zero3<float>();
            const F3 tv = rp::aux_tangent(R.A.S, R.T, g.A, d, t_o, q.em_inv_dist);
            wv3 = tv * g.A.w;
            dv = dot(g.A.dw - g.dZ * (g.iZ * g.A.w), tv);
        }
        wv3 = group_sum<G>(wv3); dv = group_sum<G>(dv);
        if (g.live && g.r == 0) {
            const F3 td = (wv3 - d * dot(d, wv3)) * g.iZ;
            rp::WarpReq &w = rp::request_slot(req, R.A.N, g.n, g.i);
            w.gdir[0] = td.x; w.gdir[1] = td.y; w.gdir[2] = td.z; w.gdiv = dv * g.iZ;
        }
    });
}

// What an entry point launches on: the two halves of its workspace and the grid of the path kernels
struct Stages { rp::WarpReq *req; int *count; dim3 path_grid; };

// What both entry points do before their first launch: the common arguments (replay_args_fill), N == 0, the entry point's own
// NULL check (`null_why`: its finding, made by the caller), the workspace, the pass's cfg.  True: R.A, R.cfg and L are filled and
// there is something to launch; false: rc is what the entry point returns.
template <class Args>
bool reparam_begin(const char *what, Args &R, Stages &L, int &rc, const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp,
                   int max_depth, int rr_depth, int64_t path_offset, int64_t N, const char *null_why, int reparam_max_depth, int reparam_rays,
                   float kappa, float exponent, uint32_t flags, void *workspace, size_t workspace_bytes) {
    epsm_host::err_buf()[0] = 0;
    rc = EPSM_OK;
    const char *why = replay_args_fill(R.A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 1);
    if (!why && N == 0) return false;
    if (!why) why = null_why;
    if (!why && !workspace_ok(workspace, workspace_bytes, rp::workspace_bytes(N))) why = "workspace: 16-byte aligned, >= epsm_trace_reparam_workspace_bytes(N)";
    if (!why) why = rp::reparam_cfg_fill(R.cfg, scene, reparam_max_depth, reparam_rays, kappa, exponent, flags);
    if (why) { rc = fail(EPSM_EINVAL, what, why); return false; }
    L.req = (rp::WarpReq *) workspace;
    L.count = (int *) ((char *) workspace + rp::request_bytes(N));
    L.path_grid = dim3((unsigned) ((N + EPSM_RP_THREADS - 1) / EPSM_RP_THREADS));
    return true;
}

// Stage 2 of either pass: launch(G, grid, n_max) starts its warp kernel for groups of G = 16, 32 or 64 >= reparam_rays lanes.
template <class Launch>
int launch_warp_stage(const TraceArgs &A, int reparam_rays, Launch launch) {
    const int n_max = rp::warp_stage_n_max(A);
    const dim3 grid((unsigned) ((A.N + 255) / 256));                       // one workgroup per 256 paths (N < 2^32: checked)
    if (reparam_rays <= 16) return launch(std::integral_constant<int, 16>(), grid, n_max);
    if (reparam_rays <= 32) return launch(std::integral_constant<int, 32>(), grid, n_max);
    return launch(std::integral_constant<int, 64>(), grid, n_max);
}

}  // namespace

extern "C" size_t epsm_trace_reparam_workspace_bytes(int64_t N) { return rp::workspace_bytes(N); }

extern "C" int epsm_trace_paths_reparam(const EpsmScene *scene, const EpsmSensor *sensor,
                                        uint32_t seed, int spp, int max_depth, int rr_depth,
                                        int64_t path_offset, int64_t N,
                                        const float *radiance, const float *adj_radiance, const float *adj_film,
                                        int reparam_max_depth, int reparam_rays, float kappa, float exponent, uint32_t flags,
                                        float *grad_pos, float *grad_nrm, void *workspace, size_t workspace_bytes, void *stream) {
    static const char *what = "epsm_trace_paths_reparam";
    rp::ReparamArgs R = {};
    Stages L;
    int rc;
    if (!reparam_begin(what, R, L, rc, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N,
                       !radiance || !adj_radiance || !adj_film || !grad_pos ? "NULL per-path input or grad_pos" : nullptr, reparam_max_depth,
                       reparam_rays, kappa, exponent, flags, workspace, workspace_bytes))
        return rc;
    R.radiance = radiance; R.adj_radiance = adj_radiance; R.adj_film = adj_film;
    R.G.pos = grad_pos; R.G.nrm = grad_nrm;
    rc = launch_checked(what, epsm_reparam_path_kernel, L.path_grid, EPSM_RP_THREADS, stream, R, L.req, L.count);
    if (rc != EPSM_OK || reparam_max_depth == 0) return rc;
    return launch_warp_stage(R.A, reparam_rays, [&](auto G, dim3 grid, int n_max) {
        return launch_checked(what, epsm_reparam_warp_kernel<decltype(G)::value>, grid, 256, stream, R, L.req, L.count, n_max);
    });
}

// Stage 2 alone on requests the caller wrote (include/epsm_trace.h): the production warp kernels through launch_warp_stage.
extern "C" int epsm_probe_reparam_warps(const EpsmScene *scene, uint32_t seed, int64_t path_offset, int64_t N, int max_depth, int reparam_rays,
                                        float kappa, float exponent, uint32_t flags, int forward, float *grad_pos, const float *tan_pos,
                                        void *workspace, size_t workspace_bytes, void *stream) {
    static const char *what = "epsm_probe_reparam_warps";
    epsm_host::err_buf()[0] = 0;
    rp::WarpReq *req = (rp::WarpReq *) workspace;
    int *count = (int *) ((char *) workspace + rp::request_bytes(N > 0 ? N : 0));
    if (forward) {
        rp::ReparamFwdArgs R = {};
        if (const char *why = rp::probe_warps_fill(R, scene, seed, path_offset, N, max_depth, reparam_rays, kappa, exponent, flags, tan_pos,
                                                   workspace, workspace_bytes))
            return fail(EPSM_EINVAL, what, why);
        if (N == 0) return EPSM_OK;
        R.T.pos = tan_pos;
        return launch_warp_stage(R.A, reparam_rays, [&](auto G, dim3 grid, int n_max) {
            return launch_checked(what, epsm_reparam_fwd_warp_kernel<decltype(G)::value>, grid, 256, stream, R, req, count, n_max);
        });
    }
    rp::ReparamArgs R = {};
    if (const char *why = rp::probe_warps_fill(R, scene, seed, path_offset, N, max_depth, reparam_rays, kappa, exponent, flags, grad_pos,
                                               workspace, workspace_bytes))
        return fail(EPSM_EINVAL, what, why);
    if (N == 0) return EPSM_OK;
    R.G.pos = grad_pos;
    return launch_warp_stage(R.A, reparam_rays, [&](auto G, dim3 grid, int n_max) {
        return launch_checked(what, epsm_reparam_warp_kernel<decltype(G)::value>, grid, 256, stream, R, req, count, n_max);
    });
}

extern "C" size_t epsm_trace_reparam_forward_workspace_bytes(int64_t N) { return epsm_trace_reparam_workspace_bytes(N); }

extern "C" int epsm_trace_paths_reparam_forward(const EpsmScene *scene, const EpsmSensor *sensor,
                                                uint32_t seed, int spp, int max_depth, int rr_depth,
                                                int64_t path_offset, int64_t N, const float *radiance,
                                                const float *tan_pos, const float *tan_nrm,
                                                int reparam_max_depth, int reparam_rays, float kappa, float exponent, uint32_t flags,
                                                float *d_radiance, float *d_film, void *workspace, size_t workspace_bytes, void *stream) {
    static const char *what = "epsm_trace_paths_reparam_forward";
    rp::ReparamFwdArgs R = {};
    Stages L;
    int rc;
    if (!reparam_begin(what, R, L, rc, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N,
                       !radiance || !tan_pos || !d_radiance || !d_film ? "NULL per-path input / output or tan_pos" : nullptr, reparam_max_depth,
                       reparam_rays, kappa, exponent, flags, workspace, workspace_bytes))
        return rc;
    R.radiance = radiance; R.T.pos = tan_pos; R.T.nrm = tan_nrm; R.d_radiance = d_radiance; R.d_film = d_film;
    if (reparam_max_depth > 0) {                                           // (no warp at depth 0: stage 3 alone)
        rc = launch_checked(what, epsm_reparam_fwd_path_kernel<rp::RecordSink>, L.path_grid, EPSM_RP_THREADS, stream, R, L.req, L.count);
        if (rc != EPSM_OK) return rc;
        rc = launch_warp_stage(R.A, reparam_rays, [&](auto G, dim3 grid, int n_max) {
            return launch_checked(what, epsm_reparam_fwd_warp_kernel<decltype(G)::value>, grid, 256, stream, R, L.req, L.count, n_max);
        });
        if (rc != EPSM_OK) return rc;
    }
    return launch_checked(what, epsm_reparam_fwd_path_kernel<rp::ReadSink>, L.path_grid, EPSM_RP_THREADS, stream, R, L.req, L.count);
}
