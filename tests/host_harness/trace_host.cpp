// TEST HARNESS ONLY: compiles the tracer's per-path code (epsm_trace_core.h) for the host CPU so
// that the analytic known-answer tests of tests/test_tracer_*.py run without a GPU.  Same entry
// point names as the product library; host pointers.  Not shipped, not a fallback.
#include <math.h>
#include <string.h>
#include "../../epsm_mitsuba3_amd/csrc/epsm_trace_replay.h"
#include "../../epsm_mitsuba3_amd/csrc/epsm_trace_wavefront.h"
#include "../../epsm_mitsuba3_amd/csrc/epsm_trace_reparam.h"
#include "../../epsm_mitsuba3_amd/csrc/epsm_probe_core.h"

using namespace epsm;

// Paths [lo, hi) of a tile one by one, each on its own stack with its primary ray traced: body(i, s, th0, st) -- what the device
// kernels' prologue hands a lane (epsm_trace_packet.h) -- and the whole tile, OpenMP over chunks of 256 paths.
template <class Body> void for_each_path(const TraceArgs &A, int64_t lo, int64_t hi, Body body) {
    for (int64_t i = lo; i < hi; ++i) {
        uint32_t stack[kBvhStack];
        const BvhStack st{stack, 1};
        PathState s = path_begin(A, i, false);
        const TriHit th0 = intersect<false>(A.S, s.ray, st);
        body(i, s, th0, st);
    }
}
template <class Body> void for_each_path(const TraceArgs &A, Body body) {
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t lo = 0; lo < A.N; lo += 256) for_each_path(A, lo, lo + 256 < A.N ? lo + 256 : A.N, body);
}

extern "C" int epsm_trace_paths(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                int rr_depth, int64_t path_offset, int64_t N, int K_log, float *ray_o, float *ray_d,
                                float *ray_dx, float *ray_dy, float *film_pos, float *radiance, uint8_t *valid,
                                const EpsmRecordOut *recs, uint32_t flags, void *) {
    if (scene && sensor && N == 0) return 0;
    TraceArgs A;
    if ((flags & EPSM_TRACE_FUSE_FIRST_HIT) || trace_args_fill(A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, K_log, ray_o, ray_d,
                                                               ray_dx, ray_dy, film_pos, radiance, valid, recs, flags))
        return -22;                                                        // (refused as the device library refuses it)
#pragma omp parallel for schedule(dynamic, 256)
    for (int64_t i = 0; i < N; ++i) {
        uint32_t stack[kBvhStack];
        trace_one_path(A, i, BvhStack{stack, 1});
    }
    return 0;
}

extern "C" int epsm_trace_paths_color(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                      int rr_depth, int64_t path_offset, int64_t N, float *film_pos, float *radiance,
                                      uint8_t *valid, float *color_sum, int n_color, void *) {
    TraceArgs A;
    if (replay_args_fill(A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 1)) return -22;
    if (N == 0) return 0;
    A.film_pos = film_pos; A.radiance = radiance; A.valid = valid;
    A.color_sum = color_sum; A.n_color = n_color;
    memset(color_sum, 0, (size_t) N * n_color * 3 * sizeof(float));
#pragma omp parallel for schedule(dynamic, 256)
    for (int64_t i = 0; i < N; ++i) {
        uint32_t stack[kBvhStack];
        trace_one_path(A, i, BvhStack{stack, 1});
    }
    return 0;
}

// The paths of a reparameterised pass (backward here, forward in trace_fwd_host.cpp), OpenMP over them: body(i, st, W, id) with
// the path's stack, the Warp its inline sink collects the auxiliary rays in, and the id of its first warp -- path
// path_offset + i under the reparameterisation's own seed, call 0 (rp::WarpId).
template <class Body> void for_each_reparam_path(const TraceArgs &A, Body body) {
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t i = 0; i < A.N; ++i) {
        uint32_t stack[kBvhStack];
        rp::Warp W;
        body(i, BvhStack{stack, 1}, W, rp::WarpId{0xffffffffu ^ A.seed, (uint32_t) (A.path_offset + i), 0});
    }
}

extern "C" int epsm_trace_paths_reparam(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                        int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                        const float *adj_radiance, const float *adj_film, int reparam_max_depth, int reparam_rays,
                                        float kappa, float exponent, uint32_t flags, float *grad_pos, float *grad_nrm, void *, size_t,
                                        void *) {
    rp::ReparamArgs R = {};
    if (replay_args_fill(R.A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 1)) return -22;
    if (N == 0) return 0;
    if (rp::reparam_cfg_fill(R.cfg, scene, reparam_max_depth, reparam_rays, kappa, exponent, flags)) return -22;   // (as the device library)
    R.radiance = radiance; R.adj_radiance = adj_radiance; R.adj_film = adj_film;
    R.G.pos = grad_pos; R.G.nrm = grad_nrm;
    for_each_reparam_path(R.A, [&](int64_t i, const BvhStack &st, rp::Warp &W, const rp::WarpId &id) {
        rp::InlineSink sink{R.A.S, R.cfg, R.G, st, W, id};
        rp::reparam_one_path(R, i, st, sink);
    });
    return 0;
}
extern "C" size_t epsm_trace_reparam_workspace_bytes(int64_t) { return 0; }

// epsm_probe_reparam_warps (include/epsm_trace.h) on host pointers: the live requests of the caller's workspace one after the
// other, each as InlineSink::warp / InlineFwdSink::warp treat a warp -- its auxiliary rays traced in turn, summed in double.
extern "C" int epsm_probe_reparam_warps(const EpsmScene *scene, uint32_t seed, int64_t path_offset, int64_t N, int max_depth, int reparam_rays,
                                        float kappa, float exponent, uint32_t flags, int forward, float *grad_pos, const float *tan_pos,
                                        void *workspace, size_t workspace_bytes, void *) {
    rp::ReparamArgs R = {};
    if (rp::probe_warps_fill(R, scene, seed, path_offset, N, max_depth, reparam_rays, kappa, exponent, flags,
                             forward ? (const void *) tan_pos : (const void *) grad_pos, workspace, workspace_bytes))
        return -22;                                                        // (refused as the device library refuses it)
    if (N == 0) return 0;
    rp::WarpReq *req = (rp::WarpReq *) workspace;
    const int *count = (const int *) ((const char *) workspace + rp::request_bytes(N));
    const int n_max = rp::warp_stage_n_max(R.A);
    const EpsmScene &S = R.A.S;
    const rp::GradOut G{grad_pos, nullptr};
    const rp::TanIn T{tan_pos, nullptr};
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t i = 0; i < N; ++i) {
        uint32_t stack[kBvhStack];
        rp::Warp W;
        const int c = count[i] < n_max ? count[i] : n_max;
        for (int n = 0; n < c; ++n) {
            rp::WarpReq &q = rp::request_slot(req, N, n, i);
            const F3 o = f3(q.o[0], q.o[1], q.o[2]), d = f3(q.d[0], q.d[1], q.d[2]);
            rp::warp_collect(S, R.cfg, rp::WarpId{0xffffffffu ^ seed, (uint32_t) (path_offset + i), n}, o, d, BvhStack{stack, 1}, W);
            if (forward) {
                const F3 t_o = q.ftri != kNoIndex ? rp::follow_tangent(S, T, q.ftri, q.fb1, q.fb2) : zero3<float>();
                const rp::WarpTan t = rp::warp_forward(S, T, W, t_o, q.em_inv_dist);
                q.gdir[0] = t.dir.x; q.gdir[1] = t.dir.y; q.gdir[2] = t.dir.z; q.gdiv = t.div;
            } else {
                F3 g_o, g_d;
                rp::warp_backward(S, G, W, f3(q.gdir[0], q.gdir[1], q.gdir[2]), q.gdiv, g_o, g_d);
                if (q.em_inv_dist != 0.f) g_o = g_o - (g_d - d * dot(d, g_d)) * q.em_inv_dist;
                if (q.ftri != kNoIndex) rp::add_follow_point(S, G, q.ftri, q.fb1, q.fb2, g_o);
            }
        }
    }
    return 0;
}

// Test probe: the warp field's value and divergence at one ray when only the ray ORIGIN moves with velocity `odot`
// (forward mode of reparam.py:155-221): out = [V_theta (3), div V_theta, Z].
extern "C" int epsm_debug_warp(const EpsmScene *scene, const float *o, const float *d, const float *odot, int rays, float kappa,
                               float exponent, uint32_t flags, uint32_t seed, float *out) {
    rp::ReparamCfg cfg; cfg.max_depth = 8; cfg.rays = rays; cfg.kappa = kappa; cfg.exponent = exponent; cfg.flags = flags;
    uint32_t stack[kBvhStack];
    rp::Warp W;
    rp::warp_collect(*scene, cfg, rp::WarpId{seed, 0u, 0}, ld3(o), ld3(d), BvhStack{stack, 1}, W);
    double V[3] = {0, 0, 0}, dl = 0;
    const F3 od = ld3(odot);
    for (int i = 0; i < W.n; ++i) {
        const rp::Aux &A = W.a[i];
        if (A.tri == kNoIndex) continue;
        const F3 dv = (od - A.v * dot(A.v, od)) * (-A.inv_dist);
        V[0] += A.w * dv.x; V[1] += A.w * dv.y; V[2] += A.w * dv.z;
        dl += dot(A.dw, dv);
    }
    const double Z = W.Z > 1e-8f ? W.Z : 1e-8;
    out[0] = (float) (V[0] / Z); out[1] = (float) (V[1] / Z); out[2] = (float) (V[2] / Z);
    out[3] = (float) ((dl - (out[0] * W.dZ.x + out[1] * W.dZ.y + out[2] * W.dZ.z)) / Z);
    out[4] = W.Z;
    return 0;
}
// Test probe: the environment's radiance along d, its derivative w.r.t. d (3 x 3, row c = d L_c / d d) and the sampling density:
// out = [L (3), dL/dd (9), pdf]
extern "C" int epsm_debug_env(const EpsmScene *scene, const float *d, float *out) {
    if (!has_environment(*scene)) return -22;
    F3 g[3];
    const F3 L = env_eval_grad(*scene, ld3(d), g);
    const F3 L2 = env_eval(*scene, ld3(d));
    if (L.x != L2.x || L.y != L2.y || L.z != L2.z) return -1;
    out[0] = L.x; out[1] = L.y; out[2] = L.z;
    for (int c = 0; c < 3; ++c) { out[3 + 3 * c] = g[c].x; out[4 + 3 * c] = g[c].y; out[5 + 3 * c] = g[c].z; }
    out[12] = env_pdf(*scene, ld3(d));
    return 0;
}
// Test probe: the hand-written ADJOINT of the same warp (same seed -> same auxiliary rays): d loss / d ray.o for given
// d loss / d direction and d loss / d divergence.  No mesh need be attached: grad_pos may be null-sized.
extern "C" int epsm_debug_warp_adjoint(const EpsmScene *scene, const float *o, const float *d, const float *g_dir, float g_div, int rays,
                                       float kappa, float exponent, uint32_t flags, uint32_t seed, float *grad_pos, float *out) {
    rp::ReparamCfg cfg; cfg.max_depth = 8; cfg.rays = rays; cfg.kappa = kappa; cfg.exponent = exponent; cfg.flags = flags;
    uint32_t stack[kBvhStack];
    rp::Warp W;
    rp::warp_collect(*scene, cfg, rp::WarpId{seed, 0u, 0}, ld3(o), ld3(d), BvhStack{stack, 1}, W);
    rp::GradOut G; G.pos = grad_pos; G.nrm = nullptr;
    F3 g_o, g_d;
    rp::warp_backward(*scene, G, W, ld3(g_dir), g_div, g_o, g_d);
    out[0] = g_o.x; out[1] = g_o.y; out[2] = g_o.z; out[3] = g_d.x; out[4] = g_d.y; out[5] = g_d.z;
    return 0;
}

// The wavefront form, stage by stage as the device launches them (serial loops in place of the kernels; the queues
// are appended in path order here, on the device in the order the waves arrive -- per-path results do not depend on it).
extern "C" size_t epsm_trace_workspace_bytes(int64_t N) { return N > 0 ? wf_workspace_bytes(N) : 0; }
extern "C" int epsm_trace_paths_wavefront(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                          int rr_depth, int64_t path_offset, int64_t N, int K_log, float *ray_o, float *ray_d,
                                          float *ray_dx, float *ray_dy, float *film_pos, float *radiance, uint8_t *valid,
                                          const EpsmRecordOut *recs, uint32_t flags, void *workspace, size_t workspace_bytes, void *) {
    if (scene && sensor && N == 0) return 0;
    TraceArgs A;
    if (trace_args_fill(A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, K_log, ray_o, ray_d, ray_dx, ray_dy, film_pos,
                        radiance, valid, recs, flags))
        return -22;                                                        // (refused as the device library refuses it)
    if (!workspace || workspace_bytes < wf_workspace_bytes(N)) return -22;
    const WfState W = wf_carve(workspace, N);
    memset(W.counters, 0, kWfCounters * sizeof(uint32_t));
    uint32_t stack[kWfStackLds];
    for (int b = 0; b < path_max_depth(A); ++b) {
        const int64_t count = b == 0 ? N : (int64_t) W.counters[wf_alive_counter(b)];
        const auto path = [&](int64_t q) { return b == 0 ? q : (int64_t) W.queue[b & 1][q]; };
        uint32_t &n_alive = W.counters[wf_alive_counter(b + 1)], &n_shadow = W.counters[wf_shadow_counter(b)];
        for (int64_t q = 0; q < count; ++q) wf_extend(A, W, path(q), stack, 1, b);
        for (int64_t q = 0; q < count; ++q) {
            const int64_t i = path(q);
            bool alive, shadow;
            WfFirstHit fh;
            const bool fuse = b == 0 && (flags & EPSM_TRACE_FUSE_FIRST_HIT);
            wf_shade(A, W, i, b, alive, shadow, fuse ? &fh : nullptr);
            if (fuse) {                                                     // (the device sums over the wave first: epsm_trace.hip, first_hit_scatter)
                auto add = [](float *p, float v) { if (first_hit_addend_kept(v)) *p += v; };
                if (A.fh.grad_o_sum) { add(A.fh.grad_o_sum, -fh.gd.x); add(A.fh.grad_o_sum + 1, -fh.gd.y); add(A.fh.grad_o_sum + 2, -fh.gd.z); }
                if (fh.rows.on)
                    for (int j = 0; j < 3; ++j) {
                        float *p = A.fh.grad_pos + 3 * (int64_t) fh.rows.key[j];
                        add(p, fh.rows.val[j].x); add(p + 1, fh.rows.val[j].y); add(p + 2, fh.rows.val[j].z);
                    }
            }
            if (alive) W.queue[(b + 1) & 1][n_alive++] = (uint32_t) i;
            if (shadow) W.shadow_queue[n_shadow++] = (uint32_t) i;
        }
        for (int64_t q = 0; q < (int64_t) n_shadow; ++q) wf_shadow(A, W, (int64_t) W.shadow_queue[q], b, stack, 1);
    }
    if (A.radiance || A.valid || !(A.flags & EPSM_TRACE_PACKED_LOG))           // as the device entry point
        for (int64_t i = 0; i < N; ++i) wf_finish(A, W, i);
    return 0;
}

extern "C" int epsm_film_splat(int64_t N, const float *pos, const float *rad, int W, int H, int rfilter, float *accum, void *) {
    for (int64_t i = 0; i < N; ++i) {
        const float px = pos[2 * i], py = pos[2 * i + 1];
        if (rfilter == EPSM_RFILTER_BOX) {
            const int x = (int) floorf(px), y = (int) floorf(py);
            if (x < 0 || y < 0 || x >= W || y >= H) continue;
            float *a = accum + 4 * ((int64_t) y * W + x);
            a[0] += rad[3 * i]; a[1] += rad[3 * i + 1]; a[2] += rad[3 * i + 2]; a[3] += 1.f;
            continue;
        }
        const float radius = kGaussRadius;
        const int x0 = (int) ceilf(px - radius - 0.5f), x1 = (int) floorf(px + radius - 0.5f);
        const int y0 = (int) ceilf(py - radius - 0.5f), y1 = (int) floorf(py + radius - 0.5f);
        for (int y = y0; y <= y1; ++y) {
            if (y < 0 || y >= H) continue;
            const float dy = (y + 0.5f) - py, wy = gaussian_rfilter(dy);
            for (int x = x0; x <= x1; ++x) {
                if (x < 0 || x >= W) continue;
                const float dx = (x + 0.5f) - px, w = wy * gaussian_rfilter(dx);
                float *a = accum + 4 * ((int64_t) y * W + x);
                a[0] += rad[3 * i] * w; a[1] += rad[3 * i + 1] * w; a[2] += rad[3 * i + 2] * w; a[3] += w;
            }
        }
    }
    return 0;
}
extern "C" int epsm_film_develop(int W, int H, const float *accum, float *image, void *) {
    for (int64_t i = 0; i < (int64_t) W * H; ++i) {
        const float w = accum[4 * i + 3], iw = w != 0.f ? 1.f / w : 0.f;
        image[3 * i] = accum[4 * i] * iw; image[3 * i + 1] = accum[4 * i + 1] * iw; image[3 * i + 2] = accum[4 * i + 2] * iw;
    }
    return 0;
}

// epsm_probe (include/epsm_trace.h) on host pointers: the same probe_row the device kernel runs
extern "C" int epsm_probe(int what, int64_t n, const float *in, float *out, const void *cfg, void *) {
    if (what < 0 || what >= EPSM_PROBE_COUNT || n < 0 || (n > 0 && (!in || !out))) return -22;
    if ((probe_needs_bsdf(what) || probe_needs_sensor(what)) && !cfg) return -22;
    EpsmBsdf bsdf = {};
    EpsmSensor sensor = {};
    if (probe_needs_bsdf(what)) bsdf = *(const EpsmBsdf *) cfg;
    if (probe_needs_sensor(what)) sensor = *(const EpsmSensor *) cfg;
    for (int64_t i = 0; i < n; ++i) probe_row(what, in + i * EPSM_PROBE_IN, out + i * EPSM_PROBE_OUT, &bsdf, &sensor);
    return 0;
}

// epsm_probe_rays (include/epsm_trace.h) on host pointers: the tracer's intersect on caller-given rays, on the two stacks the
// entry points above give a path -- kBvhStack words of its own (epsm_trace_paths), or kWfStackLds words and the rest in the
// workspace at ovf + i, stride n (epsm_trace_paths_wavefront).  The wave-packet walk is device code: refused here.
extern "C" size_t epsm_probe_rays_workspace_bytes(int form, int64_t n) {
    return probe_rays_wavefront_form(form) && n > 0 ? (size_t) n * 4 * kWfStackOvf : 0;
}
extern "C" int epsm_probe_rays(const EpsmScene *scene, int form, int64_t n, const float *rays, uint32_t *out, void *workspace,
                               size_t workspace_bytes, void *) {
    if (probe_rays_refusal(scene, form, n, rays, out, workspace, workspace_bytes, epsm_probe_rays_workspace_bytes(form, n))) return -22;
    if (form == EPSM_RAYS_PACKET) return -22;
    const bool any = form == EPSM_RAYS_LANE_ANY || form == EPSM_RAYS_WAVEFRONT_ANY;
    WfState W = {};
    W.stack_ovf = (uint32_t *) workspace; W.N = n;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t stack[kBvhStack];
        const BvhStack st = probe_rays_wavefront_form(form) ? wf_stack(W, i, stack, 1) : BvhStack{stack, 1};
        if (any) probe_ray_row<true>(*scene, rays + i * EPSM_RAYS_IN, out + i * EPSM_RAYS_OUT, st);
        else probe_ray_row<false>(*scene, rays + i * EPSM_RAYS_IN, out + i * EPSM_RAYS_OUT, st);
    }
    return 0;
}
