// epsm_trace_envpose.h -- per-path code of the envmap pose adjoint (include/epsm_trace.h, epsm_trace_paths_envpose_backward /
// epsm_trace_paths_envpose_forward): d L / d omega of the environment's `to_world <- Rot(omega) to_world` (world axes, at
// omega = 0: the convention of the sensor's rotation) and d L / d ln(scale) of the envmap's `scale`.
//
// A path is replayed through path_bounce (epsm_trace_core.h) under the primal seed, as epsm_trace_paths_color traced it; an
// observer (EnvPoseObserver) turns each bounce into at most two ITEMS -- a coefficient per colour channel and a WORLD direction,
// the terms of the path's radiance that read the map: radiance = ... + sum_items coef_c L_c(d) -- and a sink either sums
// adj x (the item's four derivatives) (backward) or adds (the item's four derivatives) x tangent to the path's radiance tangent
// (forward): one is the other's transpose.  The items are the ones the texel adjoint forms for the map (epsm_trace_texture.h,
// TexObserver; restated here so that its kernels stay what they are):
//   * a ray that leaves the scene: coef = beta mis, d = the ray's direction;
//   * an emitter sample on the map: coef = beta bsdf(wo) mis_em / pdf, d = the sample's direction, only when it is not occluded
//     (where Lr_dir == 0 for want of radiance leaves that undecided, the shadow ray is traced here).
// PRB's rules (prb.py): the sampling tables and the pdfs, the MIS weights, Russian roulette and the world directions are
// detached.  The map sits at infinity -- turning it moves no visibility boundary in direction space -- so nothing is lost in
// expectation.  Per item and channel c, with g_c = d L_c / d d (env_eval_grad):
//   d / d omega     = coef_c (g_c x d)     the local direction is to_local Rot(-omega) d, so d moves by -omega x d and
//                                          g_c . (-omega x d) = omega . (g_c x d): the torque of the world-direction gradient;
//   d / d ln(scale) = coef_c L_c(d)        the texels hold bitmap x scale.
// A term that is not finite adds nothing (env_eval_grad clamps its 1 / sin^2 theta at the poles; what is left is finite, and
// finite_or_zero keeps it so).
// Plain C++, compiled by hipcc for gfx950 and by g++ for the host harness (tests/host_harness/trace_envpose_host.cpp).
#pragma once

#include "epsm_trace_replay.h"

namespace epsm {
namespace ep {

constexpr int kRow = EPSM_ENV_POSE_GRADS;         // floats per row of partial sums: omega.x, omega.y, omega.z, ln(scale)
constexpr int kBlock = 128;                       // paths per row of partial sums (the device's workgroup)

struct EnvPoseArgs {
    TraceArgs A;
    const float *radiance;                        // (N,3) of the primal pass (the entry points' common head; no item reads it)
    const float *adj;                             // backward: (N,3) d loss / d radiance
    float *d_radiance;                            // forward: (N,3) written
    const float *tangent;                         // forward: (4) d [omega, ln(scale)]
    float *partial;                               // backward: (ceil(N / kBlock), kRow) per-block sums, the workspace
};

// One term coef_c L_c(d) of the path's radiance and its derivatives: torque[c] = coef_c (g_c x d), lnscale = coef o L(d).
struct Item {
    bool on;
    F3 coef, d;                                   // (the term itself: what the host harness exports, tests/_envpose_host.py)
    F3 torque[3];
    F3 lnscale;
};
EPSM_HD void item_clear(Item &it) {
    it.on = false;
    it.coef = it.d = it.torque[0] = it.torque[1] = it.torque[2] = it.lnscale = zero3<float>();
}
EPSM_HD void item_fill(const EpsmScene &S, F3 coef, F3 d, Item &it) {
    F3 g[3];
    const F3 L = env_eval_grad(S, d, g);
    it.coef = coef; it.d = d;
    it.torque[0] = finite_or_zero3(cross(g[0], d) * coef.x);
    it.torque[1] = finite_or_zero3(cross(g[1], d) * coef.y);
    it.torque[2] = finite_or_zero3(cross(g[2], d) * coef.z);
    it.lnscale = finite_or_zero3(mul3(coef, L));
    it.on = true;
}

// What one bounce of a path contributes: `a` the escaped ray, `b` the emitter sample on the map.  Shown the loop state before
// the bounce's update (epsm_trace_core.h, observe_state).
struct EnvPoseObserver {
    const EnvPoseArgs &T;
    const BvhStack &st;
    bool has;                        // (lanes past N ride along on the device and observe nothing)
    Item a, b;
    F3 beta, dir;
    float prev_bsdf_pdf;
    bool prev_bsdf_delta;

    EPSM_HD void state(const PathState &s) {
        beta = s.beta; dir = s.ray.d; prev_bsdf_pdf = s.prev_bsdf_pdf; prev_bsdf_delta = s.prev_bsdf_delta;
    }
    EPSM_HD void vertex(const SurfHit &si, const EpsmBsdf &bsdf, uint32_t, F3, F3 Lr_dir, const EmitterSample &es, bool active_em,
                        float mis_em, const BsdfSample &, bool active) {
        item_clear(a); item_clear(b);
        if (!has || !active) return;                                          // (an inactive vertex collects nothing)
        const EpsmScene &S = T.A.S;
        if (!si.valid) {                                                       // the ray left the scene (path_bounce's Le)
            float em_pdf = prev_bsdf_delta ? 0.f : env_pdf(S, dir);
            if (S.n_emitters > 1) em_pdf /= (float) S.n_emitters;
            item_fill(S, finite_or_zero3(beta * mis_weight(prev_bsdf_pdf, em_pdf)), dir, a);
        }
        if (active_em && es.emitter == S.env.emitter && es.pdf != 0.f) {
            F3 bval; float bpdf;
            bsdf_eval_pdf(bsdf, si.wi, to_local(si, es.d), bval, bpdf);
            const F3 c = mul3(beta, bval) * (mis_em / es.pdf);
            if (c.x != 0.f || c.y != 0.f || c.z != 0.f) {
                // visible?  path_bounce zeroed Lr_dir when the shadow ray was blocked; where Lr_dir is zero for want of radiance
                // (env(d) = 0 in every channel the coefficient has) that ray was not traced: trace it here
                bool visible = Lr_dir.x != 0.f || Lr_dir.y != 0.f || Lr_dir.z != 0.f;
                if (!visible) {
                    const F3 Ld = env_eval(S, es.d);
                    const bool decided = (c.x != 0.f && Ld.x != 0.f) || (c.y != 0.f && Ld.y != 0.f) || (c.z != 0.f && Ld.z != 0.f);
                    if (!decided) {
                        float dist;
                        visible = !intersect<true>(S, spawn_ray_to(si, es.p, dist), st).hit;
                    }
                }
                if (visible) item_fill(S, finite_or_zero3(c), es.d, b);
            }
        }
    }
};

// The replay of path i (epsm_trace_replay.h) under an EnvPoseObserver.
template <class Sink>
EPSM_HD void envpose_replay(const EnvPoseArgs &T, int64_t i, bool has, PathState &s, const TriHit &th0, const BvhStack &st, Sink &sink) {
    EnvPoseObserver obs{T, st, has};
    item_clear(obs.a); item_clear(obs.b);
    obs.beta = obs.dir = zero3<float>(); obs.prev_bsdf_pdf = 1.f; obs.prev_bsdf_delta = true;
    replay_path(T.A, i, has, s, th0, st, obs, sink);
}

// Backward, per path: acc[k] += sum_c adj_c M[c][k] over its items, M[c] = (torque[c].x, torque[c].y, torque[c].z, lnscale_c).
struct EnvPoseSums {
    F3 adj;
    float acc[kRow];
    EPSM_HD void clear() { for (int k = 0; k < kRow; ++k) acc[k] = 0.f; }
    EPSM_HD void item(const Item &it) {
        if (!it.on) return;
        const F3 w = it.torque[0] * adj.x + it.torque[1] * adj.y + it.torque[2] * adj.z;
        acc[0] += w.x; acc[1] += w.y; acc[2] += w.z;
        acc[3] += dot(adj, it.lnscale);
    }
};

// Forward: the path's radiance tangent, d_c += sum_k M[c][k] tangent[k] over its items (no atomics).
struct EnvPoseTangentSink {
    const EnvPoseArgs &T;
    int64_t i;
    bool has;
    F3 d;
    EPSM_HD void item(const Item &it) {
        if (!it.on) return;
        const F3 w = ld3(T.tangent);
        d = d + f3(dot(it.torque[0], w), dot(it.torque[1], w), dot(it.torque[2], w)) + it.lnscale * T.tangent[3];
    }
    EPSM_HD void finish() { if (has) st3(T.d_radiance, i, d); }
};

inline int64_t partial_rows(int64_t N) { return (N + kBlock - 1) / kBlock; }
inline size_t workspace_bytes(int64_t N) { return N > 0 ? (size_t) partial_rows(N) * kRow * sizeof(float) : 0; }

// The arguments of both entry points (host side; device and host builds alike): the common eight through replay_args_fill, then
// this pass's own.  NULL = fine, otherwise what is wrong; at N == 0 fine with nothing else looked at (T.A.N = 0: the caller has
// nothing to do).
inline const char *envpose_args_fill(EnvPoseArgs &T, const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp,
                                     int max_depth, int rr_depth, int64_t path_offset, int64_t N, const float *radiance) {
    memset(&T, 0, sizeof(T));
    if (const char *why = replay_args_fill(T.A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 0)) return why;
    if (N == 0) return nullptr;
    if (scene->env.kind != EPSM_ENV_ENVMAP) return "the scene's environment is not an envmap (env.kind != EPSM_ENV_ENVMAP)";
    if (!radiance) return "NULL radiance";
    T.radiance = radiance;
    return nullptr;
}

}  // namespace ep
}  // namespace epsm
