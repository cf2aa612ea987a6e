// epsm_trace_bsdf.h -- per-path code of the roughness adjoint (include/epsm_trace.h, epsm_trace_paths_bsdf_backward /
// epsm_trace_paths_bsdf_forward): d L / d alpha of every `roughconductor` BSDF whose alpha_slot >= 0.
//
// A path is replayed through path_bounce (epsm_trace_core.h) under the primal seed, as epsm_trace_paths_color traced it; an
// observer (AlphaObserver) turns each bounce into at most two ITEMS -- an alpha slot and a per-channel coefficient -- and a sink
// either sums adj . coef per slot (backward) or adds coef x tangent[slot] to the path's radiance tangent (forward): one is the
// other's transpose.  PRB's rules (prb.py:145-158, 209-226), sampling, Russian roulette and the MIS weights detached.  At an active
// bounce whose vertex k carries an attached roughconductor (through `twosided` as bsdf_eval_pdf flips it):
//   * indirect term: everything the path collects behind the bounce, L_ind = radiance - (L + Le + Lr_dir), carries the factor
//     weight = f(wi, wo) / pdf of the sampled wo, sampling detached:  coef_c = L_ind,c  d f_c / d alpha / (weight_c pdf), zero where
//     weight_c pdf = 0 (prb.py:217-218) or the term is not finite;
//   * emitter sample: Lr_dir = beta mis_em f(wo_em) em_weight, mis_em detached:  coef_c = Lr_dir,c  d ln f_c(wo_em) / d alpha, zero
//     where f_c = 0; an occluded sample has Lr_dir = 0 and adds nothing.
// d f_c / d alpha = f_c  d ln(D G) / d alpha at the half vector (rough_dlog_dalpha): one scalar for the three channels.
// Unlike a texel, alpha is not a linear factor of the radiance, so nothing is divided out of it: the value f is evaluated anew.
// Plain C++, compiled by hipcc for gfx950 and by g++ for the host harness (tests/host_harness/trace_bsdf_host.cpp).
#pragma once

#include "epsm_trace_replay.h"

namespace epsm {
namespace ba {

constexpr int kMaxSlots = EPSM_MAX_ALPHA_GRADS;
constexpr int kBlock = 128;                       // paths per row of partial sums (the device's workgroup)

struct BsdfArgs {
    TraceArgs A;
    const float *radiance;                        // (N,3) of the primal pass
    const float *adj;                             // backward: (N,3) d loss / d radiance
    float *d_radiance;                            // forward: (N,3) written
    const float *tangent;                         // forward: (n_slots) d alpha
    float *partial;                               // backward: (ceil(N / kBlock), kMaxSlots) per-block sums, the workspace
    int n_slots;
};

struct Item { int slot; F3 coef; };               // slot < 0: nothing

// What one bounce of a path contributes: `a` the indirect term, `b` the emitter sample.  Shown the loop state before the bounce's
// update (epsm_trace_core.h, observe_state).
struct AlphaObserver {
    const BsdfArgs &T;
    bool has;                        // (lanes past N ride along on the device and observe nothing)
    F3 radiance;
    Item a, b;
    F3 L;

    EPSM_HD void state(const PathState &s) { L = s.L; }
    EPSM_HD void vertex(const SurfHit &si, const EpsmBsdf &bsdf, uint32_t, F3 Le, F3 Lr_dir, const EmitterSample &es, bool active_em,
                        float, const BsdfSample &bs, bool active) {
        a.slot = b.slot = -1; a.coef = b.coef = zero3<float>();
        if (!has || !active || !si.valid) return;
        if (bsdf.type != EPSM_BSDF_ROUGHCONDUCTOR_T || bsdf.alpha_slot < 0 || bsdf.alpha_slot >= T.n_slots) return;
        if (bs.valid) {
            F3 f; float pdf;
            bsdf_eval_pdf(bsdf, si.wi, bs.wo, f, pdf);
            const float dl = rough_dlog_dalpha(bsdf, si.wi, bs.wo);
            // (the order in which InlineVis::direct sums.  At the path's last vertex this is 0 only as far as the primal launch and
            // this one contract L + beta x radiance x mis alike; a residue of an ulp of L times d ln f is noise, as in TexObserver)
            const F3 ind = radiance - (L + Le + Lr_dir);
            const F3 den = bs.weight * bs.pdf;
            a.coef = finite_or_zero3(f3(den.x != 0.f ? ind.x * f.x * dl / den.x : 0.f, den.y != 0.f ? ind.y * f.y * dl / den.y : 0.f,
                                        den.z != 0.f ? ind.z * f.z * dl / den.z : 0.f));
            a.slot = bsdf.alpha_slot;
        }
        if (active_em && (Lr_dir.x != 0.f || Lr_dir.y != 0.f || Lr_dir.z != 0.f)) {   // (Lr_dir,c != 0 has f_c != 0)
            b.coef = finite_or_zero3(Lr_dir * rough_dlog_dalpha(bsdf, si.wi, to_local(si, es.d)));
            b.slot = bsdf.alpha_slot;
        }
    }
};

// The replay of path i (epsm_trace_replay.h) under an AlphaObserver.
template <class Sink>
EPSM_HD void bsdf_replay(const BsdfArgs &T, int64_t i, bool has, PathState &s, const TriHit &th0, const BvhStack &st, Sink &sink) {
    AlphaObserver obs{T, has, has ? ld3(T.radiance + 3 * i) : zero3<float>()};
    obs.a.slot = obs.b.slot = -1; obs.a.coef = obs.b.coef = obs.L = zero3<float>();
    replay_path(T.A, i, has, s, th0, st, obs, sink);
}

// Backward, per path: sum over its items of adj . coef, per slot (registers: the slot is matched, never used as an index).
struct SlotSums {
    F3 adj;
    float acc[kMaxSlots];
    EPSM_HD void clear() { for (int k = 0; k < kMaxSlots; ++k) acc[k] = 0.f; }
    EPSM_HD void item(const Item &it) {
        const float v = it.slot >= 0 ? dot(adj, it.coef) : 0.f;
        for (int k = 0; k < kMaxSlots; ++k) acc[k] += it.slot == k ? v : 0.f;
    }
};

// Forward: the path's radiance tangent, sum over its items of coef x tangent[slot] (no atomics).
struct TangentSink {
    const BsdfArgs &T;
    int64_t i;
    bool has;
    F3 d;
    EPSM_HD void item(const Item &it) { if (it.slot >= 0) d = d + it.coef * T.tangent[it.slot]; }
    EPSM_HD void finish() { if (has) st3(T.d_radiance, i, d); }
};

inline int64_t partial_rows(int64_t N) { return (N + kBlock - 1) / kBlock; }
inline size_t workspace_bytes(int64_t N) { return N > 0 ? (size_t) partial_rows(N) * kMaxSlots * sizeof(float) : 0; }

// The arguments of both entry points (host side; device and host builds alike): the common eight through replay_args_fill, then
// this pass's own.  NULL = fine, otherwise what is wrong; at N == 0 fine with nothing else looked at (T.A.N = 0: the caller has
// nothing to do).
inline const char *bsdf_args_fill(BsdfArgs &T, const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                  int rr_depth, int64_t path_offset, int64_t N, const float *radiance, int B) {
    memset(&T, 0, sizeof(T));
    if (const char *why = replay_args_fill(T.A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 0)) return why;
    if (N == 0) return nullptr;
    if (!radiance) return "NULL radiance";
    if (B < 0) return "negative number of alpha slots";
    if (B > kMaxSlots) return "more than EPSM_MAX_ALPHA_GRADS alpha slots";
    T.radiance = radiance;
    T.n_slots = B;
    return nullptr;
}

}  // namespace ba
}  // namespace epsm
