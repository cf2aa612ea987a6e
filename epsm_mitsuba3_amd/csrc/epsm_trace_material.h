// epsm_trace_material.h -- per-path code of the conductor material adjoint (include/epsm_trace.h, epsm_trace_paths_material_backward /
// epsm_trace_paths_material_forward): d L / d eta, d L / d k and d L / d specular_reflectance, per colour channel, of every
// `conductor` / `roughconductor` BSDF whose `material` word names a slot.
//
// A path is replayed through path_bounce (epsm_trace_core.h) under the primal seed, as epsm_trace_paths_color traced it; an
// observer (MaterialObserver) turns each bounce into at most two ITEMS -- a material slot and three per-channel coefficients --
// and a sink either sums adj x coef per slot, parameter and channel (backward) or adds coef x tangent[slot] to the path's
// radiance tangent (forward): one is the other's transpose.  PRB's rules (prb.py:145-158, 209-226).  bsdf_sample's weight is
// F(cos; eta, k) x specular_reflectance x w with w, the pdf and the direction free of all three (conductor.cpp:235-270,
// roughconductor.cpp:225-300), so the detached sampling and the detached MIS weights lose nothing: below the Russian-roulette
// depth the sums are the derivative of what is rendered.  At an active bounce on an attached BSDF (through `twosided` as
// bsdf_sample / bsdf_eval_pdf flip it), per channel c:
//   * the sampled direction: everything the path collects behind the bounce, L_ind = radiance - (L + Le + Lr_dir), carries the
//     factor F_c R_c:  c_eta,c = L_ind,c  d F_c / d eta_c / F_c,  c_k,c likewise,  c_refl,c = L_ind,c / R_c, with
//     cos = wi . normalize(wi + wo), the argument bsdf_sample handed to fresnel_conductor3 (wi.z for the delta lobe);
//   * the emitter sample (roughconductor only: a delta lobe evaluates to 0): the same three with Lr_dir in place of L_ind and
//     the half vector of wo = to_local(si, es.d); an occluded sample has Lr_dir = 0 and adds nothing.
// A coefficient is 0 where its denominator is 0 or it is not finite.  Nothing crosses channels.
// Plain C++, compiled by hipcc for gfx950 and by g++ for the host harness (tests/host_harness/trace_material_host.cpp).
#pragma once

#include "epsm_trace_replay.h"

namespace epsm {
namespace ma {

constexpr int kMaxSlots = EPSM_MAX_MATERIAL_GRADS;
constexpr int kPerSlot = 9;                       // [eta, k, specular_reflectance] x rgb
constexpr int kRow = kPerSlot * kMaxSlots;        // floats per row of partial sums
constexpr int kBlock = 128;                       // paths per row of partial sums (the device's workgroup)

struct MaterialArgs {
    TraceArgs A;
    const float *radiance;                        // (N,3) of the primal pass
    const float *adj;                             // backward: (N,3) d loss / d radiance
    float *d_radiance;                            // forward: (N,3) written
    const float *tangent;                         // forward: (n_slots,3,3) d [eta, k, specular_reflectance]
    float *partial;                               // backward: (ceil(N / kBlock), kRow) per-block sums, the workspace
    int n_slots;
};

struct Item { int slot; F3 c_eta, c_k, c_refl; };         // slot < 0: nothing

EPSM_HD float ratio_or_zero(float num, float den) { return den != 0.f ? finite_or_zero(num / den) : 0.f; }

// The three coefficients of a term `Lt` that carries the factor F(cos; eta_c, k_c) R_c in every channel.
EPSM_HD void material_coefs(const EpsmBsdf &b, float cos_i, F3 Lt, Item &it) {
    const float lt[3] = {Lt.x, Lt.y, Lt.z};
    float ce[3], ck[3], cr[3];
    for (int c = 0; c < 3; ++c) {
        float de, dk;
        const float F = fresnel_conductor_grad(cos_i, b.eta[c], b.k[c], &de, &dk);
        ce[c] = ratio_or_zero(lt[c] * de, F);
        ck[c] = ratio_or_zero(lt[c] * dk, F);
        cr[c] = ratio_or_zero(lt[c], b.reflectance[c]);
    }
    it.c_eta = f3(ce[0], ce[1], ce[2]); it.c_k = f3(ck[0], ck[1], ck[2]); it.c_refl = f3(cr[0], cr[1], cr[2]);
}

// What one bounce of a path contributes: `a` the sampled direction, `b` the emitter sample.  Shown the loop state before the
// bounce's update (epsm_trace_core.h, observe_state).
struct MaterialObserver {
    const MaterialArgs &T;
    bool has;                        // (lanes past N ride along on the device and observe nothing)
    F3 radiance;
    Item a, b;
    F3 L;

    EPSM_HD void state(const PathState &s) { L = s.L; }
    EPSM_HD void vertex(const SurfHit &si, const EpsmBsdf &bsdf, uint32_t, F3 Le, F3 Lr_dir, const EmitterSample &es, bool active_em,
                        float, const BsdfSample &bs, bool active) {
        a.slot = b.slot = -1;
        a.c_eta = a.c_k = a.c_refl = b.c_eta = b.c_k = b.c_refl = zero3<float>();
        if (!has || !active || !si.valid) return;
        const bool rough = bsdf.type == EPSM_BSDF_ROUGHCONDUCTOR_T;
        if (!(rough || bsdf.type == EPSM_BSDF_CONDUCTOR_T) || bsdf.material == 0 || bsdf.material > (uint32_t) T.n_slots) return;
        const int slot = (int) bsdf.material - 1;
        F3 wi = si.wi;
        const bool flipped = bsdf.twosided && wi.z < 0.f;
        if (flipped) wi.z = -wi.z;
        if (bs.valid) {
            F3 wo = bs.wo;
            if (flipped) wo.z = -wo.z;
            // (the order in which InlineVis::direct sums; at the path's last vertex a residue of an ulp of L, as in AlphaObserver)
            const F3 ind = radiance - (L + Le + Lr_dir);
            material_coefs(bsdf, rough ? dot(wi, normalize3(wi + wo)) : wi.z, ind, a);
            a.slot = slot;
        }
        if (rough && active_em && (Lr_dir.x != 0.f || Lr_dir.y != 0.f || Lr_dir.z != 0.f)) {   // (Lr_dir,c != 0 has f_c != 0)
            F3 wo = to_local(si, es.d);
            if (flipped) wo.z = -wo.z;
            material_coefs(bsdf, dot(wi, normalize3(wi + wo)), Lr_dir, b);
            b.slot = slot;
        }
    }
};

// The replay of path i (epsm_trace_replay.h) under a MaterialObserver.
template <class Sink>
EPSM_HD void material_replay(const MaterialArgs &T, int64_t i, bool has, PathState &s, const TriHit &th0, const BvhStack &st, Sink &sink) {
    MaterialObserver obs{T, has, has ? ld3(T.radiance + 3 * i) : zero3<float>()};
    obs.a.slot = obs.b.slot = -1;
    obs.a.c_eta = obs.a.c_k = obs.a.c_refl = obs.b.c_eta = obs.b.c_k = obs.b.c_refl = obs.L = zero3<float>();
    replay_path(T.A, i, has, s, th0, st, obs, sink);
}

// Backward, per path: sum over its items of adj_c coef_c, per slot, parameter and channel (the slot is matched, never used as
// an index).  acc[slot * 9 + 3 * parameter + channel].
struct MaterialSums {
    F3 adj;
    float acc[kRow];
    EPSM_HD void clear() { for (int k = 0; k < kRow; ++k) acc[k] = 0.f; }
    EPSM_HD void item(const Item &it) {
        const F3 e = mul3(adj, it.c_eta), k = mul3(adj, it.c_k), r = mul3(adj, it.c_refl);
        const float v[kPerSlot] = {e.x, e.y, e.z, k.x, k.y, k.z, r.x, r.y, r.z};
        for (int s = 0; s < kMaxSlots; ++s)
            for (int j = 0; j < kPerSlot; ++j) acc[s * kPerSlot + j] += it.slot == s ? v[j] : 0.f;
    }
};

// Forward: the path's radiance tangent, sum over its items of coef x tangent[slot] per channel (no atomics).
struct MaterialTangentSink {
    const MaterialArgs &T;
    int64_t i;
    bool has;
    F3 d;
    EPSM_HD void item(const Item &it) {
        if (it.slot < 0) return;
        const float *t = T.tangent + kPerSlot * it.slot;
        d = d + mul3(it.c_eta, ld3(t)) + mul3(it.c_k, ld3(t + 3)) + mul3(it.c_refl, ld3(t + 6));
    }
    EPSM_HD void finish() { if (has) st3(T.d_radiance, i, d); }
};

inline int64_t partial_rows(int64_t N) { return (N + kBlock - 1) / kBlock; }
inline size_t workspace_bytes(int64_t N) { return N > 0 ? (size_t) partial_rows(N) * kRow * sizeof(float) : 0; }

// The arguments of both entry points (host side; device and host builds alike): the common eight through replay_args_fill, then
// this pass's own.  NULL = fine, otherwise what is wrong; at N == 0 fine with nothing else looked at (T.A.N = 0: the caller has
// nothing to do).
inline const char *material_args_fill(MaterialArgs &T, const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp,
                                      int max_depth, int rr_depth, int64_t path_offset, int64_t N, const float *radiance, int M) {
    memset(&T, 0, sizeof(T));
    if (const char *why = replay_args_fill(T.A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 0)) return why;
    if (N == 0) return nullptr;
    if (!radiance) return "NULL radiance";
    if (M < 0) return "negative number of material slots";
    if (M > kMaxSlots) return "more than EPSM_MAX_MATERIAL_GRADS material slots";
    T.radiance = radiance;
    T.n_slots = M;
    return nullptr;
}

}  // namespace ma
}  // namespace epsm
