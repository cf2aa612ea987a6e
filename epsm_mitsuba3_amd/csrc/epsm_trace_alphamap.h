// epsm_trace_alphamap.h -- per-path code of the roughness-map adjoint (include/epsm_trace.h,
// epsm_trace_paths_alpha_texture_backward / epsm_trace_paths_alpha_texture_forward): d L / d texel of the 1-channel `bitmap` the
// alpha of a `roughconductor` is (EpsmBsdf.texture on a roughconductor, EpsmTexture.channels = 1).
//
// A path is replayed through path_bounce (epsm_trace_core.h) under the primal seed, as epsm_trace_paths_color traced it; an
// observer (AlphaMapObserver) turns each bounce into at most ONE item -- the footprint of the lookup that gave the vertex its
// alpha (texture_footprint, epsm_trace_texture.h) and a per-channel coefficient -- and a sink either scatters
// adj . coef x weight into the texels (backward) or gathers coef x sum(weight x tangent) into the path's radiance tangent
// (forward): one is the other's transpose.  The coefficient is AlphaObserver's (epsm_trace_bsdf.h), sampling, Russian roulette
// and the MIS weights detached: at an active bounce whose vertex carries such a BSDF, alpha = tex_eval_1(uv) (path_bounce),
//   * indirect term: coef_c = L_ind,c  f_c  d ln f / d alpha / (weight_c pdf), L_ind = radiance - (L + Le + Lr_dir), zero where
//     weight_c pdf = 0 or the term is not finite;
//   * emitter sample: coef_c = Lr_dir,c  d ln f(wo_em) / d alpha; an occluded sample has Lr_dir = 0 and adds nothing.
// Both terms are derivatives w.r.t. the same alpha, i.e. sit on the same footprint: the item carries their sum.
// Plain C++, compiled by hipcc for gfx950 and by g++ for the host harness (tests/host_harness/trace_alphamap_host.cpp).
#pragma once

#include "epsm_trace_texture.h"

namespace epsm {
namespace am {

constexpr int kMaxBufs = EPSM_MAX_TEXTURE_GRADS;

struct AlphaMapArgs {
    TraceArgs A;
    const float *radiance;                        // (N,3) of the primal pass
    const float *adj;                             // backward: (N,3) d loss / d radiance; forward: unused
    float *d_radiance;                            // forward: (N,3) written; backward: unused
    int n_buf;                                    // texture buffers in use, <= kMaxBufs
    int32_t tex[kMaxBufs];                        // buffer b belongs to EpsmScene.textures[tex[b]]
    float *buf[kMaxBufs];                         // (H_t, W_t) per buffer
};

struct NoItem {};                                 // (the replay frame hands a sink two items per bounce: this pass has one)

// What one bounce of a path contributes: `a`, a tx::Item whose `b` is the buffer; `b` never anything.  Shown the loop state
// before the bounce's update (epsm_trace_core.h, observe_state).
struct AlphaMapObserver {
    const AlphaMapArgs &T;
    bool has;                        // (lanes past N ride along on the device and observe nothing)
    F3 radiance;
    tx::Item a;
    NoItem b;
    F3 L;

    EPSM_HD void state(const PathState &s) { L = s.L; }
    EPSM_HD int buffer_of(int32_t texture) const {
        for (int k = 0; k < kMaxBufs; ++k)
            if (k < T.n_buf && T.tex[k] == texture && T.buf[k]) return k;
        return -1;
    }
    EPSM_HD void vertex(const SurfHit &si, const EpsmBsdf &bsdf, uint32_t, F3 Le, F3 Lr_dir, const EmitterSample &es, bool active_em,
                        float, const BsdfSample &bs, bool active) {
        tx::item_clear(a);
        if (!has || !active || !si.valid) return;
        const EpsmScene &S = T.A.S;
        if (bsdf.type != EPSM_BSDF_ROUGHCONDUCTOR_T || bsdf.texture < 0 || bsdf.texture >= S.n_textures) return;
        if (S.textures[bsdf.texture].channels != 1) return;                    // (path_bounce ignored it too: bsdf.alpha is the table's)
        const int k = buffer_of(bsdf.texture);
        if (k < 0) return;
        F3 coef = zero3<float>();
        if (bs.valid) {
            F3 f; float pdf;
            bsdf_eval_pdf(bsdf, si.wi, bs.wo, f, pdf);
            const float dl = rough_dlog_dalpha(bsdf, si.wi, bs.wo);
            const F3 ind = radiance - (L + Le + Lr_dir);                       // (the order in which InlineVis::direct sums; AlphaObserver)
            const F3 den = bs.weight * bs.pdf;
            coef = finite_or_zero3(f3(den.x != 0.f ? ind.x * f.x * dl / den.x : 0.f, den.y != 0.f ? ind.y * f.y * dl / den.y : 0.f,
                                      den.z != 0.f ? ind.z * f.z * dl / den.z : 0.f));
        }
        if (active_em && (Lr_dir.x != 0.f || Lr_dir.y != 0.f || Lr_dir.z != 0.f))   // (Lr_dir,c != 0 has f_c != 0)
            coef = coef + finite_or_zero3(Lr_dir * rough_dlog_dalpha(bsdf, si.wi, to_local(si, es.d)));
        a.coef = coef;
        tx::texture_footprint(S.textures[bsdf.texture], si.uvx, si.uvy, a);
        a.b = (uint32_t) k; a.on = true;
    }
};

// The replay of path i (epsm_trace_replay.h) under an AlphaMapObserver.
template <class Sink>
EPSM_HD void alphamap_replay(const AlphaMapArgs &T, int64_t i, bool has, PathState &s, const TriHit &th0, const BvhStack &st, Sink &sink) {
    AlphaMapObserver obs{T, has, has ? ld3(T.radiance + 3 * i) : zero3<float>()};
    tx::item_clear(obs.a);
    obs.L = zero3<float>();
    replay_path(T.A, i, has, s, th0, st, obs, sink);
}

// The arguments of both entry points (host side; device and host builds alike): the common eight through replay_args_fill, then
// this pass's own.  NULL = fine, otherwise what is wrong; at N == 0 fine with nothing else looked at (T.A.N = 0: the caller has
// nothing to do).  `bufs` holds n_textures pointers (or is NULL); both entry points' buffers go into T.buf.
inline const char *alphamap_args_fill(AlphaMapArgs &T, const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp,
                                      int max_depth, int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                      float *const *bufs) {
    memset(&T, 0, sizeof(T));
    if (const char *why = replay_args_fill(T.A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 0)) return why;
    if (N == 0) return nullptr;
    if (!radiance) return "NULL radiance";
    T.radiance = radiance;
    if (bufs)
        for (int t = 0; t < scene->n_textures; ++t) {
            if (!bufs[t]) continue;
            if (T.n_buf >= kMaxBufs) return "more than EPSM_MAX_TEXTURE_GRADS texture buffers";
            T.tex[T.n_buf] = t; T.buf[T.n_buf] = bufs[t]; ++T.n_buf;
        }
    return nullptr;
}

// Forward: the path's radiance tangent, sum over its items of coef x sum_k w_k tangent[texel k] (no atomics).
struct GatherSink {
    const AlphaMapArgs &T;
    int64_t i;
    bool has;
    F3 d;
    EPSM_HD void item(const tx::Item &it) {
        if (!it.on) return;
        const float *t = T.buf[it.b];
        float g = 0.f;
        for (int k = 0; k < 4; ++k)
            if (it.w[k] != 0.f) g += t[it.off[k]] * it.w[k];
        d = d + it.coef * g;
    }
    EPSM_HD void item(const NoItem &) {}
    EPSM_HD void finish() { if (has) st3(T.d_radiance, i, d); }
};

}  // namespace am
}  // namespace epsm
