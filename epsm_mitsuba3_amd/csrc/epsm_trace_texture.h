// epsm_trace_texture.h -- per-path code of the texel adjoint (include/epsm_trace.h, epsm_trace_paths_texture_backward /
// epsm_trace_paths_texture_forward): d L / d texel of the `bitmap` reflectances of diffuse BSDFs and of the envmap's bitmap, and
// d L / d colour of the per-vertex reflectances (`mesh_attribute`, EPSM_TEXTURE_VERTEX_RGB: a footprint of three vertices).
//
// A path is replayed through path_bounce (epsm_trace_core.h) under the primal seed, as epsm_trace_paths_color traced it; an
// observer (TexObserver) turns each bounce into at most two ITEMS -- a footprint of up to four texels of one buffer, their
// interpolation weights and a per-channel coefficient -- and a sink either scatters adj x coef x weight into the texels
// (backward) or gathers sum(weight x tangent) x coef into the path's radiance tangent (forward): one is the other's transpose.
// PRB's rules (prb.py), sampling, Russian roulette and MIS detached:
//   * diffuse vertex k whose reflectance is a texture with a buffer: every term the path collects after its emission at k
//     (NEE at k and everything downstream) is linear in rho_k = tex_eval(uv_k) (vertex_attr_eval at a per-vertex table), channel by channel:
//     coef = L_after_k / rho_k, L_after_k = radiance - (L up to and including Le_k).  Where rho_k,c = 0 the coefficient is 0
//     (prb.py's inv_bsdf_val_det select): the terms through k are 0 in that channel and their derivative is not recovered.
//   * a ray that leaves the scene: Le = beta env(d) mis, coef = beta mis.
//   * an emitter sample on the envmap: Lr_dir = beta bsdf(wo) env(d) / pdf mis_em, coef = beta bsdf(wo) mis_em / pdf, zero
//     when the sample is occluded (the sampling tables are detached: envmap.cpp builds its warp from detached data).
// Plain C++, compiled by hipcc for gfx950 and by g++ for the host harness (tests/host_harness/trace_tex_host.cpp).
#pragma once

#include "epsm_trace_replay.h"

namespace epsm {
namespace tx {

constexpr int kMaxBufs = EPSM_MAX_TEXTURE_GRADS;
constexpr int kEnvBuf = kMaxBufs;                 // buffer index of the envmap's (H, W, 3) gradient / tangent

struct TexArgs {
    TraceArgs A;
    const float *radiance;                        // (N,3) of the primal pass
    const float *adj;                             // backward: (N,3) d loss / d radiance; forward: unused
    float *d_radiance;                            // forward: (N,3) written; backward: unused
    int n_buf;                                    // texture buffers in use, <= kMaxBufs
    int32_t tex[kMaxBufs];                        // buffer b belongs to EpsmScene.textures[tex[b]]
    float *buf[kMaxBufs + 1];                     // (H_t, W_t, 3) per buffer; [kEnvBuf]: the envmap's (H, W, 3) or NULL
};

// A footprint: four texels of buffer b (nearest: one, weights 0 for the others) -- element offsets (row * width + column) into
// the buffer -- their weights, and the coefficient of the term per channel.  (b, i0, j0) names the footprint within a wave.
struct Item {
    bool on;
    uint32_t b, i0, j0;
    uint32_t off[4];
    float w[4];
    F3 coef;
};
EPSM_HD void item_clear(Item &it) {
    it.on = false; it.b = it.i0 = it.j0 = 0u;
    for (int k = 0; k < 4; ++k) { it.off[k] = 0u; it.w[k] = 0.f; }
    it.coef = zero3<float>();
}

// the texels tex_eval interpolates at (u, v), same wrap.  A per-vertex table has no such footprint (vertex_footprint): it is read
// as a 1 x 1 bitmap with zero weights, none of its words taken for a size.
EPSM_HD void texture_footprint(const EpsmTexture &T, float u, float v, Item &it) {
    const bool bitmap = !tex_is_vertex(T);
    const int W = bitmap ? T.width : 1, H = bitmap ? T.height : 1;
    const float x = u * (float) W - 0.5f, y = v * (float) H - 0.5f;
    if (T.nearest) {
        const int i = tex_wrap((int) floorf(x + 0.5f), W), j = tex_wrap((int) floorf(y + 0.5f), H);
        it.i0 = (uint32_t) i; it.j0 = (uint32_t) j;
        it.off[0] = it.off[1] = it.off[2] = it.off[3] = (uint32_t) (j * W + i);
        it.w[0] = bitmap ? 1.f : 0.f; it.w[1] = it.w[2] = it.w[3] = 0.f;
        return;
    }
    const float fxf = floorf(x), fyf = floorf(y);
    const int i0 = tex_wrap((int) fxf, W), j0 = tex_wrap((int) fyf, H), i1 = tex_wrap((int) fxf + 1, W), j1 = tex_wrap((int) fyf + 1, H);
    const float fx = x - fxf, fy = y - fyf, on = bitmap ? 1.f : 0.f;
    it.i0 = (uint32_t) i0; it.j0 = (uint32_t) j0;
    it.off[0] = (uint32_t) (j0 * W + i0); it.off[1] = (uint32_t) (j0 * W + i1);
    it.off[2] = (uint32_t) (j1 * W + i0); it.off[3] = (uint32_t) (j1 * W + i1);
    it.w[0] = (1.f - fx) * (1.f - fy) * on; it.w[1] = fx * (1.f - fy) * on; it.w[2] = (1.f - fx) * fy * on; it.w[3] = fx * fy * on;
}
// the three rows vertex_attr_eval interpolates at a hit, their weights its barycentrics; the fourth entry repeats the third with
// weight 0.  The footprint's name is the TRIANGLE (i0 = triangle id, j0 = 0): lanes in two triangles may share a vertex, never a
// footprint, and lanes merged under one name add under the last lane's rows.  False where a vertex lies outside the table.
EPSM_HD bool vertex_footprint(const EpsmTexture &T, const SurfHit &si, Item &it) {
    uint32_t r0, r1, r2;
    if (!vertex_attr_rows(T, si, r0, r1, r2)) return false;
    it.i0 = si.tri; it.j0 = 0u;
    it.off[0] = r0; it.off[1] = r1; it.off[2] = r2; it.off[3] = r2;
    it.w[0] = si.b0; it.w[1] = si.b1; it.w[2] = si.b2; it.w[3] = 0.f;
    return true;
}
// the texels env_eval interpolates along the world direction d; column W of EpsmEnvironment.texels is column 0 of the bitmap
EPSM_HD void env_footprint(const EpsmEnvironment &E, F3 d, Item &it) {
    float x, y;
    env_cell_coords(E, env_to_local(E, d), x, y);
    int i = (int) x, j = (int) fminf(y, (float) (E.height - 2));
    const float fx = x - (float) i, fy = y - (float) j;
    // (these index the buffer the adds go to: kept inside it whatever a degenerate direction makes of x, y)
    i = i < 0 ? 0 : (i >= E.width ? E.width - 1 : i); j = j < 0 ? 0 : (j > E.height - 2 ? E.height - 2 : j);
    const int i1 = i + 1 < E.width ? i + 1 : 0;
    it.i0 = (uint32_t) i; it.j0 = (uint32_t) j;
    it.off[0] = (uint32_t) (j * E.width + i); it.off[1] = (uint32_t) (j * E.width + i1);
    it.off[2] = (uint32_t) ((j + 1) * E.width + i); it.off[3] = (uint32_t) ((j + 1) * E.width + i1);
    it.w[0] = (1.f - fx) * (1.f - fy); it.w[1] = fx * (1.f - fy); it.w[2] = (1.f - fx) * fy; it.w[3] = fx * fy;
}

// What one bounce of a path contributes: `a` the textured vertex or the escaped ray (never both), `b` the emitter sample on the
// envmap.  Shown the loop state before the bounce's update (epsm_trace_core.h, observe_state).
struct TexObserver {
    const TexArgs &T;
    const BvhStack &st;
    bool has;                        // (lanes past N ride along on the device and observe nothing)
    F3 radiance;
    Item a, b;
    F3 L, beta, dir;
    float prev_bsdf_pdf;
    bool prev_bsdf_delta;

    EPSM_HD void state(const PathState &s) {
        L = s.L; beta = s.beta; dir = s.ray.d; prev_bsdf_pdf = s.prev_bsdf_pdf; prev_bsdf_delta = s.prev_bsdf_delta;
    }
    EPSM_HD int buffer_of(int32_t texture) const {
        for (int k = 0; k < kMaxBufs; ++k)
            if (k < T.n_buf && T.tex[k] == texture && T.buf[k]) return k;
        return -1;
    }
    EPSM_HD void vertex(const SurfHit &si, const EpsmBsdf &bsdf, uint32_t, F3 Le, F3 Lr_dir, const EmitterSample &es, bool active_em,
                        float mis_em, const BsdfSample &, bool active) {
        item_clear(a); item_clear(b);
        if (!has || !active) return;                                          // (an inactive vertex collects nothing)
        const EpsmScene &S = T.A.S;
        const bool env_on = S.env.kind == EPSM_ENV_ENVMAP && T.buf[kEnvBuf] != nullptr;
        if (si.valid) {
            // (a 1-channel texture is a roughness map: its buffer is (H, W) and belongs to epsm_trace_alphamap.h)
            const int k = bsdf.type == EPSM_BSDF_DIFFUSE_T && bsdf.texture >= 0 && bsdf.texture < S.n_textures &&
                          S.textures[bsdf.texture].channels != 1 ? buffer_of(bsdf.texture) : -1;
            if (k >= 0) {
                const F3 rho = ld3(bsdf.reflectance);                          // tex_eval(uv) (path_bounce)
                const F3 after = radiance - (L + Le);                           // (the order in which InlineVis::direct sums)
                a.coef = finite_or_zero3(f3(rho.x != 0.f ? after.x / rho.x : 0.f, rho.y != 0.f ? after.y / rho.y : 0.f,
                                            rho.z != 0.f ? after.z / rho.z : 0.f));
                const EpsmTexture &tex = S.textures[bsdf.texture];
                a.b = (uint32_t) k; a.on = true;
                // (a per-vertex table with a vertex outside it: path_bounce ignored the lookup, rho is not the table's)
                if (tex_is_vertex(tex)) a.on = vertex_footprint(tex, si, a);
                else texture_footprint(tex, si.uvx, si.uvy, a);
            }
        } else if (env_on) {                                                   // the ray left the scene (path_bounce's Le)
            float em_pdf = prev_bsdf_delta ? 0.f : env_pdf(S, dir);
            if (S.n_emitters > 1) em_pdf /= (float) S.n_emitters;
            a.coef = finite_or_zero3(beta * mis_weight(prev_bsdf_pdf, em_pdf));
            env_footprint(S.env, dir, a);
            a.b = (uint32_t) kEnvBuf; a.on = true;
        }
        if (env_on && active_em && es.emitter == S.env.emitter && es.pdf != 0.f) {
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
                if (visible) {
                    b.coef = finite_or_zero3(c);
                    env_footprint(S.env, es.d, b);
                    b.b = (uint32_t) kEnvBuf; b.on = true;
                }
            }
        }
    }
};

// The replay of path i (epsm_trace_replay.h) under a TexObserver.
template <class Sink>
EPSM_HD void texture_replay(const TexArgs &T, int64_t i, bool has, PathState &s, const TriHit &th0, const BvhStack &st, Sink &sink) {
    TexObserver obs{T, st, has, has ? ld3(T.radiance + 3 * i) : zero3<float>()};
    item_clear(obs.a); item_clear(obs.b);
    obs.L = obs.beta = obs.dir = zero3<float>(); obs.prev_bsdf_pdf = 1.f; obs.prev_bsdf_delta = true;
    replay_path(T.A, i, has, s, th0, st, obs, sink);
}

// The arguments of both entry points (host side; device and host builds alike): the common eight through replay_args_fill, then
// this pass's own.  NULL = fine, otherwise what is wrong; at N == 0 fine with nothing else looked at (T.A.N = 0: the caller has
// nothing to do).  `bufs` holds n_textures pointers (or is NULL), `env` the envmap's; both entry points' buffers go into T.buf.
inline const char *tex_args_fill(TexArgs &T, const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                 int rr_depth, int64_t path_offset, int64_t N, const float *radiance, float *const *bufs, float *env) {
    memset(&T, 0, sizeof(T));
    if (const char *why = replay_args_fill(T.A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 0)) return why;
    if (N == 0) return nullptr;
    if (!radiance) return "NULL radiance";
    if (env && scene->env.kind != EPSM_ENV_ENVMAP) return "an envmap buffer for a scene without an envmap";
    T.radiance = radiance;
    if (bufs)
        for (int t = 0; t < scene->n_textures; ++t) {
            if (!bufs[t]) continue;
            if (T.n_buf >= kMaxBufs) return "more than EPSM_MAX_TEXTURE_GRADS texture buffers";
            T.tex[T.n_buf] = t; T.buf[T.n_buf] = bufs[t]; ++T.n_buf;
        }
    T.buf[kEnvBuf] = env;
    return nullptr;
}

// Forward: the path's radiance tangent, sum over its items of coef x sum_k w_k tangent[texel k] (no atomics).
struct GatherSink {
    const TexArgs &T;
    int64_t i;
    bool has;
    F3 d;
    EPSM_HD void item(const Item &it) {
        if (!it.on) return;
        const float *t = T.buf[it.b];
        F3 g = zero3<float>();
        for (int k = 0; k < 4; ++k)
            if (it.w[k] != 0.f) g = g + ld3(t + 3 * (int64_t) it.off[k]) * it.w[k];
        d = d + mul3(it.coef, g);
    }
    EPSM_HD void finish() { if (has) st3(T.d_radiance, i, d); }
};

}  // namespace tx
}  // namespace epsm
