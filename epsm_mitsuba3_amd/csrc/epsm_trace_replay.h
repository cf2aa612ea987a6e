// epsm_trace_replay.h -- the frame the tracer's derivative passes share ("the replay frame"): the check of the
// arguments every replay entry point of include/epsm_trace.h starts with, and the loop that replays a path through path_bounce
// under the primal seed, shows every bounce to an OBSERVER and hands what the observer made of it to a SINK.
// Plain C++, compiled by hipcc for gfx950 and by g++ for the host harness (tests/host_harness).
#pragma once

#include <string.h>

#include "epsm_trace_core.h"

#if defined(__HIPCC__)
#include "epsm_common.h"
#else
// (epsm_common.h brings the HIP runtime with it, which the host harness is built without: its table check, word for word)
namespace epsm_host {
inline const char *scene_tables_invalid(const EpsmScene *s) {
    if (s->n_emitters < 0 || (s->n_emitters > 0 && !s->emitters)) return "NULL emitters";
    const EpsmEnvironment &e = s->env;
    if (e.kind != EPSM_ENV_NONE && e.kind != EPSM_ENV_CONSTANT && e.kind != EPSM_ENV_ENVMAP) return "env.kind is not an EPSM_ENV_* value";
    if (e.kind != EPSM_ENV_NONE && (e.emitter < 0 || e.emitter >= s->n_emitters)) return "env.emitter is not an index into emitters";
    if (e.kind == EPSM_ENV_ENVMAP && (!e.texels || !e.row_cdf || !e.col_cdf || !e.cell_pdf || e.width < 2 || e.height < 2))
        return "envmap environment needs texels, row_cdf, col_cdf, cell_pdf and width, height >= 2";
    if (s->n_textures < 0 || (s->n_textures > 0 && !s->textures)) return "NULL textures";
    return nullptr;
}
}  // namespace epsm_host
#endif

namespace epsm {

// The arguments every entry point that traces or replays a tile of paths starts with: NULL = fine and A filled (zeroed first;
// K_log 0, no outputs), otherwise what is wrong.  `min_depth`: the smallest max_depth the pass accepts (the tracer 1, the texel
// and roughness replays 0: a path of no bounce has no item).  N == 0 is fine whatever else is passed beside scene and sensor:
// the caller returns EPSM_OK before it looks at its own arguments.
inline const char *replay_args_fill(TraceArgs &A, const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                    int rr_depth, int64_t path_offset, int64_t N, int min_depth) {
    memset(&A, 0, sizeof(A));
    if (!scene || !sensor) return "NULL scene / sensor";
    if (N == 0) return nullptr;
    if (N < 0 || spp < 1 || max_depth < min_depth || rr_depth < 1 || path_offset < 0)
        return "bad N / spp / max_depth / rr_depth / path_offset";
    if (sensor->border < 0 || sensor->border > 8) return "bad sensor border";
    if (path_offset + N > (int64_t) (sensor->width + 2 * sensor->border) * (sensor->height + 2 * sensor->border) * spp ||
        path_offset + N > 0xFFFFFFFFLL)
        return "path range exceeds (width + 2 border) * (height + 2 border) * spp (or 2^32, common.py:468-475)";
    if (scene->n_triangles > 0 && (!scene->positions || !scene->normals || !scene->tri || !scene->tri_mesh ||
                                   !scene->meshes || !scene->bsdfs || !scene->bvh || !scene->prim_index || !scene->tri_verts))
        return "NULL scene array";
    if (const char *why = epsm_host::scene_tables_invalid(scene)) return why;
    A.S = *scene; A.C = *sensor;
    A.seed = seed; A.spp = spp; A.max_depth = max_depth; A.rr_depth = rr_depth;
    A.path_offset = path_offset; A.N = N;
    return nullptr;
}

// The arguments of the tracer's own entry points (epsm_trace_paths, _color, _wavefront), device library and host twin alike:
// replay_args_fill, then the log, the outputs and the flags.  NULL = fine and A filled, otherwise what is wrong.
inline const char *trace_args_fill(TraceArgs &A, const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                   int rr_depth, int64_t path_offset, int64_t N, int K_log, float *ray_o, float *ray_d, float *ray_dx,
                                   float *ray_dy, float *film_pos, float *radiance, uint8_t *valid, const EpsmRecordOut *recs,
                                   uint32_t flags) {
    if (const char *why = replay_args_fill(A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 1)) return why;
    if (K_log < 0 || K_log > EPSM_MAX_VERTICES || K_log > (max_depth < 6 ? max_depth : 6))
        return "K_log must be <= min(max_depth, 5)";
    const bool packed = (flags & EPSM_TRACE_PACKED_LOG) != 0;
    if (!ray_o || (!packed && (!ray_d || !ray_dx || !ray_dy)) || (K_log > 0 && !recs)) return "NULL output";
    if (packed && ((((uintptr_t) ray_o) & 15) || (K_log > 0 && (!recs[0].packed || !recs[0].pflags || (((uintptr_t) recs[0].packed) & 15)))))
        return "EPSM_TRACE_PACKED_LOG needs 16-byte aligned ray_o (N,12), recs[0].packed and recs[0].pflags";
    if (packed && K_log > 0) {
        const int64_t rs = recs[0].ray_stride, ps = recs[0].packed_stride;
        if (rs < 0 || ps < 0 || (rs & 3) || (ps & 3) || (rs && rs < 12) || (ps && ps < (int64_t) K_log * 32))
            return "EpsmRecordOut.ray_stride / packed_stride must be 0 or multiples of 4 words >= 12 / 32 K_log";
    }
    if (flags & ~(uint32_t) (EPSM_TRACE_SPARSE_LOG | EPSM_TRACE_PACKED_LOG | EPSM_TRACE_GRADIENT_ONLY | EPSM_TRACE_GRADIENT_CAUSTIC | EPSM_TRACE_NO_TAIL |
                             EPSM_TRACE_FUSE_FIRST_HIT))
        return "unknown flag";
    if (flags & EPSM_TRACE_FUSE_FIRST_HIT) {
        if (!(flags & EPSM_TRACE_GRADIENT_ONLY) || !packed || K_log < 1) return "EPSM_TRACE_FUSE_FIRST_HIT needs EPSM_TRACE_GRADIENT_ONLY and EPSM_TRACE_PACKED_LOG";
        const EpsmFirstHitBackward *f = recs[0].first_hit;
        if (!f || !f->grad_img || !f->grad_pos || (f->T > 0 && !f->tri_table) || f->T < 0 || f->V < 0 || f->res < 1 || f->img_width < f->res ||
            f->img_channels < 5 || (((uintptr_t) f->tri_table) & 15))
            return "EPSM_TRACE_FUSE_FIRST_HIT: recs[0].first_hit needs grad_img (>= 5 channels, img_width >= res >= 1), grad_pos and a 16-byte aligned tri_table";
        if (path_offset + N > (int64_t) f->res * f->res * spp) return "EPSM_TRACE_FUSE_FIRST_HIT: path range exceeds res * res * spp";
        if (recs[0].shadow && max_depth <= 3) return "EPSM_TRACE_FUSE_FIRST_HIT: not with the occluder record (max_depth <= 3)";
        if ((f->survivors != nullptr) != (f->survivor_count != nullptr)) return "EPSM_TRACE_FUSE_FIRST_HIT: survivors and survivor_count come together";
    }
    if ((flags & EPSM_TRACE_GRADIENT_CAUSTIC) && !(flags & EPSM_TRACE_GRADIENT_ONLY)) return "EPSM_TRACE_GRADIENT_CAUSTIC modifies EPSM_TRACE_GRADIENT_ONLY";
    if ((flags & EPSM_TRACE_GRADIENT_ONLY) && K_log < 1) return "EPSM_TRACE_GRADIENT_ONLY needs a vertex log (K_log >= 1)";
    A.flags = flags; A.K_log = K_log;
    A.ray_o = ray_o; A.ray_d = ray_d; A.ray_dx = ray_dx; A.ray_dy = ray_dy;
    A.film_pos = film_pos; A.radiance = radiance; A.valid = valid;
    for (int k = 0; k < K_log; ++k) {
        const EpsmRecordOut &r = recs[k];
        if (packed) { A.rec[k] = r; continue; }
        if (!r.p0 || !r.p1 || !r.p2 || !r.n0 || !r.n1 || !r.n2 || !r.b0 || !r.b1 || !r.eta || !r.hf || !r.light ||
            !r.bsdf || !r.active || !r.active_em || !r.ismesh || !r.tri || !r.aux || !r.emit)
            return "NULL pointer in a record (p / normal may be NULL)";
        A.rec[k] = r;
    }
    trace_args_log_strides(A);
    if (flags & EPSM_TRACE_FUSE_FIRST_HIT) A.fh = *recs[0].first_hit;
    return nullptr;
}

EPSM_HD float finite_or_zero(float x) { return fabsf(x) < __builtin_inff() ? x : 0.f; }   // (a non-finite coefficient adds nothing)
EPSM_HD F3 finite_or_zero3(F3 v) { return f3(finite_or_zero(v.x), finite_or_zero(v.y), finite_or_zero(v.z)); }

// The replay of path i after its primary ray's closest hit th0 (the device walks those as a packet, the host one by one).  The
// observer is shown every bounce (epsm_trace_core.h: obs.vertex, and obs.state where it declares one) and leaves two items, obs.a
// and obs.b; sink.item(it) after every bounce for both (on or not: a device sink may work across the wave), sink.finish() at the
// end.  `has`: lanes past N ride along on the device without a path; their observer sees nothing.
template <class Obs, class Sink>
EPSM_HD void replay_path(const TraceArgs &A, int64_t i, bool has, PathState &s, const TriHit &th0, const BvhStack &st, Obs &obs,
                         Sink &sink) {
    InlineVis vis{st};
    if (!has) s.active = false;
    const int max_depth = path_max_depth(A);
    for (int iteration = 0; iteration < max_depth; ++iteration) {
        TriHit th; th.hit = false; th.tri = 0; th.t = kInf; th.u = th.v = 0.f;
        if (iteration == 0) th = th0;
        else if (s.active) th = intersect<false>(A.S, s.ray, st);
        path_bounce(A, i, iteration, s, th, vis, obs);
        sink.item(obs.a);
        sink.item(obs.b);
    }
    sink.finish();
}

}  // namespace epsm
