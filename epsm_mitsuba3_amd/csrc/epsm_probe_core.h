// epsm_probe_core.h -- one row of epsm_probe (include/epsm_trace.h): evaluates ONE of the tracer's per-path functions on
// plain numbers, so that the known answers the reference's own tests hold for them (tests/golden/reference_vectors.py)
// can be checked against the very code the tracer runs -- on the device through the product library, on the host through
// tests/host_harness/trace_host.cpp.  Rows are EPSM_PROBE_IN floats in, EPSM_PROBE_OUT floats out; integers travel as bits.
#pragma once

#include "epsm_trace_core.h"
#include "epsm_trace_reparam.h"      // the dual-number restatements of the BSDF values (rp::bsdf_eval_t, rp::fresnel_conductor_t)

namespace epsm {


EPSM_HD void probe_row(int what, const float *in, float *out, const EpsmBsdf *bsdf, const EpsmSensor *sensor) {
    for (int j = 0; j < EPSM_PROBE_OUT; ++j) out[j] = 0.f;
    switch (what) {
        case EPSM_PROBE_TEA: {                         // in: v0, v1 (bits) -> out: v0', v1' (bits)
            uint32_t o0, o1;
            sample_tea_32(f2u(in[0]), f2u(in[1]), o0, o1);
            out[0] = u2f(o0); out[1] = u2f(o1);
        } break;
        case EPSM_PROBE_PCG32: {                       // in: initstate lo, hi, initseq lo, hi (bits)
            Pcg32 r = pcg32_seed((uint64_t) f2u(in[0]) | ((uint64_t) f2u(in[1]) << 32),
                                 (uint64_t) f2u(in[2]) | ((uint64_t) f2u(in[3]) << 32));
            for (int j = 0; j < 6; ++j) out[j] = u2f(r.next_u32());       // six draws as bits
            for (int j = 6; j < 12; ++j) out[j] = r.next_1d();            // the next six as next_1d()
        } break;
        case EPSM_PROBE_SAMPLER: {                     // in: seed, wavefront index (bits): the tracer's per-path stream
            Pcg32 r = seed_sampler(f2u(in[0]), f2u(in[1]));
            for (int j = 0; j < 12; ++j) out[j] = r.next_1d();
        } break;
        case EPSM_PROBE_MICROFACET: {                  // in: m (3), wi (3) -> D(m), pdf(wi, m), G1(m; wi)
            const F3 m = f3(in[0], in[1], in[2]), wi = f3(in[3], in[4], in[5]);
            out[0] = mf_eval(*bsdf, m); out[1] = mf_pdf(*bsdf, wi, m); out[2] = mf_smith_g1(*bsdf, m, wi);
        } break;
        case EPSM_PROBE_MICROFACET_SAMPLE: {           // in: u1, u2 -> m (3), pdf, d m / d alpha (3)
            float pdf; F3 dm;
            const F3 m = mf_sample(*bsdf, in[0], in[1], pdf, dm);
            out[0] = m.x; out[1] = m.y; out[2] = m.z; out[3] = pdf; out[4] = dm.x; out[5] = dm.y; out[6] = dm.z;
        } break;
        case EPSM_PROBE_FRESNEL: {                     // in: cos_theta_i, eta -> F, cos_theta_t, eta_it, eta_ti
            fresnel(in[0], in[1], out[0], out[1], out[2], out[3]);
        } break;
        case EPSM_PROBE_FRESNEL_CONDUCTOR: {           // in: cos_theta_i, eta, k -> F
            out[0] = fresnel_conductor(in[0], in[1], in[2]);
        } break;
        case EPSM_PROBE_RFILTER: {                     // in: x -> gaussian(x)
            out[0] = gaussian_rfilter(in[0]);
        } break;
        case EPSM_PROBE_PRIMARY_RAY: {                 // in: film position (pixels) -> o, d, d_x, d_y
            const PrimaryRay p = primary_ray_at(*sensor, in[0], in[1]);
            out[0] = p.ray.o.x; out[1] = p.ray.o.y; out[2] = p.ray.o.z; out[3] = p.ray.d.x; out[4] = p.ray.d.y; out[5] = p.ray.d.z;
            out[6] = p.dx.x; out[7] = p.dx.y; out[8] = p.dx.z; out[9] = p.dy.x; out[10] = p.dy.y; out[11] = p.dy.z;
        } break;
        case EPSM_PROBE_BSDF_SAMPLE: {                 // in: wi (3), sample1, sample2 (2) -> wo, weight, pdf, eta, sampled_type, valid
            const BsdfSample b = bsdf_sample(*bsdf, f3(in[0], in[1], in[2]), in[3], in[4], in[5], true);
            out[0] = b.wo.x; out[1] = b.wo.y; out[2] = b.wo.z; out[3] = b.weight.x; out[4] = b.weight.y; out[5] = b.weight.z;
            out[6] = b.pdf; out[7] = b.eta; out[8] = u2f(b.sampled_type); out[9] = b.valid ? 1.f : 0.f;
        } break;
        case EPSM_PROBE_BSDF_EVAL: {                   // in: wi (3), wo (3) -> value incl. the cosine (3), pdf
            F3 v; float pdf;
            bsdf_eval_pdf(*bsdf, f3(in[0], in[1], in[2]), f3(in[3], in[4], in[5]), v, pdf);
            out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = pdf;
        } break;
        case EPSM_PROBE_MICROFACET_DALPHA: {           // in: m (3), v (3) -> d ln D(m) / d alpha, d ln G1(v, m) / d alpha, D(m), G1(v, m)
            const F3 m = f3(in[0], in[1], in[2]), v = f3(in[3], in[4], in[5]);
            out[0] = mf_eval_dlog_dalpha(*bsdf, m); out[1] = mf_smith_g1_dlog_dalpha(*bsdf, v, m);
            out[2] = mf_eval(*bsdf, m); out[3] = mf_smith_g1(*bsdf, v, m);
        } break;
        case EPSM_PROBE_BSDF_DALPHA: {                 // in: wi (3), wo (3) -> d value / d alpha (3), d ln value / d alpha
            F3 v; float pdf;
            const F3 wi = f3(in[0], in[1], in[2]), wo = f3(in[3], in[4], in[5]);
            bsdf_eval_pdf(*bsdf, wi, wo, v, pdf);
            const float dl = bsdf->type == EPSM_BSDF_ROUGHCONDUCTOR_T ? rough_dlog_dalpha(*bsdf, wi, wo) : 0.f;
            out[0] = v.x * dl; out[1] = v.y * dl; out[2] = v.z * dl; out[3] = dl;
        } break;
        case EPSM_PROBE_FRESNEL_CONDUCTOR_GRAD: {      // in: cos_theta_i, eta, k -> F, d F / d eta, d F / d k
            out[0] = fresnel_conductor_grad(in[0], in[1], in[2], &out[1], &out[2]);
        } break;
        case EPSM_PROBE_REPARAM_BSDF: {                // in: wi (3), wo (3), which of them carries the seeds (0: wi, else wo) ->
            // rp::bsdf_eval_t<float> (3), the value of rp::bsdf_eval_t<rp::Dual> (3), d value_c / d seeded_k (3 x 3, row c)
            const F3 wi = f3(in[0], in[1], in[2]), wo = f3(in[3], in[4], in[5]);
            const bool seed_wo = in[6] != 0.f;
            const F3 v = rp::bsdf_eval_t<float>(*bsdf, wi, wo);
            const V3<rp::Dual> d = rp::bsdf_eval_t<rp::Dual>(*bsdf, rp::seed3<rp::Dual>(wi, seed_wo ? -1 : 0), rp::seed3<rp::Dual>(wo, seed_wo ? 0 : -1));
            out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = d.x.v; out[4] = d.y.v; out[5] = d.z.v;
            for (int k = 0; k < 3; ++k) { out[6 + k] = d.x.d[k]; out[9 + k] = d.y.d[k]; out[12 + k] = d.z.d[k]; }
        } break;
        case EPSM_PROBE_REPARAM_FRESNEL: {             // in: cos_theta_i, eta, k -> rp::fresnel_conductor_t<rp::Dual>: F, d F / d cos
            rp::Dual c(in[0]);
            c.d[0] = 1.f;
            const rp::Dual F = rp::fresnel_conductor_t<rp::Dual>(c, in[1], in[2]);
            out[0] = F.v; out[1] = F.d[0];
        } break;
        default: break;
    }
}

// ---- epsm_probe_rays (include/epsm_trace.h): one row of caller-given rays in, one hit out.  The traversal itself is the
// tracer's (intersect, packet_intersect) on the stack the caller of these helpers hands over; nothing of it is restated here.
EPSM_HD bool probe_ray_load(const float *row, Ray &r) {                  // -> the row carries a ray
    r.o = f3(row[0], row[1], row[2]); r.d = f3(row[3], row[4], row[5]); r.maxt = row[6];
    return row[7] != 0.f;
}
EPSM_HD TriHit probe_ray_miss(const Ray &r) { TriHit th; th.hit = false; th.tri = 0; th.t = r.maxt; th.u = th.v = 0.f; return th; }
EPSM_HD void probe_ray_store(uint32_t *out, const TriHit &th) {
    out[0] = th.hit ? th.tri : 0xffffffffu; out[1] = f2u(th.t); out[2] = f2u(th.u); out[3] = f2u(th.v);
}
template <bool ANY_HIT>
EPSM_HD void probe_ray_row(const EpsmScene &S, const float *row, uint32_t *out, const BvhStack &st) {
    Ray r;
    const bool on = probe_ray_load(row, r);
    probe_ray_store(out, on ? intersect<ANY_HIT>(S, r, st) : probe_ray_miss(r));
}
EPSM_HD bool probe_rays_wavefront_form(int form) { return form == EPSM_RAYS_WAVEFRONT || form == EPSM_RAYS_WAVEFRONT_ANY; }
// what every build of epsm_probe_rays refuses before it touches anything (NULL: fine); `need` = the form's workspace bytes
EPSM_HD const char *probe_rays_refusal(const EpsmScene *scene, int form, int64_t n, const float *rays, const uint32_t *out,
                                       const void *workspace, size_t workspace_bytes, size_t need) {
    if (form < 0 || form >= EPSM_RAYS_FORM_COUNT) return "epsm_probe_rays: unknown form";
    if (n < 0) return "epsm_probe_rays: n < 0";
    if (n == 0) return nullptr;
    if (!scene || !rays || !out) return "epsm_probe_rays: NULL argument";
    if (scene->n_nodes < 0 || (scene->n_nodes > 0 && (!scene->bvh || !scene->prim_index || !scene->tri_verts)))
        return "epsm_probe_rays: the scene has nodes but no bvh / prim_index / tri_verts";
    if (need > 0 && (!workspace || workspace_bytes < need)) return "epsm_probe_rays: workspace NULL or too small";
    return nullptr;
}

EPSM_HD bool probe_needs_bsdf(int what) {
    return what == EPSM_PROBE_MICROFACET || what == EPSM_PROBE_MICROFACET_SAMPLE || what == EPSM_PROBE_BSDF_SAMPLE || what == EPSM_PROBE_BSDF_EVAL ||
           what == EPSM_PROBE_MICROFACET_DALPHA || what == EPSM_PROBE_BSDF_DALPHA || what == EPSM_PROBE_REPARAM_BSDF;
}
EPSM_HD bool probe_needs_sensor(int what) { return what == EPSM_PROBE_PRIMARY_RAY; }

}  // namespace epsm
