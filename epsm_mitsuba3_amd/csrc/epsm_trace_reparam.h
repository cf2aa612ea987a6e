// epsm_trace_reparam.h -- the reparameterised backward pass of the hybrid scheme's second phase:
// gradients of vertex positions / normals through visibility, i.e. what `prb_reparam` adds to path replay.
//
// Restates, for the estimator of epsm_trace_core.h (path_bounce) and triangle meshes,
//   _sample_warp_field / _ReparameterizeOp.backward        src/python/python/ad/reparam.py:10-123, 224-333
//   PRBReparamIntegrator.sample (ADMode.Backward)           src/python/python/ad/integrators/prb_reparam.py:277-607
//   ADIntegrator.sample_rays (reparameterised film position) src/python/python/ad/integrators/common.py:376-421
//   Mesh::compute_surface_interaction's three AD modes + boundary test   src/render/mesh.cpp:652-700, 832-887
//   Rectangle's boundary test                                src/shapes/rectangle.cpp:320-321
// WITHOUT an AD system: a path replays under the primal pass's seed; every vertex `cur` evaluates its contribution
//   Lo = (Le + Lr_dir + Lr_ind) * det + extra                (prb_reparam.py:572)
// once more in DUAL numbers (forward mode) with respect to the few local quantities the reference's AD graph reaches
// from there -- the reparameterised direction d' of the ray into the vertex, that of the emitter ray, the three vertices
// and vertex normals of the triangle -- and hands the resulting adjoints (a) straight to the triangle's rows of the
// gradient buffers and (b) to the hand-derived adjoint of the warp field (reparam.py:269-327), which distributes them over
// the triangles its auxiliary rays hit (`FollowShape`: si.p = sum b_j p_j with the b_j detached) and over the ray origin.
// Sampling is detached as in the reference (pdfs, MIS weights, emitter samples are constants).
// Where a warp is traced is a policy (`Sink`): on the spot, one auxiliary ray after the other (InlineSink: the host build,
// the test probes), or left as a request for a second launch that gives every auxiliary ray its own lane (QueueSink:
// epsm_trace_reparam.hip).  Every auxiliary ray has its own random stream, so both trace the same rays.
//
// PARITY: no Dr.Jit here, so the pass as a whole is pinned by the reference's OWN recipe for this integrator
// (src/integrators/tests/test_ad_integrators.py:833-871: backward gradient against finite differences of the primal
// image), tests/test_reparam*.py, on the host build of this file and on the GPU.  Pinned by an independent float64
// restatement (tests/_warp_oracle.py), request by request in units of the sum of absolute terms: everything a warp computes
// from its request -- the drawn rays, boundary term, weights, Z, dZ, warp_backward / warp_forward and, on the device, stage 2's
// request list, lane groups, butterflies and per-triangle rounds (epsm_probe_reparam_warps; tests/test_warp_stage.py,
// tests/test_gpu_warp_stage.py) -- and the partials of bsdf_eval_t / fresnel_conductor_t against float64 autograd
// (EPSM_PROBE_REPARAM_BSDF / _FRESNEL).  Still unpinned by anything but the finite differences: surf_t and eval_lo as a whole,
// the film's Jacobian, and which warps a path asks for (stage 1).
#pragma once

#include "epsm_trace_core.h"

namespace epsm {
namespace rp {

constexpr int kMaxAux = 64;              // reparam_rays <= 64 (the reference's tests use 64, its default is 16)
constexpr int kD = 6;                    // partials carried per dual evaluation

// ---------------------------------------------------------------------------
// dual numbers: value + K partial derivatives (the backward pass carries kD basis partials per evaluation, the forward pass
// one directional derivative: DualN<1>)
// ---------------------------------------------------------------------------
template <int K> struct DualN {
    float v;
    float d[K];
    EPSM_HD DualN() {}
    EPSM_HD DualN(float x) : v(x) {
#pragma unroll
        for (int i = 0; i < K; ++i) d[i] = 0.f;
    }
};
using Dual = DualN<kD>;
template <int K> EPSM_HD DualN<K> operator+(DualN<K> a, DualN<K> b) { DualN<K> r; r.v = a.v + b.v; for (int i = 0; i < K; ++i) r.d[i] = a.d[i] + b.d[i]; return r; }
template <int K> EPSM_HD DualN<K> operator-(DualN<K> a, DualN<K> b) { DualN<K> r; r.v = a.v - b.v; for (int i = 0; i < K; ++i) r.d[i] = a.d[i] - b.d[i]; return r; }
template <int K> EPSM_HD DualN<K> operator-(DualN<K> a) { DualN<K> r; r.v = -a.v; for (int i = 0; i < K; ++i) r.d[i] = -a.d[i]; return r; }
template <int K> EPSM_HD DualN<K> operator*(DualN<K> a, DualN<K> b) { DualN<K> r; r.v = a.v * b.v; for (int i = 0; i < K; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i]; return r; }
template <int K> EPSM_HD DualN<K> operator/(DualN<K> a, DualN<K> b) {
    DualN<K> r; const float ib = 1.f / b.v; r.v = a.v * ib;
    for (int i = 0; i < K; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * ib;
    return r;
}
template <int K> EPSM_HD DualN<K> t_sqrt(DualN<K> a) { DualN<K> r; r.v = sqrtf(a.v); const float k = r.v > 0.f ? 0.5f / r.v : 0.f; for (int i = 0; i < K; ++i) r.d[i] = a.d[i] * k; return r; }
template <int K> EPSM_HD DualN<K> t_exp(DualN<K> a) { DualN<K> r; r.v = expf(a.v); for (int i = 0; i < K; ++i) r.d[i] = a.d[i] * r.v; return r; }
EPSM_HD float t_sqrt(float a) { return sqrtf(a); }
EPSM_HD float t_exp(float a) { return expf(a); }
EPSM_HD float val(float a) { return a; }
template <int K> EPSM_HD float val(DualN<K> a) { return a.v; }
// dr.replace_grad(primal, x): x's derivative on the stored primal value
template <int K> EPSM_HD DualN<K> replace_value(DualN<K> a, float primal) { a.v = primal; return a; }
EPSM_HD float replace_value(float, float primal) { return primal; }

template <class T> EPSM_HD V3<T> lift3(F3 a) { return mk3<T>(T(a.x), T(a.y), T(a.z)); }
template <class T> EPSM_HD V3<T> t_normalize(V3<T> v) { const T il = T(1.f) / t_sqrt(dot(v, v)); return v * il; }
template <class T> EPSM_HD T t_mulsign(T x, T s) { return val(s) < 0.f ? -x : x; }
template <class T> EPSM_HD T t_sqr(T x) { return x * x; }
template <class T> EPSM_HD void t_coordinate_system(V3<T> n, V3<T> &s, V3<T> &t) {                 // vector.h (Duff et al.)
    const T sign = T(val(n.z) >= 0.f ? 1.f : -1.f), a = T(-1.f) / (sign + n.z), b = n.x * n.y * a;
    s = mk3<T>(t_mulsign(n.x * n.x * a, n.z) + T(1.f), t_mulsign(b, n.z), t_mulsign(-n.x, n.z));
    t = mk3<T>(b, n.y * n.y * a + sign, -n.y);
}

// ---------------------------------------------------------------------------
// the surface interaction as a function of (ray, triangle) -- mesh.cpp:652-827
// ---------------------------------------------------------------------------
template <class T> struct SurfT { V3<T> p, n, shn, fs, ft, wi; T t, bu, bv; };      // bu, bv: the weights of p1, p2 (prim_uv)
template <class T> EPSM_HD V3<T> to_local_t(const SurfT<T> &h, V3<T> v) { return mk3<T>(dot(v, h.fs), dot(v, h.ft), dot(v, h.shn)); }

// `u0, v0, t0`: the primal hit (prim_uv, t of the preliminary intersection: the derivative rides on them, mesh.cpp:690-695)
template <class T>
EPSM_HD SurfT<T> surf_t(V3<T> o, V3<T> d, V3<T> P0, V3<T> P1, V3<T> P2, V3<T> N0, V3<T> N1, V3<T> N2, uint32_t mesh_flags,
                        float u0, float v0, float t0) {
    SurfT<T> h;
    const V3<T> e1 = P1 - P0, e2 = P2 - P0;
    const V3<T> pvec = cross(d, e2);
    const T inv_det = T(1.f) / dot(e1, pvec);
    const V3<T> tvec = o - P0;
    const T u = replace_value(dot(tvec, pvec) * inv_det, u0);
    const V3<T> qvec = cross(tvec, e1);
    const T v = replace_value(dot(d, qvec) * inv_det, v0);
    h.t = replace_value(dot(e2, qvec) * inv_det, t0);
    const T b0 = T(1.f) - u - v;
    h.bu = u; h.bv = v;
    h.p = P0 * b0 + P1 * u + P2 * v;                                      // mesh.cpp:709
    h.n = t_normalize(cross(e1, e2));                                     // :729
    if (mesh_flags & EPSM_MESH_VERTEX_NORMALS) h.shn = t_normalize(N0 * b0 + N1 * u + N2 * v);     // :784-790
    else h.shn = h.n;
    if (mesh_flags & EPSM_MESH_FLIP_NORMALS) { h.n = -h.n; h.shn = -h.shn; }
    V3<T> dpdu, dpdv;
    t_coordinate_system(h.n, dpdu, dpdv);                                 // :734, SurfaceInteraction::initialize_sh_frame
    h.fs = t_normalize(dpdu - h.shn * dot(h.shn, dpdu));
    h.ft = cross(h.shn, h.fs);
    h.wi = to_local_t(h, -d);
    return h;
}

// ---------------------------------------------------------------------------
// BSDF values (incl. cosine) in T: diffuse.cpp:152-190, roughconductor.cpp:302-400; delta lobes evaluate to zero
// ---------------------------------------------------------------------------
template <class T> EPSM_HD T mf_eval_t(const EpsmBsdf &b, V3<T> m) {
    const float a = b.alpha;
    const T ct = m.z, ct2 = ct * ct;
    T result;
    if (b.distr == EPSM_DISTR_BECKMANN)
        result = t_exp(-(t_sqr(m.x * T(1.f / a)) + t_sqr(m.y * T(1.f / a))) / ct2) / (T(kPi * a * a) * t_sqr(ct2));
    else
        result = T(1.f) / (T(kPi * a * a) * t_sqr(t_sqr(m.x * T(1.f / a)) + t_sqr(m.y * T(1.f / a)) + t_sqr(m.z)));
    return val(result) * val(ct) > 1e-20f ? result : T(0.f);
}
template <class T> EPSM_HD T mf_smith_g1_t(const EpsmBsdf &b, V3<T> v, V3<T> m) {
    const T xy_alpha_2 = t_sqr(v.x * T(b.alpha)) + t_sqr(v.y * T(b.alpha)), tan2 = xy_alpha_2 / t_sqr(v.z);
    T result;
    if (b.distr == EPSM_DISTR_BECKMANN) {
        const T a = T(1.f) / t_sqrt(tan2), a2 = a * a;
        result = val(a) >= 1.6f ? T(1.f) : (a * T(3.535f) + a2 * T(2.181f)) / (T(1.f) + a * T(2.276f) + a2 * T(2.577f));
    } else {
        result = T(2.f) / (T(1.f) + t_sqrt(T(1.f) + tan2));
    }
    if (val(xy_alpha_2) == 0.f) result = T(1.f);
    if (val(dot(v, m)) * val(v.z) <= 0.f) result = T(0.f);
    return result;
}
template <class T> EPSM_HD T fresnel_conductor_t(T cos_i, float eta_r, float eta_i) {               // fresnel.h:92-117
    const T c2 = cos_i * cos_i, s2 = T(1.f) - c2, s4 = s2 * s2;
    const T temp_1 = T(eta_r * eta_r - eta_i * eta_i) - s2;
    const T x = temp_1 * temp_1 + T(4.f * eta_i * eta_i * eta_r * eta_r);
    const T a_2_pb_2 = val(x) > 0.f ? t_sqrt(x) : T(0.f);
    const T y = (a_2_pb_2 + temp_1) * T(0.5f);
    const T a = val(y) > 0.f ? t_sqrt(y) : T(0.f);
    const T term_1 = a_2_pb_2 + c2, term_2 = cos_i * a * T(2.f);
    const T r_s = (term_1 - term_2) / (term_1 + term_2);
    const T term_3 = a_2_pb_2 * c2 + s4, term_4 = term_2 * s2;
    const T r_p = r_s * (term_3 - term_4) / (term_3 + term_4);
    return (r_s + r_p) * T(0.5f);
}
template <class T> EPSM_HD V3<T> bsdf_eval_restated_t(const EpsmBsdf &b, V3<T> wi, V3<T> wo) {
    if (b.twosided && val(wi.z) < 0.f) { wi.z = -wi.z; wo.z = -wo.z; }
    const T cti = wi.z, cto = wo.z;
    if (!(val(cti) > 0.f && val(cto) > 0.f)) return zero3<T>();
    if (b.type == EPSM_BSDF_DIFFUSE_T) return lift3<T>(ld3(b.reflectance)) * (cto * T(kInvPi));
    if (b.type == EPSM_BSDF_ROUGHCONDUCTOR_T) {
        const V3<T> H = t_normalize(wi + wo);
        const T D = mf_eval_t(b, H);
        if (val(D) == 0.f) return zero3<T>();
        const T G = mf_smith_g1_t(b, wi, H) * mf_smith_g1_t(b, wo, H);
        const T result = D * G / (cti * T(4.f));
        const T c = dot(wi, H);
        return mk3<T>(fresnel_conductor_t(c, b.eta[0], b.k[0]) * T(b.reflectance[0]) * result,
                      fresnel_conductor_t(c, b.eta[1], b.k[1]) * T(b.reflectance[1]) * result,
                      fresnel_conductor_t(c, b.eta[2], b.k[2]) * T(b.reflectance[2]) * result);
    }
    return zero3<T>();                                                    // conductor / dielectric: delta lobes
}
// The BSDF value the passes differentiate: the restatement above supplies the PARTIALS, the value is the primal's own --
// bsdf_eval_pdf's float arithmetic at the same directions (dr.replace_grad(primal, x)).  The two copies round differently (up to
// 10 ulp for GGX, 120 ulp in Beckmann's tail, whose exp multiplies an ulp of its argument by the argument): tied here, the dual
// value is the number the tracer shaded with, and eval_lo's ratios f / f0 against bsdf_eval_pdf are exactly 1 in value.
template <class T> EPSM_HD V3<T> bsdf_eval_t(const EpsmBsdf &b, V3<T> wi, V3<T> wo) {
    const V3<T> r = bsdf_eval_restated_t<T>(b, wi, wo);
    F3 primal; float pdf;
    bsdf_eval_pdf(b, f3(val(wi.x), val(wi.y), val(wi.z)), f3(val(wo.x), val(wo.y), val(wo.z)), primal, pdf);
    return mk3<T>(replace_value(r.x, primal.x), replace_value(r.y, primal.y), replace_value(r.z, primal.z));
}

// ---------------------------------------------------------------------------
// the warp field (reparam.py:10-123): auxiliary rays around a ray, harmonic weights, the field's value and the
// ingredients of its divergence
// ---------------------------------------------------------------------------
struct Aux {
    float w;                 // harmonic weight (detached)
    F3 dw;                   // its gradient w.r.t. tangential changes of ray.d (detached)
    F3 v;                    // V_direct: normalize(si.p - ray.o), or ray.d for a miss
    uint32_t tri;            // triangle hit (kNoIndex: none)
    float b1, b2, inv_dist;  // barycentrics of the hit (FollowShape: detached), 1 / |si.p - ray.o|
};
struct Warp {
    int n;                   // auxiliary rays collected (0: reparameterisation inactive -> identity, no gradient)
    float Z;
    F3 dZ, o, d;
    Aux a[kMaxAux];
};
struct ReparamCfg { int max_depth, rays; float kappa, exponent; uint32_t flags; };      // flags: EPSM_REPARAM_* (epsm_trace.h)
// The pass's own arguments behind replay_args_fill, device library and host twin alike: NULL = fine and cfg filled, otherwise
// what is wrong.
inline const char *reparam_cfg_fill(ReparamCfg &cfg, const EpsmScene *scene, int reparam_max_depth, int reparam_rays, float kappa,
                                    float exponent, uint32_t flags) {
    if (reparam_rays < 1 || reparam_rays > kMaxAux || reparam_max_depth < 0 || !(kappa > 0.f) || !(exponent > 0.f))
        return "need 1 <= reparam_rays <= 64, reparam_max_depth >= 0, kappa > 0, exponent > 0";
    if (flags & ~EPSM_REPARAM_ANTITHETIC) return "unknown flag";
    // (this pass's own rule: there is nothing to move, and its kernels have not been tried on a scene without geometry)
    if (scene->n_triangles <= 0) return "the scene has no triangles";
    cfg.max_depth = reparam_max_depth; cfg.rays = reparam_rays; cfg.kappa = kappa; cfg.exponent = exponent; cfg.flags = flags;
    return nullptr;
}

// Boundary term of a hit (mesh.cpp:832-887; rectangle.cpp:320-321 for the tessellated rectangles)
EPSM_HD float boundary_test(const EpsmScene &S, const TriHit &th, F3 ray_d) {
    const uint32_t mi = S.tri_mesh[th.tri];
    const EpsmMesh m = S.meshes[mi];
    const float u = th.u, v = th.v, w = 1.f - u - v;
    if (!(m.flags & EPSM_MESH_IS_MESH)) {
        // rectangle = its first two triangles (v0 v1 v2), (v0 v2 v3): uv in [0,1]^2 along v1 - v0 and v2 - v1
        const uint32_t *i0 = S.tri + 3 * (int64_t) m.tri_begin;
        const F3 q0 = ld3(S.positions + 3 * (int64_t) i0[0]), q1 = ld3(S.positions + 3 * (int64_t) i0[1]), q2 = ld3(S.positions + 3 * (int64_t) i0[2]);
        const uint32_t *iv = S.tri + 3 * (int64_t) th.tri;
        const F3 p = ld3(S.positions + 3 * (int64_t) iv[0]) * w + ld3(S.positions + 3 * (int64_t) iv[1]) * u + ld3(S.positions + 3 * (int64_t) iv[2]) * v;
        const F3 eu = q1 - q0, ev = q2 - q1, r = p - q0;
        const float uu = dot(r, eu) / dot(eu, eu), vv = dot(r, ev) / dot(ev, ev);
        return fminf(0.5f - fabsf(uu - 0.5f), 0.5f - fabsf(vv - 0.5f));
    }
    const uint32_t *iv = S.tri + 3 * (int64_t) th.tri;
    if (!(m.flags & EPSM_MESH_VERTEX_NORMALS)) {
        // flat shading: distance to the nearest edge in an equilateral parameterisation, 1 at the barycentre
        const float s3 = 1.7320508075688772f;
        const float px = u + 0.5f * v, py = 0.5f * s3 * v;                // tp0 = (0,0), tp1 = (1,0), tp2 = (1/2, sqrt(3)/2)
        const float ex[3] = {1.f, -0.5f, -0.5f}, ey[3] = {0.f, 0.5f * s3, -0.5f * s3};
        const float ax[3] = {0.f, 1.f, 0.5f}, ay[3] = {0.f, 0.f, 0.5f * s3};
        float best = kInf;
        for (int e = 0; e < 3; ++e) {
            const float vx = px - ax[e], vy = py - ay[e];
            const float h = fminf(fmaxf((vx * ex[e] + vy * ey[e]) / (ex[e] * ex[e] + ey[e] * ey[e]), 0.f), 1.f);
            const float qx = vx - ex[e] * h, qy = vy - ey[e] * h;
            best = fminf(best, qx * qx + qy * qy);
        }
        return sqrtf(best) / (s3 / 6.f);
    }
    const F3 n = ld3(S.normals + 3 * (int64_t) iv[0]) * w + ld3(S.normals + 3 * (int64_t) iv[1]) * u + ld3(S.normals + 3 * (int64_t) iv[2]) * v;
    const float dp = -dot(n, ray_d);                                       // zero at silhouette points
    return dp * dp;
}

// Which warp of which path: the n-th reparameterize_ray call of path `widx` under the reparameterisation's own seed
// (common.py:1196-1203: 0xffffffff ^ seed).  Every auxiliary ray draws from its OWN stream, keyed by (seed, path, call,
// ray), so that the rays of a warp can be traced by different lanes (the device's second stage) or one after the other
// (the host build) with the same numbers.
struct WarpId { uint32_t key, widx; int n; };
// An auxiliary ray in two halves, so that the device can walk the rays of a wave TOGETHER between them (epsm_trace_packet.h):
// aux_begin draws the ray, aux_finish turns its closest hit into the warp's weight and its derivative.
struct AuxDraw { Ray ray; F3 tangent; float sy_; };                        // tangent = fs * omega.x + ft * omega.y
EPSM_HD AuxDraw aux_begin(const ReparamCfg &cfg, const WarpId &id, int r, F3 o, F3 d, F3 fs, F3 ft) {
    // antithetic pairs (reparam.py:82-84, 189-196): rays 2m and 2m + 1 share one sample; the even one mirrors it about the
    // ray (omega_local.x, .y negated), which cancels the odd part of the warp field's estimator
    const bool anti = (cfg.flags & EPSM_REPARAM_ANTITHETIC) != 0;
    const int rs = anti ? (r & ~1) : r;
    Pcg32 rng = seed_sampler(id.key ^ (0x9E3779B9u * (uint32_t) (id.n * 64 + rs + 1)), id.widx);
    const float kappa = cfg.kappa;
    const float sx = rng.next_1d(), sy_ = rng.next_1d();
    // warp.h:559-566 square_to_von_mises_fisher (1 - cos^2 formed without the cancellation of fp32)
    const float sy = fmaxf(1.f - sy_, 1e-6f);
    const float e = logf(sy + (1.f - sy) * expf(-2.f * kappa)) / kappa;             // cos_theta - 1 <= 0
    const float cos_theta = 1.f + e, sin_theta = safe_sqrt(-e * (2.f + e));
    const float phi = 2.f * kPi * sx;
    const float mirror = anti && !(r & 1) ? -1.f : 1.f;
    const F3 ol = f3(mirror * cosf(phi) * sin_theta, mirror * sinf(phi) * sin_theta, cos_theta);
    AuxDraw D;
    D.tangent = fs * ol.x + ft * ol.y;
    D.ray.o = o; D.ray.d = D.tangent + d * ol.z; D.ray.maxt = kInf;
    D.sy_ = sy_;
    return D;
}
EPSM_HD Aux aux_finish(const EpsmScene &S, const ReparamCfg &cfg, const AuxDraw &D, const TriHit &th, F3 o, F3 d) {
    const float kappa = cfg.kappa;
    Aux A;
    float B = 1.f;                                                         // reparam.py:104
    A.tri = kNoIndex; A.b1 = A.b2 = 0.f; A.inv_dist = 0.f; A.v = d;
    if (th.hit) {
        const uint32_t *iv = S.tri + 3 * (int64_t) th.tri;
        const F3 p = ld3(S.positions + 3 * (int64_t) iv[0]) * (1.f - th.u - th.v) + ld3(S.positions + 3 * (int64_t) iv[1]) * th.u +
                     ld3(S.positions + 3 * (int64_t) iv[2]) * th.v;
        const F3 r3 = p - o;
        const float dist = sqrtf(dot(r3, r3));
        if (dist > 0.f) {
            A.tri = th.tri; A.b1 = th.u; A.b2 = th.v; A.inv_dist = 1.f / dist; A.v = r3 * A.inv_dist;
            B = boundary_test(S, th, D.ray.d);
        }
    }
    const float inv_vmf = 1.f / (D.sy_ * expf(-2.f * kappa) + (1.f - D.sy_));              // reparam.py:111
    const float w_denom = inv_vmf - 1.f + B;
    const float w_denom_rcp = w_denom > 1e-4f ? 1.f / w_denom : 0.f;
    const float w = powf(w_denom_rcp, cfg.exponent) * inv_vmf;
    const float tmp1 = fminf(fmaxf(inv_vmf * w * w_denom_rcp * kappa * cfg.exponent, -1e10f), 1e10f);
    A.w = w;
    A.dw = D.tangent * tmp1;
    return A;
}
EPSM_HD Aux aux_ray(const EpsmScene &S, const ReparamCfg &cfg, const WarpId &id, int r, F3 o, F3 d, F3 fs, F3 ft, const BvhStack &st) {
    const AuxDraw D = aux_begin(cfg, id, r, o, d, fs, ft);
    return aux_finish(S, cfg, D, intersect<false>(S, D.ray, st), o, d);
}
// One call of reparameterize_ray's sampling loops (reparam.py:249-267 and 300-328 trace the same rays: kept instead of
// traced twice).
EPSM_HD void warp_collect(const EpsmScene &S, const ReparamCfg &cfg, const WarpId &id, F3 o, F3 d, const BvhStack &st, Warp &W) {
    W.n = cfg.rays; W.Z = 0.f; W.dZ = zero3<float>(); W.o = o; W.d = d;
    F3 fs, ft;
    coordinate_system(d, fs, ft);                                          // Frame3f(ray.d)
    for (int it = 0; it < cfg.rays; ++it) {
        W.a[it] = aux_ray(S, cfg, id, it, o, d, fs, ft, st);
        W.Z += W.a[it].w; W.dZ = W.dZ + W.a[it].dw;
    }
}

// ---------------------------------------------------------------------------
// accumulation into the gradient buffers
// ---------------------------------------------------------------------------
EPSM_HD void acc_add(float *p, float v) {
    // (a degenerate contribution -- a grazing ray's 1 / 0, a zero-length normal -- is dropped here instead of poisoning the
    // row for good; the reference scrubs NaN from the final parameter gradients, EPSM/optim.py:143-154)
    if (v == 0.f || !(fabsf(v) <= 3.0e38f)) return;
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
#pragma omp atomic
    *p += v;
#endif
}
struct GradOut { float *pos, *nrm; };                                      // (V,3) each, accumulated; nrm may be null
EPSM_HD void add_vertex(float *buf, uint32_t row, F3 g) { acc_add(buf + 3 * (int64_t) row, g.x); acc_add(buf + 3 * (int64_t) row + 1, g.y); acc_add(buf + 3 * (int64_t) row + 2, g.z); }
// d loss / d (a point glued to triangle `tri` at barycentrics b1, b2) = g  ->  the triangle's three vertices
EPSM_HD void add_follow_point(const EpsmScene &S, const GradOut &G, uint32_t tri, float b1, float b2, F3 g) {
    const EpsmMesh m = S.meshes[S.tri_mesh[tri]];
    if (!(m.flags & EPSM_MESH_POS_ATTACHED)) return;
    const uint32_t *iv = S.tri + 3 * (int64_t) tri;
    add_vertex(G.pos, iv[0], g * (1.f - b1 - b2)); add_vertex(G.pos, iv[1], g * b1); add_vertex(G.pos, iv[2], g * b2);
}

// Adjoint of one reparameterize_ray call (reparam.py:269-333) given d loss / d direction and d loss / d divergence:
// vertices of the triangles the auxiliary rays hit receive theirs; returns d loss / d ray.o and d loss / d ray.d.
EPSM_HD void warp_backward(const EpsmScene &S, const GradOut &G, const Warp &W, F3 g_dir, float g_div, F3 &g_o, F3 &g_d) {
    g_o = zero3<float>(); g_d = zero3<float>();
    if (W.n <= 0) return;
    const float Z = fmaxf(W.Z, 1e-8f), iZ = 1.f / Z;
    // direction = normalize(ray.d + V / Z), divergence = (div_V_1 - dot(V / Z, dZ)) / Z  at V = 0, div_V_1 = 0
    const F3 g_V = (g_dir - W.d * dot(W.d, g_dir)) * iZ - W.dZ * (g_div * iZ * iZ);
    const float g_div1 = g_div * iZ;
    // The divergence's two halves (dw_i g_div1 and the -dZ part of g_V) are each ~sqrt(kappa) times their sum and cancel
    // only over the auxiliary rays: the rays of a warp mostly hit the same one or two triangles, so their vertex
    // contributions are summed here in double, per triangle, before they go to the buffers.
    uint32_t tri[2] = {kNoIndex, kNoIndex};
    double acc[2][9], go[3] = {0.0, 0.0, 0.0};
    auto flush = [&](int e) {
        if (tri[e] == kNoIndex) return;
        const EpsmMesh m = S.meshes[S.tri_mesh[tri[e]]];
        if (m.flags & EPSM_MESH_POS_ATTACHED) {
            const uint32_t *iv = S.tri + 3 * (int64_t) tri[e];
            for (int j = 0; j < 3; ++j) add_vertex(G.pos, iv[j], f3((float) acc[e][3 * j], (float) acc[e][3 * j + 1], (float) acc[e][3 * j + 2]));
        }
        tri[e] = kNoIndex;
    };
    int victim = 0;
    for (int it = 0; it < W.n; ++it) {
        const Aux &A = W.a[it];
        const F3 g_v = g_V * A.w + A.dw * g_div1;                          // V_i = w V_direct, div_lhs_i = dot(d_w_omega, V_direct)
        if (A.tri == kNoIndex) { g_d = g_d + g_v; continue; }              // V_direct = ray.d (reparam.py:100)
        const F3 g_p = (g_v - A.v * dot(A.v, g_v)) * A.inv_dist;           // normalize(si.p - ray.o)
        int e = A.tri == tri[0] ? 0 : (A.tri == tri[1] ? 1 : -1);
        if (e < 0) {
            e = tri[0] == kNoIndex ? 0 : (tri[1] == kNoIndex ? 1 : victim);
            if (tri[e] != kNoIndex) { flush(e); victim ^= 1; }
            tri[e] = A.tri;
            for (int k = 0; k < 9; ++k) acc[e][k] = 0.0;
        }
        const double b[3] = {(double) (1.f - A.b1 - A.b2), (double) A.b1, (double) A.b2};
        for (int j = 0; j < 3; ++j) { acc[e][3 * j] += b[j] * g_p.x; acc[e][3 * j + 1] += b[j] * g_p.y; acc[e][3 * j + 2] += b[j] * g_p.z; }
        go[0] -= g_p.x; go[1] -= g_p.y; go[2] -= g_p.z;
    }
    flush(0); flush(1);
    g_o = f3((float) go[0], (float) go[1], (float) go[2]);
}

// The forward pass reads tangents where the backward adds gradients: (V,3) vertex-position / vertex-normal tangents of the
// meshes flagged EPSM_MESH_POS_ATTACHED / EPSM_MESH_NRM_ATTACHED (the rows of other meshes are not read); nrm may be null.
struct TanIn { const float *pos, *nrm; };
EPSM_HD F3 tan_vertex(const float *buf, uint32_t row) { return ld3(buf + 3 * (int64_t) row); }
// The motion of a point glued to triangle `tri` at barycentrics b1, b2: the gather that add_follow_point scatters
EPSM_HD F3 follow_tangent(const EpsmScene &S, const TanIn &T, uint32_t tri, float b1, float b2) {
    const EpsmMesh m = S.meshes[S.tri_mesh[tri]];
    if (!(m.flags & EPSM_MESH_POS_ATTACHED)) return zero3<float>();
    const uint32_t *iv = S.tri + 3 * (int64_t) tri;
    return tan_vertex(T.pos, iv[0]) * (1.f - b1 - b2) + tan_vertex(T.pos, iv[1]) * b1 + tan_vertex(T.pos, iv[2]) * b2;
}
// The tangent of V_direct of one auxiliary ray: the motion of its hit (glued to the triangle, b detached) minus that of the
// ray's origin `t_o`, projected by normalize(si.p - ray.o); a miss follows ray.d, which moves only for an emitter ray
// (em_inv_dist != 0: ray.d = normalize(ds.p - o)).  Transpose of the per-ray step of warp_backward.
EPSM_HD F3 aux_tangent(const EpsmScene &S, const TanIn &T, const Aux &A, F3 d, F3 t_o, float em_inv_dist) {
    if (A.tri == kNoIndex) return em_inv_dist != 0.f ? (t_o - d * dot(d, t_o)) * (-em_inv_dist) : zero3<float>();
    const F3 dp = follow_tangent(S, T, A.tri, A.b1, A.b2) - t_o;
    return (dp - A.v * dot(A.v, dp)) * A.inv_dist;
}
// Forward mode of one reparameterize_ray call (reparam.py:155-221) -- the transpose of warp_backward: from the tangent of
// every auxiliary ray's V_direct, the tangent of the reparameterised direction and of the divergence,
//   d' = iZ P(sum_i w_i v_i'),   div' = iZ sum_i (dw_i - w_i dZ / Z) . v_i'     (P = 1 - d d^T)
// with the terms that cancel over the rays (dw_i against w_i dZ / Z, each ~sqrt(kappa) times their sum) combined per ray and
// summed in double, as warp_backward sums its per-triangle shares.
struct WarpTan { F3 dir; float div; };
EPSM_HD WarpTan warp_forward(const EpsmScene &S, const TanIn &T, const Warp &W, F3 t_o, float em_inv_dist) {
    WarpTan r; r.dir = zero3<float>(); r.div = 0.f;
    if (W.n <= 0) return r;
    const float Z = fmaxf(W.Z, 1e-8f), iZ = 1.f / Z;
    const F3 dZn = W.dZ * iZ;
    double V[3] = {0.0, 0.0, 0.0}, div = 0.0;
    for (int it = 0; it < W.n; ++it) {
        const Aux &A = W.a[it];
        const F3 tv = aux_tangent(S, T, A, W.d, t_o, em_inv_dist);
        const F3 c = A.dw - dZn * A.w;
        V[0] += (double) A.w * tv.x; V[1] += (double) A.w * tv.y; V[2] += (double) A.w * tv.z;
        div += (double) dot(c, tv);
    }
    const F3 Vf = f3((float) V[0], (float) V[1], (float) V[2]);
    r.dir = (Vf - W.d * dot(W.d, Vf)) * iZ;
    r.div = (float) div * iZ;
    return r;
}

// ---------------------------------------------------------------------------
// what the differential step of a vertex needs to know about a vertex (captured from path_bounce, detached)
// ---------------------------------------------------------------------------
struct Vertex {
    bool valid;              // the path was alive and its ray hit something
    bool escaped;            // the path was alive and its ray left the scene (an environment emitter may shine along it)
    Ray ray;                 // the ray that arrived here
    TriHit th;
    SurfHit si;
    EpsmBsdf bsdf;
    uint32_t flags;
    F3 beta;                 // throughput on arrival
    F3 Le, Lr_dir;           // what this vertex added to L (already weighted by beta and MIS)
    F3 L_in, L_after;        // remaining radiance before / after those two terms (prb_reparam.py:435-436)
    EmitterSample es; bool active_em; float mis_em;
    BsdfSample bs; bool bs_valid;
    F3 wo_world;             // direction of the ray to the next vertex
    int depth;               // valid vertices before this one
};
EPSM_HD void vertex_clear(Vertex &v) { v.valid = false; v.escaped = false; v.L_in = v.L_after = v.Le = v.Lr_dir = zero3<float>(); v.active_em = false; v.bs_valid = false; v.depth = 0; }

// Which rays get a warp beside the ray into a valid vertex and the camera ray -- asked by both passes, so that request n of
// path i is the same warp in both.
EPSM_HD bool nonzero3(F3 a) { return a.x != 0.f || a.y != 0.f || a.z != 0.f; }
// a ray that left the scene towards an environment emitter carries that emitter's radiance: its warp's divergence multiplies it
// and its direction moves the lookup (prb_reparam.py:341-358 reparameterises every ray before it is known to hit).  (The camera
// ray has its own warp: prev == nullptr.)
EPSM_HD bool escaped_warp(const EpsmScene &S, const ReparamCfg &cfg, const Vertex *prev, const Vertex &cur) {
    return cur.escaped && prev && has_environment(S) && cur.depth < cfg.max_depth && nonzero3(cur.Le);
}
// the emitter ray of a vertex whose emitter sample added something (prb_reparam.py:394-411)
EPSM_HD bool emitter_warp(const ReparamCfg &cfg, const Vertex &cur) { return cur.active_em && cur.depth + 1 < cfg.max_depth && nonzero3(cur.Lr_dir); }

// path_bounce observer: copies what the bounce computed
struct Capture {
    Vertex *out;
    EPSM_HD void vertex(const SurfHit &si, const EpsmBsdf &bsdf, uint32_t flags, F3 Le, F3 Lr_dir, const EmitterSample &es,
                        bool active_em, float mis_em, const BsdfSample &bs, bool path_active) {
        Vertex &v = *out;
        v.valid = path_active && si.valid;
        v.si = si; v.bsdf = bsdf; v.flags = flags;
        v.Le = path_active ? Le : zero3<float>(); v.Lr_dir = path_active ? Lr_dir : zero3<float>();
        v.es = es; v.active_em = active_em && path_active; v.mis_em = mis_em;
        v.bs = bs; v.bs_valid = bs.valid;
        v.wo_world = to_world(si, bs.wo);
    }
};

// The vertex walk of both passes: path i replays under the primal seed through path_bounce, three Vertex records go round,
// and vertex j - 1's step runs when vertex j is known -- visit(prev, cur, next, j) for j = 1 .. max_depth with cur = vertex
// j - 1 (slots (j - 2, j - 1, j) mod 3; prev == nullptr at the first vertex, *next cleared behind the last bounce).  cur may be
// invalid (a dead path, or a ray that left the scene: cur.escaped).  `radiance_i`: L of the primal pass, from which the
// radiance still to come before / after a vertex's own terms is counted down (L_in, L_after: prb_reparam.py:435-436).
// `pr`: the camera ray, there before the first visit.  Returns whether the camera ray reached a vertex.
template <class Visit>
EPSM_HD bool walk_vertices(const TraceArgs &A, int64_t i, const BvhStack &st, const float *radiance_i, PrimaryRay &pr, Visit &&visit) {
    PathState s = path_begin(A, i, false, &pr);
    InlineVis vis{st};
    Vertex v[3];
    for (int k = 0; k < 3; ++k) vertex_clear(v[k]);
    F3 L_run = ld3(radiance_i);
    const int max_depth = path_max_depth(A);
    bool first_valid = false;
    for (int j = 0; j <= max_depth; ++j) {
        Vertex &nx = v[j % 3];
        vertex_clear(nx);
        if (j < max_depth) {
            TriHit th; th.hit = false; th.tri = 0; th.t = kInf; th.u = th.v = 0.f;
            const bool was_active = s.active;
            if (s.active) th = intersect<false>(A.S, s.ray, st);
            nx.ray = s.ray; nx.th = th; nx.beta = s.beta; nx.depth = s.depth;
            Capture cap{&nx};
            path_bounce(A, i, j, s, th, vis, cap);
            nx.valid = nx.valid && was_active;
            nx.escaped = was_active && !th.hit;
            nx.L_in = L_run;
            L_run = L_run - nx.Le - nx.Lr_dir;
            nx.L_after = L_run;
        }
        if (j == 0) continue;
        const Vertex &cur = v[(j - 1) % 3];
        if (j == 1) first_valid = cur.valid;
        visit(j >= 2 ? &v[(j - 2) % 3] : nullptr, cur, &nx, j);
    }
    return first_valid;
}

// The inputs of one dual evaluation of eval_lo, by index: d', d_em', P0, P1, P2, N0, N1, N2
enum { kInD = 0, kInDem = 1, kInP = 2, kInN = 5, kInputs = 8 };
template <class T> EPSM_HD V3<T> seed3(F3 a, int first) {
    V3<T> r = lift3<T>(a);
    if constexpr (!std::is_same<T, float>::value) {
        if (first >= 0) { r.x.d[first] = 1.f; r.y.d[first + 1] = 1.f; r.z.d[first + 2] = 1.f; }
    }
    return r;
}
// Per-slot seeds of one dual evaluation of the backward pass: which input carries partials k .. k + 2 (all others are constants)
struct Seeds {
    int d, dem, P[3], Nn[3];                                               // first partial index of each 3-vector, -1 = constant
    EPSM_HD int slot(int w) const { return w == kInD ? d : w == kInDem ? dem : w < kInN ? P[w - kInP] : Nn[w - kInN]; }
    EPSM_HD bool live(int w) const { return slot(w) >= 0; }
    template <class T> EPSM_HD V3<T> in(F3 a, int w) const { return seed3<T>(a, slot(w)); }
};
// The forward pass's seeds: every live input carries its TANGENT in the one partial of a DualN<1>
struct TanSeeds {
    bool on[kInputs];
    F3 t[kInputs];
    EPSM_HD bool live(int w) const { return on[w]; }
    template <class T> EPSM_HD V3<T> in(F3 a, int w) const {
        V3<T> r = lift3<T>(a);
        if constexpr (!std::is_same<T, float>::value) {
            if (on[w]) { r.x.d[0] = t[w].x; r.y.d[0] = t[w].y; r.z.d[0] = t[w].z; }
        }
        return r;
    }
};
template <class T> EPSM_HD T dot3c(F3 a, V3<T> b) { return b.x * T(a.x) + b.y * T(a.y) + b.z * T(a.z); }
template <class T> EPSM_HD V3<T> ratio3(F3 num, V3<T> f, F3 den, float floor_) {
    // num * f / max(floor, den) per channel (prb_reparam.py:541-542); zero where the detached value is zero
    return mk3<T>(den.x != 0.f ? f.x * T(num.x / fmaxf(floor_, den.x)) : T(0.f), den.y != 0.f ? f.y * T(num.y / fmaxf(floor_, den.y)) : T(0.f),
                  den.z != 0.f ? f.z * T(num.z / fmaxf(floor_, den.z)) : T(0.f));
}

// delta_L . [ (Le + Lr_dir + Lr_ind) + extra ] of vertex `cur` as a function of the seeded inputs (prb_reparam.py:362-572;
// the two determinants multiply terms whose values are known: handled by the caller).
template <class T, class SD>
EPSM_HD T eval_lo(const EpsmScene &S, const Vertex *prev, const Vertex &cur, const Vertex *next, F3 dL, const SD &sd) {
    const SurfHit &c = cur.si;
    const V3<T> o = lift3<T>(cur.ray.o);
    const V3<T> d = sd.template in<T>(cur.ray.d, kInD);
    const V3<T> P0 = sd.template in<T>(c.p0, kInP), P1 = sd.template in<T>(c.p1, kInP + 1), P2 = sd.template in<T>(c.p2, kInP + 2);
    // the stored normals are post-flip (surface_interaction); surf_t flips after interpolating, as mesh.cpp does
    const float fl = (c.mesh_flags & EPSM_MESH_FLIP_NORMALS) ? -1.f : 1.f;
    const V3<T> N0 = sd.template in<T>(c.n0 * fl, kInN), N1 = sd.template in<T>(c.n1 * fl, kInN + 1), N2 = sd.template in<T>(c.n2 * fl, kInN + 2);
    const SurfT<T> h = surf_t<T>(o, d, P0, P1, P2, N0, N1, N2, c.mesh_flags, cur.th.u, cur.th.v, cur.th.t);
    T s = T(0.f);
    // ---- a `bitmap` or per-vertex reflectance follows the point the ray sees: rho(uv') / rho(uv) per channel multiplies both BSDF values below
    //      (bitmap.cpp:366-418: the texture lookup is attached to si.uv, mesh.cpp:736-745)
    V3<T> tex = mk3<T>(T(1.f), T(1.f), T(1.f));
    if (cur.bsdf.texture >= 0 && cur.bsdf.texture < S.n_textures && cur.bsdf.type == EPSM_BSDF_DIFFUSE_T &&
        S.textures[cur.bsdf.texture].channels != 1) {
        F3 r0, du, dv;                                                     // rho at the primal hit, d rho / d (eu, ev)
        T eu, ev;                                                          // zero value, the derivative of what rho is looked up at
        bool on = true;
        if (tex_is_vertex(S.textures[cur.bsdf.texture])) {
            // ---- a per-vertex reflectance (mesh_attribute.cpp) follows it through the barycentrics themselves: rho = b0 c0 + b1 c1
            //      + b2 c2 with b0 = 1 - b1 - b2, so (b0' - b0) c0 + (bu - b1) c1 + (bv - b2) c2 = eu (c1 - c0) + ev (c2 - c0)
            const EpsmTexture &V = S.textures[cur.bsdf.texture];
            uint32_t q0, q1, q2;
            on = vertex_attr_rows(V, c, q0, q1, q2);                       // (outside the table: path_bounce kept the constant)
            r0 = du = dv = zero3<float>();
            if (on) {
                const F3 c0 = ld3(V.texels + 3 * (int64_t) q0), c1 = ld3(V.texels + 3 * (int64_t) q1), c2 = ld3(V.texels + 3 * (int64_t) q2);
                r0 = c0 * c.b0 + c1 * c.b1 + c2 * c.b2;                    // (vertex_attr_eval)
                du = c1 - c0; dv = c2 - c0;
            }
            eu = h.bu - T(c.b1); ev = h.bv - T(c.b2);
        } else {
            float a0[2] = {0.f, 0.f}, a1[2] = {1.f, 0.f}, a2[2] = {0.f, 1.f};                    // no texture coordinates: uv = (b1, b2)
            if ((c.mesh_flags & EPSM_MESH_HAS_UV) && S.texcoords)
                for (int j = 0; j < 2; ++j) { a0[j] = S.texcoords[2 * (int64_t) c.vi[0] + j]; a1[j] = S.texcoords[2 * (int64_t) c.vi[1] + j]; a2[j] = S.texcoords[2 * (int64_t) c.vi[2] + j]; }
            const T b0 = T(1.f) - h.bu - h.bv;
            const T uu = b0 * T(a0[0]) + h.bu * T(a1[0]) + h.bv * T(a2[0]), vv = b0 * T(a0[1]) + h.bu * T(a1[1]) + h.bv * T(a2[1]);
            r0 = tex_eval(S.textures[cur.bsdf.texture], c.uvx, c.uvy, &du, &dv);
            eu = uu - T(c.uvx); ev = vv - T(c.uvy);
        }
        if (on && r0.x > 0.f) tex.x = T(1.f) + (eu * T(du.x) + ev * T(dv.x)) * T(1.f / r0.x);
        if (on && r0.y > 0.f) tex.y = T(1.f) + (eu * T(du.y) + ev * T(dv.y)) * T(1.f / r0.y);
        if (on && r0.z > 0.f) tex.z = T(1.f) + (eu * T(du.z) + ev * T(dv.z)) * T(1.f / r0.z);
    }
    // ---- Lr_dir = beta * mis * bsdf(wi, to_local(d_em')) * em_weight (prb_reparam.py:413-418)
    if (cur.active_em && (cur.Lr_dir.x != 0.f || cur.Lr_dir.y != 0.f || cur.Lr_dir.z != 0.f)) {
        const V3<T> wo = to_local_t(h, sd.template in<T>(cur.es.d, kInDem));
        const V3<T> f0_ = bsdf_eval_t<T>(cur.bsdf, h.wi, wo);
        const V3<T> f = mk3<T>(f0_.x * tex.x, f0_.y * tex.y, f0_.z * tex.z);
        const F3 k = mul3(mul3(cur.beta, cur.es.weight), dL) * cur.mis_em;
        T em = T(1.f);
        const bool env_sample = cur.es.emitter >= 0 && !cur.es.delta && cur.es.tri == kNoIndex && has_environment(S) && cur.es.emitter == S.env.emitter;
        if (env_sample && sd.live(kInDem)) {
            // envmap.cpp:438-443 eval_direction at the reparameterised direction: L(d_em') / L(d_em) per channel, folded into
            // one factor weighted by what each channel contributes (k . f): d/d d_em of sum_c k_c f_c L_c(d') / L_c
            F3 g[3];
            const F3 L0 = env_eval_grad(S, cur.es.d, g);
            const V3<T> dd = sd.template in<T>(cur.es.d, kInDem);
            const float Lc[3] = {L0.x, L0.y, L0.z};
            const float kc[3] = {k.x, k.y, k.z};
            const T fc[3] = {f.x, f.y, f.z};
            T acc = T(0.f);
            for (int c2 = 0; c2 < 3; ++c2) {
                const T ratio = Lc[c2] > 0.f ? T(1.f - dot(g[c2], cur.es.d) / Lc[c2]) + dot3c(g[c2] * (1.f / Lc[c2]), dd) : T(1.f);
                acc = acc + fc[c2] * T(kc[c2]) * ratio;
            }
            s = s + acc;
        } else
        if (cur.es.delta) {
            // point.cpp:154-164 eval_direction: intensity / |ds.p - it.p|^2 with it = si_cur ATTACHED (an area light's
            // value has no such dependence, area.cpp:182-192; its falloff sits in the detached pdf and the warp's divergence)
            const V3<T> r = lift3<T>(cur.es.p) - h.p;
            em = T(cur.es.dist * cur.es.dist) / dot(r, r);
            s = s + dot3c(k, f) * em;
        } else {
            s = s + dot3c(k, f) * em;
        }
    }
    // ---- Lr_ind = L * bsdf(wi, to_local(ray_next.d)) / detached (prb_reparam.py:554-568)
    if (cur.bs_valid) {
        const V3<T> wo = to_local_t(h, lift3<T>(cur.wo_world));
        const V3<T> f1_ = bsdf_eval_t<T>(cur.bsdf, h.wi, wo);
        const V3<T> f = mk3<T>(f1_.x * tex.x, f1_.y * tex.y, f1_.z * tex.z);
        const F3 den = cur.bs.weight * cur.bs.pdf;                         // bsdf_weight * bsdf_sample.pdf
        const V3<T> r = mk3<T>(den.x != 0.f ? f.x * T(cur.L_after.x / den.x) : T(0.f), den.y != 0.f ? f.y * T(cur.L_after.y / den.y) : T(0.f),
                               den.z != 0.f ? f.z * T(cur.L_after.z / den.z) : T(0.f));
        s = s + dot3c(dL, r);
    }
    // ---- extra: the neighbours' BSDFs as the point moves along the reparameterised ray over the DETACHED triangle
    //      (prb_reparam.py:515-542; the emission at the next vertex has no directional derivative for area lights)
    const bool want_prev = prev && prev->valid, want_next = next && next->valid;
    if (sd.live(kInD) && (want_prev || want_next)) {
        const V3<T> e1 = lift3<T>(c.p1 - c.p0), e2 = lift3<T>(c.p2 - c.p0);
        const V3<T> pvec = cross(d, e2);
        const V3<T> qvec = lift3<T>(cross(cur.ray.o - c.p0, c.p1 - c.p0));
        const T t = replace_value(dot(e2, qvec) / dot(e1, pvec), cur.th.t);
        const V3<T> p = o + d * t;
        if (want_prev) {
            const SurfHit &q = prev->si;
            const V3<T> wo_w = t_normalize(p - lift3<T>(q.p));
            const V3<T> wo = mk3<T>(dot3c(q.fs, wo_w), dot3c(q.ft, wo_w), dot3c(q.shn, wo_w));
            const V3<T> f = bsdf_eval_t<T>(prev->bsdf, lift3<T>(q.wi), wo);
            F3 f0; float pdf0; bsdf_eval_pdf(prev->bsdf, q.wi, f3(val(wo.x), val(wo.y), val(wo.z)), f0, pdf0);
            s = s + dot3c(dL, ratio3<T>(cur.L_in, f, f0, 1e-8f));
        }
        if (want_next) {
            const SurfHit &q = next->si;
            const V3<T> wi_w = t_normalize(p - lift3<T>(q.p));
            const V3<T> wi = mk3<T>(dot3c(q.fs, wi_w), dot3c(q.ft, wi_w), dot3c(q.shn, wi_w));
            const V3<T> f = bsdf_eval_t<T>(next->bsdf, wi, lift3<T>(next->bs.wo));
            F3 f0; float pdf0; bsdf_eval_pdf(next->bsdf, f3(val(wi.x), val(wi.y), val(wi.z)), next->bs.wo, f0, pdf0);
            s = s + dot3c(dL, ratio3<T>(next->L_after, f, f0, 1e-8f));
        }
    }
    return s;
}

// ---------------------------------------------------------------------------
// per-path arguments and the camera's Jacobian
// ---------------------------------------------------------------------------
struct ReparamArgs {
    TraceArgs A;                 // scene, sensor, seed, spp, max_depth, rr_depth, path range (nothing logged)
    ReparamCfg cfg;
    const float *radiance;       // (N,3) L of the primal pass under the same seed
    const float *adj_radiance;   // (N,3) d loss / d L
    const float *adj_film;       // (N,3) d loss / d film position (x, y) and d loss / d det of the primary ray
    GradOut G;
};

// The film position as a function of the primary direction (common.py:405-418: the position is the projection of ray.o + d' by
// sensor.sample_direction; perspective.cpp's near plane is affine in the film position): what its derivative needs, both ways
struct CameraFrame {
    F3 c0, c1, c2;               // the camera axes in world space (the columns of to_world)
    F3 q;                        // ray.o + d in camera space (orthonormal to_world)
    float s;                     // [u, v] = q.xy * s = base.xy + px * dx.xy + py * dy.xy on the near plane
    float a, b, c, d, idet;      // A = [dx.xy dy.xy] = [a b; c d] and 1 / det A
};
EPSM_HD CameraFrame camera_frame(const EpsmSensor &C, const PrimaryRay &pr) {
    CameraFrame f;
    const float *W = C.to_world;
    f.c0 = f3(W[0], W[4], W[8]); f.c1 = f3(W[1], W[5], W[9]); f.c2 = f3(W[2], W[6], W[10]);
    const F3 origin = f3(W[3], W[7], W[11]);
    const F3 r = (pr.ray.o - origin) + pr.ray.d;
    f.q = f3(dot(f.c0, r), dot(f.c1, r), dot(f.c2, r));
    const F3 base = xform_point(C.sample_to_camera, f3(0.f, 0.f, 0.f));
    f.s = base.z / f.q.z;
    f.a = C.dx[0]; f.b = C.dy[0]; f.c = C.dx[1]; f.d = C.dy[1]; f.idet = 1.f / (f.a * f.d - f.b * f.c);
    return f;
}
// d loss / d film position -> d loss / d reparameterised primary direction: h = A^-T g, then through q.xy * s
EPSM_HD F3 film_to_direction(const EpsmSensor &C, const PrimaryRay &pr, float gx, float gy) {
    const CameraFrame f = camera_frame(C, pr);
    const float hx = (f.d * gx - f.c * gy) * f.idet, hy = (-f.b * gx + f.a * gy) * f.idet;
    const F3 gq = f3(f.s * hx, f.s * hy, -(f.q.x * hx + f.q.y * hy) * f.s / f.q.z);
    return f.c0 * gq.x + f.c1 * gq.y + f.c2 * gq.z;
}
// Transpose of film_to_direction: the tangent of the reparameterised primary direction -> that of the film position (pixels)
EPSM_HD void direction_to_film(const EpsmSensor &C, const PrimaryRay &pr, F3 td, float &fx, float &fy) {
    const CameraFrame f = camera_frame(C, pr);
    const F3 tq = f3(dot(f.c0, td), dot(f.c1, td), dot(f.c2, td));
    const float th = tq.z * f.s / f.q.z;
    const float hx = f.s * tq.x - f.q.x * th, hy = f.s * tq.y - f.q.y * th;
    fx = (f.d * hx - f.b * hy) * f.idet; fy = (-f.c * hx + f.a * hy) * f.idet;
}

// What happens to a warp once its ray and the adjoints of its direction / divergence are known.
//   o, d            the ray; g_dir, g_div: d loss / d direction, d loss / d divergence of its reparameterisation
//   ftri, fb1, fb2  the triangle + barycentrics its ORIGIN is glued to (kNoIndex: the camera)
//   em_inv_dist     emitter rays: 1 / |ds.p - o| -- their direction normalize(ds.p - o) follows the origin; else 0
// InlineSink: traced and back-propagated on the spot (the host build, and epsm_debug_*).
struct InlineSink {
    const EpsmScene &S; const ReparamCfg &cfg; const GradOut &G; const BvhStack &st; Warp &W; WarpId id;
    EPSM_HD void warp(F3 o, F3 d, F3 g_dir, float g_div, uint32_t ftri, float fb1, float fb2, float em_inv_dist) {
        warp_collect(S, cfg, id, o, d, st, W);
        id.n += 1;
        F3 g_o, g_d;
        warp_backward(S, G, W, g_dir, g_div, g_o, g_d);
        if (em_inv_dist != 0.f) g_o = g_o - (g_d - d * dot(d, g_d)) * em_inv_dist;
        if (ftri != kNoIndex) add_follow_point(S, G, ftri, fb1, fb2, g_o);
    }
};
// On the device a warp is a REQUEST for the second stage (epsm_trace_reparam.hip): the same eight things; gdir / gdiv hold the
// adjoints on the way in (backward pass) or the tangents d', div' on the way back (forward pass).
struct alignas(16) WarpReq { float o[3], gdiv, d[3], em_inv_dist, gdir[3], fb1; uint32_t ftri; float fb2, pad0, pad1; };
constexpr int kMaxReq = 1 + 2 * 6;           // the camera ray + two warps per vertex (epsm.py:549: at most six vertices)
EPSM_HD WarpReq make_request(F3 o, F3 d, F3 g_dir, float g_div, uint32_t ftri, float fb1, float fb2, float em_inv_dist) {
    WarpReq q;
    q.o[0] = o.x; q.o[1] = o.y; q.o[2] = o.z; q.gdiv = g_div; q.d[0] = d.x; q.d[1] = d.y; q.d[2] = d.z; q.em_inv_dist = em_inv_dist;
    q.gdir[0] = g_dir.x; q.gdir[1] = g_dir.y; q.gdir[2] = g_dir.z; q.fb1 = fb1; q.ftri = ftri; q.fb2 = fb2; q.pad0 = q.pad1 = 0.f;
    return q;
}
// the n-th request of path i of a tile of N paths: n-major, so that neighbouring lanes hold the same call of neighbouring paths
template <class Req> EPSM_HD Req &request_slot(Req *req, int64_t N, int n, int64_t i) { return req[(int64_t) n * N + i]; }
// The requests of path i in the order its walk asks for them (what the three device sinks are): next() is the slot of the
// following one, nullptr past kMaxReq -- such a warp is dropped (backward) or the identity (forward).
struct RequestCursor {
    WarpReq *req; int64_t N, i; int n;
    EPSM_HD WarpReq *next() {
        if (n >= kMaxReq) return nullptr;
        n += 1;
        return &request_slot(req, N, n - 1, i);
    }
};
// QueueSink: the request is written with the adjoints of its direction / divergence
struct QueueSink : RequestCursor {
    EPSM_HD void warp(F3 o, F3 d, F3 g_dir, float g_div, uint32_t ftri, float fb1, float fb2, float em_inv_dist) {
        if (WarpReq *q = next()) *q = make_request(o, d, g_dir, g_div, ftri, fb1, fb2, em_inv_dist);
    }
};

// The differential step of one vertex (prb_reparam.py:341-589).  The camera ray's direction adjoint goes back to the
// caller (`primary_g_dir`): its warp also serves the film's reparameterisation.
template <class Sink>
EPSM_HD void differential(const ReparamArgs &R, Sink &sink, const Vertex *prev, const Vertex &cur, const Vertex *next, F3 dL, F3 *primary_g_dir) {
    const EpsmScene &S = R.A.S;
    const SurfHit &c = cur.si;
    const bool first = prev == nullptr;
    const bool has_normals = (c.mesh_flags & EPSM_MESH_VERTEX_NORMALS) != 0;
    const EpsmMesh m = S.meshes[c.mesh];
    // ---- dual evaluations: [d', d_em'], [P0, P1], [P2, N0], [N1, N2]
    float g[24];
    for (int k = 0; k < 24; ++k) g[k] = 0.f;
    const bool want_pos = (m.flags & EPSM_MESH_POS_ATTACHED) != 0, want_nrm = has_normals && (m.flags & EPSM_MESH_NRM_ATTACHED) && R.G.nrm;
    for (int chunk = 0; chunk < 4; ++chunk) {
        Seeds sd; sd.d = sd.dem = -1; sd.P[0] = sd.P[1] = sd.P[2] = sd.Nn[0] = sd.Nn[1] = sd.Nn[2] = -1;
        if (chunk == 0) { sd.d = 0; sd.dem = 3; }
        else if (chunk == 1) { if (!want_pos) continue; sd.P[0] = 0; sd.P[1] = 3; }
        else if (chunk == 2) { if (!want_pos && !want_nrm) continue; sd.P[2] = 0; sd.Nn[0] = 3; }
        else { if (!want_nrm) continue; sd.Nn[1] = 0; sd.Nn[2] = 3; }
        const Dual s = eval_lo<Dual, Seeds>(S, prev, cur, next, dL, sd);
        for (int k = 0; k < kD; ++k) g[6 * chunk + k] = s.d[k];
    }
    if (want_pos) {
        add_vertex(R.G.pos, c.vi[0], f3(g[6], g[7], g[8])); add_vertex(R.G.pos, c.vi[1], f3(g[9], g[10], g[11]));
        add_vertex(R.G.pos, c.vi[2], f3(g[12], g[13], g[14]));
    }
    if (want_nrm) {
        add_vertex(R.G.nrm, c.vi[0], f3(g[15], g[16], g[17])); add_vertex(R.G.nrm, c.vi[1], f3(g[18], g[19], g[20]));
        add_vertex(R.G.nrm, c.vi[2], f3(g[21], g[22], g[23]));
    }
    // ---- the ray into this vertex (prb_reparam.py:341-358): d', det (det = 1 for the camera ray: the film carries it);
    //      its origin follows the previous shape (si_prev.spawn_ray: offset_p along the detached normal)
    const F3 g_dir = f3(g[0], g[1], g[2]);
    if (first) *primary_g_dir = g_dir;
    else if (cur.depth < R.cfg.max_depth)
        sink.warp(cur.ray.o, cur.ray.d, g_dir, dot(dL, cur.L_in) /* (Le + Lr_dir + Lr_ind) has the value L_in */, prev->th.tri, prev->th.u, prev->th.v, 0.f);
    // ---- the emitter ray (prb_reparam.py:394-411): em_ray.d = normalize(ds.p - o) with o glued to this triangle
    //      (si_cur_follow.spawn_ray_to)
    if (emitter_warp(R.cfg, cur)) {
        float dist;
        const Ray er = spawn_ray_to(c, cur.es.p, dist);
        sink.warp(er.o, er.d, f3(g[3], g[4], g[5]), dot(dL, cur.Lr_dir), cur.th.tri, cur.th.u, cur.th.v, 1.f / dist);
    }
}

// One path of RBIntegrator.render_backward's second pass (common.py:944-955).
template <class Sink>
EPSM_HD void reparam_one_path(const ReparamArgs &R, int64_t i, const BvhStack &st, Sink &sink) {
    const TraceArgs &A = R.A;
    const F3 dL = ld3(R.adj_radiance + 3 * i);
    PrimaryRay pr;
    // ---- the camera ray: one warp serves sample_rays (film position + det, common.py:405-418) and the first vertex, whose
    //      direction adjoint it adds (g_first; the environment's where the ray hit nothing).  g_film is formed at the first
    //      visit (there is one: max_depth >= 1), once, for whichever of the two places asks for that warp; formed in both,
    //      the path kernel's scratch grows by 96 bytes per lane (MEASUREMENTS.md 26).
    F3 g_film = zero3<float>();
    const float g_det_film = R.adj_film[3 * i + 2];
    const bool hit = walk_vertices(A, i, st, R.radiance + 3 * i, pr, [&](const Vertex *prev, const Vertex &cur, const Vertex *next, int j) EPSM_LAMBDA {
        if (j == 1) g_film = film_to_direction(A.C, pr, R.adj_film[3 * i], R.adj_film[3 * i + 1]);
        if (!cur.valid) {                                                  // a dead path: every term is zero but an escaped ray's
            if (escaped_warp(A.S, R.cfg, prev, cur)) {
                F3 g[3];
                const F3 L0 = env_eval_grad(A.S, cur.ray.d, g);            // Le = beta mis L(d): d Le / d d = Le / L * grad L, per channel
                const F3 w = f3(L0.x > 0.f ? dL.x * cur.Le.x / L0.x : 0.f, L0.y > 0.f ? dL.y * cur.Le.y / L0.y : 0.f, L0.z > 0.f ? dL.z * cur.Le.z / L0.z : 0.f);
                sink.warp(cur.ray.o, cur.ray.d, g[0] * w.x + g[1] * w.y + g[2] * w.z, dot(dL, cur.L_in), prev->th.tri, prev->th.u, prev->th.v, 0.f);
            }
            return;
        }
        F3 g_first = zero3<float>();
        differential(R, sink, prev, cur, next, dL, &g_first);
        if (j == 1 && R.cfg.max_depth > 0) sink.warp(pr.ray.o, pr.ray.d, g_film + g_first, g_det_film, kNoIndex, 0.f, 0.f, 0.f);
    });
    if (!hit && R.cfg.max_depth > 0) {                                     // the camera ray hit nothing: the film's term, and the
        F3 g_env = zero3<float>();                                         // environment's radiance along the reparameterised ray
        if (has_environment(A.S)) {
            F3 g[3];
            env_eval_grad(A.S, pr.ray.d, g);
            g_env = g[0] * dL.x + g[1] * dL.y + g[2] * dL.z;
        }
        sink.warp(pr.ray.o, pr.ray.d, g_film + g_env, g_det_film, kNoIndex, 0.f, 0.f, 0.f);
    }
}

// ---------------------------------------------------------------------------
// the forward pass (epsm_trace_paths_reparam_forward): the transpose of reparam_one_path, statement by statement.  A warp is
// needed BEFORE the vertex it serves (its d' tangent feeds the dual evaluation), so a sink returns the warp's tangents:
//   InlineFwdSink  traced and evaluated on the spot (the host build)
//   RecordSink     stage 1 of the device: the request is written (ray, glued origin, em_inv_dist), nothing is evaluated
//   ReadSink       stage 3 of the device: the tangents stage 2 left in the request (gdir, gdiv) are read back
// Both passes ride walk_vertices and ask for a vertex's warps under the same predicates in the same order, and the device sinks
// are one RequestCursor: request n of path i is the same warp in both, so every warp draws the auxiliary rays the backward draws.
// ---------------------------------------------------------------------------
struct ReparamFwdArgs {
    TraceArgs A;
    ReparamCfg cfg;
    const float *radiance;       // (N,3) L of the primal pass under the same seed
    TanIn T;                     // (V,3) tangents of the vertex positions / normals
    float *d_radiance;           // (N,3) out: dL
    float *d_film;               // (N,3) out: d film position (x, y) and d det of the primary ray
};
struct InlineFwdSink {
    static constexpr bool kEval = true;
    const EpsmScene &S; const ReparamCfg &cfg; const TanIn &T; const BvhStack &st; Warp &W; WarpId id;
    EPSM_HD WarpTan warp(F3 o, F3 d, uint32_t ftri, float fb1, float fb2, float em_inv_dist) {
        warp_collect(S, cfg, id, o, d, st, W);
        id.n += 1;
        const F3 t_o = ftri != kNoIndex ? follow_tangent(S, T, ftri, fb1, fb2) : zero3<float>();
        return warp_forward(S, T, W, t_o, em_inv_dist);
    }
};
EPSM_HD WarpTan identity_warp() { WarpTan r; r.dir = zero3<float>(); r.div = 0.f; return r; }     // no reparameterisation: nothing moves
struct RecordSink : RequestCursor {
    static constexpr bool kEval = false;
    EPSM_HD WarpTan warp(F3 o, F3 d, uint32_t ftri, float fb1, float fb2, float em_inv_dist) {
        if (WarpReq *q = next()) *q = make_request(o, d, zero3<float>(), 0.f, ftri, fb1, fb2, em_inv_dist);
        return identity_warp();
    }
};
struct ReadSink : RequestCursor {
    static constexpr bool kEval = true;
    EPSM_HD WarpTan warp(F3, F3, uint32_t, float, float, float) {
        WarpTan r = identity_warp();
        if (const WarpReq *q = next()) { r.dir = f3(q->gdir[0], q->gdir[1], q->gdir[2]); r.div = q->gdiv; }
        return r;
    }
};

// Forward form of `differential`: the vertex's warps first (the ray into it, its emitter ray; for the first vertex the camera
// ray, in the order the backward pass asks for them), then one DualN<1> evaluation of eval_lo per colour channel with every
// input seeded by its tangent.  Adds d(Le + Lr_dir + Lr_ind + extra) and the divergence terms to dLo; the camera ray's warp
// goes back to the caller (`cam`).
template <class Sink>
EPSM_HD void differential_forward(const ReparamFwdArgs &R, Sink &sink, const Vertex *prev, const Vertex &cur, const Vertex *next,
                                  const PrimaryRay &pr, F3 &dLo, WarpTan *cam) {
    const EpsmScene &S = R.A.S;
    const SurfHit &c = cur.si;
    const bool first = prev == nullptr;
    const bool has_normals = (c.mesh_flags & EPSM_MESH_VERTEX_NORMALS) != 0;
    const EpsmMesh m = S.meshes[c.mesh];
    TanSeeds sd;
    for (int k = 0; k < kInputs; ++k) { sd.on[k] = false; sd.t[k] = zero3<float>(); }
    WarpTan tin = identity_warp(), tem = identity_warp();
    if (!first && cur.depth < R.cfg.max_depth) {
        tin = sink.warp(cur.ray.o, cur.ray.d, prev->th.tri, prev->th.u, prev->th.v, 0.f);
        sd.on[kInD] = true;
    }
    const bool em = emitter_warp(R.cfg, cur);
    if (em) {
        float dist;
        const Ray er = spawn_ray_to(c, cur.es.p, dist);
        tem = sink.warp(er.o, er.d, cur.th.tri, cur.th.u, cur.th.v, 1.f / dist);
        sd.on[kInDem] = true;
    }
    if (first && R.cfg.max_depth > 0) {
        tin = sink.warp(pr.ray.o, pr.ray.d, kNoIndex, 0.f, 0.f, 0.f);
        sd.on[kInD] = true;
        *cam = tin;
    }
    if (!Sink::kEval) return;
    sd.t[kInD] = tin.dir; sd.t[kInDem] = tem.dir;
    if ((m.flags & EPSM_MESH_POS_ATTACHED) && R.T.pos)
        for (int j = 0; j < 3; ++j) { sd.on[kInP + j] = true; sd.t[kInP + j] = tan_vertex(R.T.pos, c.vi[j]); }
    if (has_normals && (m.flags & EPSM_MESH_NRM_ATTACHED) && R.T.nrm)
        for (int j = 0; j < 3; ++j) { sd.on[kInN + j] = true; sd.t[kInN + j] = tan_vertex(R.T.nrm, c.vi[j]); }
    bool any = false;
    for (int k = 0; k < kInputs; ++k) any = any || sd.on[k];
    if (any) {
        // eval_lo is linear in its weight dL: the unit weights give the three channels
        const float e[3][3] = {{1.f, 0.f, 0.f}, {0.f, 1.f, 0.f}, {0.f, 0.f, 1.f}};
        float out[3];
        for (int ch = 0; ch < 3; ++ch) out[ch] = eval_lo<DualN<1>, TanSeeds>(S, prev, cur, next, f3(e[ch][0], e[ch][1], e[ch][2]), sd).d[0];
        dLo = dLo + f3(out[0], out[1], out[2]);
    }
    // the divergences: that of the ray into the vertex multiplies (Le + Lr_dir + Lr_ind), whose value is L_in; the emitter
    // ray's multiplies Lr_dir.  (The camera ray's is the film's determinant: the caller's.)
    if (!first) dLo = dLo + cur.L_in * tin.div;
    if (em) dLo = dLo + cur.Lr_dir * tem.div;
}

// One path of the forward pass: d L and d (film x, film y, det) of path i for the tangents R.T.
template <class Sink>
EPSM_HD void reparam_forward_one_path(const ReparamFwdArgs &R, int64_t i, const BvhStack &st, Sink &sink) {
    const TraceArgs &A = R.A;
    PrimaryRay pr;
    F3 dLo = zero3<float>();
    WarpTan cam = identity_warp();
    const bool hit = walk_vertices(A, i, st, R.radiance + 3 * i, pr, [&](const Vertex *prev, const Vertex &cur, const Vertex *next, int) EPSM_LAMBDA {
        if (!cur.valid) {
            // an escaped ray towards an environment emitter: its warp's direction moves the lookup, its divergence multiplies L_in
            if (escaped_warp(A.S, R.cfg, prev, cur)) {
                const WarpTan t = sink.warp(cur.ray.o, cur.ray.d, prev->th.tri, prev->th.u, prev->th.v, 0.f);
                if (Sink::kEval) {
                    F3 g[3];
                    const F3 L0 = env_eval_grad(A.S, cur.ray.d, g);
                    dLo = dLo + f3(L0.x > 0.f ? dot(g[0], t.dir) * cur.Le.x / L0.x : 0.f, L0.y > 0.f ? dot(g[1], t.dir) * cur.Le.y / L0.y : 0.f,
                                   L0.z > 0.f ? dot(g[2], t.dir) * cur.Le.z / L0.z : 0.f) + cur.L_in * t.div;
                }
            }
            return;
        }
        differential_forward(R, sink, prev, cur, next, pr, dLo, &cam);
    });
    if (!hit && R.cfg.max_depth > 0) {                                     // the camera ray hit nothing: the film's term, and the
        cam = sink.warp(pr.ray.o, pr.ray.d, kNoIndex, 0.f, 0.f, 0.f);      // environment's radiance along the reparameterised ray
        if (Sink::kEval && has_environment(A.S)) {
            F3 g[3];
            env_eval_grad(A.S, pr.ray.d, g);
            dLo = dLo + f3(dot(g[0], cam.dir), dot(g[1], cam.dir), dot(g[2], cam.dir));
        }
    }
    if (!Sink::kEval) return;
    float fx, fy;
    direction_to_film(A.C, pr, cam.dir, fx, fy);
    R.d_radiance[3 * i] = dLo.x; R.d_radiance[3 * i + 1] = dLo.y; R.d_radiance[3 * i + 2] = dLo.z;
    R.d_film[3 * i] = fx; R.d_film[3 * i + 1] = fy; R.d_film[3 * i + 2] = cam.div;
}

// ---------------------------------------------------------------------------
// the workspace of both passes and what stage 2 alone needs (host side; device library and host twin alike)
// ---------------------------------------------------------------------------
// The requests of N paths (kMaxReq x N, n-major, rounded up to 256 bytes), then one count per path.
inline size_t request_bytes(int64_t N) { return ((size_t) N * kMaxReq * sizeof(WarpReq) + 255) & ~(size_t) 255; }
inline size_t workspace_bytes(int64_t N) { return N > 0 ? request_bytes(N) + (size_t) N * sizeof(int) : 0; }
// The n-th requests of all paths that stage 2 looks at, n = 0 .. n_max - 1: the camera ray + two warps per vertex the depths allow
inline int warp_stage_n_max(const TraceArgs &A) {
    const int depth = path_max_depth(A);
    return 1 + 2 * depth < kMaxReq ? 1 + 2 * depth : kMaxReq;
}
// epsm_probe_reparam_warps (include/epsm_trace.h): the arguments of stage 2 on requests the caller wrote.  NULL = fine, R.A (scene,
// seed, path range, max_depth: what the warp stage reads of it) and R.cfg filled (R zeroed by the caller); otherwise what is
// wrong.  N == 0 is fine whatever else is passed beside the scene.  `vertex_rows`: grad_pos or tan_pos.
template <class Args>
inline const char *probe_warps_fill(Args &R, const EpsmScene *scene, uint32_t seed, int64_t path_offset, int64_t N, int max_depth,
                                    int reparam_rays, float kappa, float exponent, uint32_t flags, const void *vertex_rows,
                                    const void *workspace, size_t workspace_size) {
    if (!scene) return "NULL scene";
    if (N == 0) return nullptr;
    if (N < 0 || max_depth < 1 || path_offset < 0 || path_offset + N > 0xFFFFFFFFLL) return "bad N / max_depth / path_offset";
    if (scene->n_triangles > 0 && (!scene->positions || !scene->normals || !scene->tri || !scene->tri_mesh || !scene->meshes ||
                                   !scene->bvh || !scene->prim_index || !scene->tri_verts))
        return "NULL scene array";
    if (!vertex_rows) return "NULL grad_pos (backward) / tan_pos (forward)";
    if (!workspace || workspace_size < workspace_bytes(N) || ((uintptr_t) workspace & 15u))
        return "workspace: 16-byte aligned, >= epsm_trace_reparam_workspace_bytes(N)";
    if (const char *why = reparam_cfg_fill(R.cfg, scene, 1, reparam_rays, kappa, exponent, flags)) return why;
    R.A.S = *scene; R.A.seed = seed; R.A.max_depth = max_depth; R.A.path_offset = path_offset; R.A.N = N;
    return nullptr;
}

}  // namespace rp
}  // namespace epsm
