// TEST HARNESS ONLY: cp_core_host.cpp -- epsm_cp_core.h compiled for the host, calc_grad's dense lists -- plus the one number
// the dense lists do not carry: geta = d / d eta_k per (vertex, path), the gradient with respect to the record's eta that
// cp::manifold_contract / cp::caustic_finish return beside gn (EPSM_OPT_IOR_GRADS).  The loops are those of
// manifold_one / caustic_one; the arithmetic is the kernel's own.  Built on demand by tests/_ior_host.py.  Not shipped.
#include "cp_core_host.cpp"

// geta: (K, N), after the clamp / NaN rule of the per-vertex values (finalize); rows the kernel drops are 0
template <typename R> static void manifold_geta(const HostArgs<R> &A, int64_t i, R *geta) {
    const uint32_t plan = cp::manifold_plan(flag_word(A, i));
    const int nv = cp::plan_nv(plan), m = cp::plan_m(plan);
    cp::Pts<R> pts[kMaxVertices + 1];
    cp::MBlocks<R> ev[kMaxVertices + 1];
    cp::MFwd<R> fw[kMaxVertices + 2];
    for (int k = 1; k <= m; ++k) {
        const bool has_next = k + 1 <= nv;
        const cp::Own<R> own = own_of(A, k, i);
        cp::Nbr<R> next; next.x = next.e1 = next.e2 = zero3<R>();
        if (has_next) next = nbr_of(A, k + 1, i);
        const cp::Nbr<R> prev = nbr_of(A, k - 1, i);
        ev[k] = cp::manifold_blocks(own, prev, next, cp::plan_a(plan, k), has_next);
        pts[k] = pts_of(own, prev, next);
    }
    fw[0] = cp::mfwd_zero<R>();
    for (int k = 1; k <= m; ++k)
        fw[k] = cp::manifold_fwd(ev[k], d_of(A, k, i), k == 1, fw[k - 1], k > 1 ? ev[k - 1].Aup : ev[k].Aup, cp::plan_a(plan, k), k + 1 <= nv);
    cp::MBwd<R> nb; nb.q = mk2<R>(R(0), R(0)); nb.W = 0;
    for (int k = m; k >= 1; --k) {
        cp::MBwd<R> mine;
        const cp::MSeeds<R> sd = cp::manifold_bwd(ev[k], fw[k], nb, cp::plan_a(plan, k), cp::plan_b(plan, k), k + 1 <= nv, mine);
        nb = mine;
        geta[(int64_t) (k - 1) * A.N + i] = finalize(cp::manifold_contract(pts[k], sd, k + 1 <= nv).geta, A.clip);
    }
}

template <typename R> static void caustic_geta(const HostArgs<R> &A, int64_t i, R *geta) {
    const uint32_t plan = cp::caustic_plan(flag_word(A, i));
    const int m = cp::plan_m(plan), idstar = cp::plan_idstar(plan);
    cp::CFwd<R> fw[kMaxVertices + 2];
    cp::CBlocks<R> ev[kMaxVertices + 1];
    R g[kMaxVertices + 1];
    fw[0] = cp::cfwd_zero<R>();
    bool poisoned = false;
    for (int k = 1; k <= m; ++k) {
        const cp::Own<R> own = own_of(A, k, i);
        const cp::Nbr<R> prev = nbr_of(A, k - 1, i), next = nbr_of(A, k + 1, i);
        ev[k] = cp::caustic_blocks(own, prev, next, k == 1);
        fw[k] = cp::caustic_fwd(ev[k], d_of(A, k, i), k == 1, fw[k - 1], k > 1 ? ev[k - 1].Aup : ev[k].Aup);
        if (k == idstar && !fw[k].fin) poisoned = true;
        g[k] = cp::caustic_finish(pts_of(own, prev, next), fw[k], k == 1, k <= idstar, k == idstar, cp::plan_b(plan, k)).geta;
    }
    for (int k = 1; k <= m; ++k)
        if (!poisoned && k <= idstar) geta[(int64_t) (k - 1) * A.N + i] = finalize(g[k], A.clip);
}

template <typename R>
static int run_ior(int variant, int64_t N, int K, const void *cam, const EpsmVertexRecord *verts, const void *dlduv, int64_t stride, int dcols,
                   const void *dldp, double clip, void *op, void *ol, void *od, void *geta) {
    const int rc = run<R>(variant, N, K, cam, verts, dlduv, stride, dcols, dldp, clip, op, ol, od);
    if (rc != 0) return rc;
    HostArgs<R> A{};
    A.N = N; A.K = K;
    A.cam = (const R *) cam;
    for (int k = 0; k < K; ++k) {
        const EpsmVertexRecord &v = verts[k];
        VertexPtrs<R> &o = A.v[k];
        o.p0 = (const R *) v.p0; o.p1 = (const R *) v.p1; o.p2 = (const R *) v.p2;
        o.n0 = (const R *) v.n0; o.n1 = (const R *) v.n1; o.n2 = (const R *) v.n2;
        o.b0 = (const R *) v.b0; o.b1 = (const R *) v.b1; o.eta = (const R *) v.eta;
        o.light = (const R *) v.light;
        o.bsdf = v.bsdf; o.active = v.active; o.active_em = v.active_em; o.ismesh = v.ismesh;
    }
    A.dlduv = (const R *) dlduv; A.stride = stride; A.dcols = dcols > 2 * K ? 2 * K : dcols;
    A.dldp = (const R *) dldp;
    A.clip = (clip > 0 && clip < 1e300) ? (R) clip : realmax_(R(0));
    memset(geta, 0, sizeof(R) * (size_t) N * (size_t) K);
    for (int64_t i = 0; i < N; ++i) {
        if (variant == EPSM_VARIANT_MANIFOLD) manifold_geta(A, i, (R *) geta); else caustic_geta(A, i, (R *) geta);
    }
    return 0;
}

extern "C" int epsm_host_cp_ior_f32(int variant, int64_t N, int K, const void *cam, const EpsmVertexRecord *verts,
                                    const void *dlduv, int64_t stride, int dcols, const void *dldp, double clip,
                                    void *op, void *ol, void *od, void *geta) {
    return run_ior<float>(variant, N, K, cam, verts, dlduv, stride, dcols, dldp, clip, op, ol, od, geta);
}
extern "C" int epsm_host_cp_ior_f64(int variant, int64_t N, int K, const void *cam, const EpsmVertexRecord *verts,
                                    const void *dlduv, int64_t stride, int dcols, const void *dldp, double clip,
                                    void *op, void *ol, void *od, void *geta) {
    return run_ior<double>(variant, N, K, cam, verts, dlduv, stride, dcols, dldp, clip, op, ol, od, geta);
}
