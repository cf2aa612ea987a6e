// TEST HARNESS ONLY: the host build of the tracer (trace_host.cpp) plus the forward mode of the reparameterised pass,
// epsm_trace_paths_reparam_forward (include/epsm_trace.h) on host pointers.  Like the host backward pass, a path traces its
// warps on the spot (rp::InlineFwdSink): same auxiliary rays, same numbers as the device's three stages.  Built into its own
// library by tests/_forward_host.py.  Not shipped, not a fallback.
#include "trace_host.cpp"

extern "C" size_t epsm_trace_reparam_forward_workspace_bytes(int64_t) { return 0; }

extern "C" int epsm_trace_paths_reparam_forward(const EpsmScene *scene, const EpsmSensor *sensor, uint32_t seed, int spp, int max_depth,
                                                int rr_depth, int64_t path_offset, int64_t N, const float *radiance,
                                                const float *tan_pos, const float *tan_nrm, int reparam_max_depth, int reparam_rays,
                                                float kappa, float exponent, uint32_t flags, float *d_radiance, float *d_film, void *,
                                                size_t, void *) {
    rp::ReparamFwdArgs R = {};
    if (replay_args_fill(R.A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 1)) return -22;
    if (N == 0) return 0;
    if (!radiance || !tan_pos || !d_radiance || !d_film) return -22;
    if (rp::reparam_cfg_fill(R.cfg, scene, reparam_max_depth, reparam_rays, kappa, exponent, flags)) return -22;   // (as the device library)
    R.radiance = radiance; R.T.pos = tan_pos; R.T.nrm = tan_nrm; R.d_radiance = d_radiance; R.d_film = d_film;
    for_each_reparam_path(R.A, [&](int64_t i, const BvhStack &st, rp::Warp &W, const rp::WarpId &id) {
        rp::InlineFwdSink sink{R.A.S, R.cfg, R.T, st, W, id};
        rp::reparam_forward_one_path(R, i, st, sink);
    });
    return 0;
}
