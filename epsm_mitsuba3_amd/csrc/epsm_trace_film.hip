// epsm_trace_film.hip -- the film's kernels + their C ABI (include/epsm_trace.h): splat, its adjoint and its tangent, develop.
//
// ImageBlock::put (src/render/imageblock.cpp) with the reconstruction filter evaluated
// exactly (box: the pixel under the sample; gaussian: stddev 0.5, radius 4 sigma = 2,
// src/rfilters/gaussian.cpp) -- separable weights, float atomics into [r,g,b,w].
//
// The wavefront is ordered pixel-major, sample-minor (common.py:320-330), so the lanes of a wave are the
// samples of one pixel (spp >= 64) or of a few pixels (8, 16, 32 spp).  Lanes of an aligned group of G
// lanes that sit in the same pixel splat onto the same 5x5 window: their weighted radiances are summed
// with DPP adds and ONE lane issues the four atomics of a window pixel -- 100 atomics per group instead
// of 64 x 16 x 4 per wave (the render was bound by the atomic rate: 68 ms at 512x512 @ 64 spp).
// Arbitrary sample positions are still correct: a wave whose groups are not uniform splats lane by lane (G = 1).
#include <type_traits>

#include "epsm_common.h"
#include "epsm_trace_core.h"
#include "epsm_trace_launch.h"
#include "epsm_wave_scatter.h"           // dpp_add, wave_total_lane63

using namespace epsm;
using epsm_host::fail;

namespace {

// Sum over aligned groups of G lanes (all 64 lanes active); the last lane of each group holds the total.  G = 1: its own value.
template <int G> __device__ __forceinline__ float group_total(float v) {
    static_assert(G == 1 || G == 8 || G == 16 || G == 64, "the group sizes of for_pixel_group");
    if constexpr (G == 64) return wave_total_lane63(v);
    if constexpr (G == 8 || G == 16) {
        v = dpp_add<0xB1, 0xf>(v);                      // quad_perm [1,0,3,2]
        v = dpp_add<0x4E, 0xf>(v);                      // quad_perm [2,3,0,1]
        v = dpp_add<0x141, 0xf>(v);                     // row_half_mirror: 8 lanes
        if constexpr (G == 16) v = dpp_add<0x140, 0xf>(v);      // row_mirror: 16 lanes
    }
    return v;
}
// f(G) with the largest aligned group size -- 64, 16, 8, else 1, a compile-time constant -- whose lanes all sit in one pixel,
// the same for the whole wave
template <class F> __device__ __forceinline__ void for_pixel_group(int X, int Y, F f) {
    const int lane = threadIdx.x & 63;
    const int X8 = __shfl(X, lane & ~7), Y8 = __shfl(Y, lane & ~7);
    const int X16 = __shfl(X, lane & ~15), Y16 = __shfl(Y, lane & ~15);
    const int X64 = __builtin_amdgcn_readfirstlane(X), Y64 = __builtin_amdgcn_readfirstlane(Y);
    if (__ballot(X != X64 || Y != Y64) == 0ull) { f(std::integral_constant<int, 64>()); return; }
    if (__ballot(X != X16 || Y != Y16) == 0ull) { f(std::integral_constant<int, 16>()); return; }
    if (__ballot(X != X8 || Y != Y8) == 0ull) { f(std::integral_constant<int, 8>()); return; }
    f(std::integral_constant<int, 1>());
}

// The gaussian window of a sample: the 5 x 5 pixels around pixel (X, Y), separable weights and, with DERIV, their derivatives
// in the sample's position.  Pixel centres farther than the radius get weight 0 (gaussian_rfilter): the window holds exactly
// the pixels ImageBlock::put visits (ceil(p - r - 0.5) .. floor(p + r - 0.5)).  So does every pixel of a lane that is not
// `live` (past N: it takes part in the group sums with weight 0) and, with DERIV, every pixel off the film.  (The primal splat
// tests for the film at its atomics: with that test folded in here too it measured 1 % slower, MEASUREMENTS.md 24.)
template <bool DERIV> struct FilmWindow { int X, Y; float wx[5], wy[5]; };
template <> struct FilmWindow<true> : FilmWindow<false> { float dwx[5], dwy[5]; };
template <bool DERIV>
__device__ __forceinline__ FilmWindow<DERIV> film_window(float px, float py, int W, int H, bool live) {
    FilmWindow<DERIV> w;
    w.X = (int) floorf(px); w.Y = (int) floorf(py);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int x = w.X + j - 2, y = w.Y + j - 2;
        const float dx = (x + 0.5f) - px, dy = (y + 0.5f) - py;
        const bool lx = live && (!DERIV || (x >= 0 && x < W)), ly = live && (!DERIV || (y >= 0 && y < H));
        float ddx = 0.f, ddy = 0.f;
        const float fx = DERIV ? gaussian_rfilter_d(dx, ddx) : gaussian_rfilter(dx);
        const float fy = DERIV ? gaussian_rfilter_d(dy, ddy) : gaussian_rfilter(dy);
        w.wx[j] = lx ? fx : 0.f; w.wy[j] = ly ? fy : 0.f;
        if constexpr (DERIV) { w.dwx[j] = lx ? ddx : 0.f; w.dwy[j] = ly ? ddy : 0.f; }
    }
    return w;
}

template <int G>
__device__ __forceinline__ void splat_groups(const FilmWindow<false> &w, float r, float g, float b, int W, int H, float *accum) {
    const bool carrier = (threadIdx.x & (G - 1)) == G - 1;
#pragma unroll
    for (int jy = 0; jy < 5; ++jy) {
        const int y = w.Y + jy - 2;
#pragma unroll
        for (int jx = 0; jx < 5; ++jx) {
            const int x = w.X + jx - 2;
            const float wt = w.wy[jy] * w.wx[jx];
            const float sr = group_total<G>(r * wt), sg = group_total<G>(g * wt), sb = group_total<G>(b * wt),
                        sw = group_total<G>(wt);
            if (carrier && sw != 0.f && x >= 0 && y >= 0 && x < W && y < H) {
                float *a = accum + 4 * ((int64_t) y * W + x);
                atomicAdd(a + 0, sr); atomicAdd(a + 1, sg); atomicAdd(a + 2, sb); atomicAdd(a + 3, sw);
            }
        }
    }
}
__global__ __launch_bounds__(256) void epsm_film_splat_kernel(int64_t N, const float *pos, const float *rad, int W, int H,
                                                              int rfilter, float *accum) {
    const int64_t i0 = (int64_t) blockIdx.x * 256 + threadIdx.x;
    const bool live = i0 < N;
    const int64_t i = live ? i0 : N - 1;                // lanes past the end take part in the sums with weight 0
    const float px = pos[2 * i], py = pos[2 * i + 1];
    float r = rad[3 * i], g = rad[3 * i + 1], b = rad[3 * i + 2];
    if (rfilter == EPSM_RFILTER_BOX) {
        const int x = (int) floorf(px), y = (int) floorf(py);
        if (!live || x < 0 || y < 0 || x >= W || y >= H) return;
        float *a = accum + 4 * ((int64_t) y * W + x);
        atomicAdd(a + 0, r); atomicAdd(a + 1, g); atomicAdd(a + 2, b); atomicAdd(a + 3, 1.f);
        return;
    }
    const FilmWindow<false> w = film_window<false>(px, py, W, H, live);
    for_pixel_group(w.X, w.Y, [&](auto G) {
        if constexpr (decltype(G)::value > 1) splat_groups<decltype(G)::value>(w, r, g, b, W, H, accum);
        else {
            // lane by lane: a loop of its own, which leaves a row or a pixel before it forms the products (splat_groups<1>
            // issues the same atomics; 13.49 against 13.43 ms at 4.26 M scattered samples, MEASUREMENTS.md 24)
#pragma unroll
            for (int jy = 0; jy < 5; ++jy) {
                const int y = w.Y + jy - 2;
                if (y < 0 || y >= H) continue;
#pragma unroll
                for (int jx = 0; jx < 5; ++jx) {
                    const int x = w.X + jx - 2;
                    const float wt = w.wy[jy] * w.wx[jx];
                    if (x < 0 || x >= W || wt == 0.f) continue;
                    float *a = accum + 4 * ((int64_t) y * W + x);
                    atomicAdd(a + 0, r * wt); atomicAdd(a + 1, g * wt); atomicAdd(a + 2, b * wt); atomicAdd(a + 3, wt);
                }
            }
        }
    });
}
// Adjoint of the gaussian splat + weight division w.r.t. a sample's radiance, its FILM POSITION and the determinant of the
// reparameterisation that multiplies both its value and its weight (common.py:880-920; prb_reparam's pass between its two
// traces):   image[p] = sum_i w_ip L_i det_i / sum_i w_ip det_i,   w_ip = f(p - pos_i).
// One lane per sample, its 5 x 5 window of pixels: dL = sum_p w_ip grad_p / W_p;  A_p = grad_p . (L_i - image_p) / W_p;
// d/d pos.x = sum_p A_p wy dwx,  d/d pos.y = sum_p A_p dwy wx,  d/d det = sum_p A_p w.  (Round 3 ran this as ~40 small torch
// kernels per tile: integrators.film_adjoint_reparam, kept as the checker.)
__global__ __launch_bounds__(256) void epsm_film_adjoint_reparam_kernel(int64_t N, const float *pos, const float *rad, const float *grad,
                                                                        int grad_stride, const float *accum, int W, int H,
                                                                        float *dL, float *adj) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float r = rad[3 * i], g = rad[3 * i + 1], b = rad[3 * i + 2];
    const FilmWindow<true> w = film_window<true>(pos[2 * i], pos[2 * i + 1], W, H, true);
    float lr = 0.f, lg = 0.f, lb = 0.f, ax = 0.f, ay = 0.f, ad = 0.f;
#pragma unroll
    for (int jy = 0; jy < 5; ++jy) {
        const int y = min(max(w.Y + jy - 2, 0), H - 1);                 // (off the film: weight 0, any pixel will do)
#pragma unroll
        for (int jx = 0; jx < 5; ++jx) {
            const int x = min(max(w.X + jx - 2, 0), W - 1);
            const float w2 = w.wy[jy] * w.wx[jx], wdx = w.wy[jy] * w.dwx[jx], wdy = w.dwy[jy] * w.wx[jx];
            if (w2 == 0.f && wdx == 0.f && wdy == 0.f) continue;
            const int64_t p = (int64_t) y * W + x;
            const float Wp = accum[4 * p + 3];
            const float inv = Wp > 0.f ? 1.f / fmaxf(Wp, 1e-30f) : 0.f;
            const float *gp = grad + p * grad_stride;
            const float gr = gp[0] * inv, gg = gp[1] * inv, gb = gp[2] * inv;             // grad / W_p
            const float gi = (gr * accum[4 * p] + gg * accum[4 * p + 1] + gb * accum[4 * p + 2]) * inv;   // (grad . image) / W_p
            const float A = gr * r + gg * g + gb * b - gi;
            lr += gr * w2; lg += gg * w2; lb += gb * w2;
            ax += A * wdx; ay += A * wdy; ad += A * w2;
        }
    }
    dL[3 * i] = lr; dL[3 * i + 1] = lg; dL[3 * i + 2] = lb;
    adj[3 * i] = ax; adj[3 * i + 1] = ay; adj[3 * i + 2] = ad;
}
// Forward mode of the splat + weight division (common.py:880-920), the transpose of epsm_film_adjoint_reparam_kernel: one lane per
// sample, its 5 x 5 window (the box filter: the pixel under it).  Per pixel p, with w_ip = f(p - pos_i) and its gradient,
//   dA_p += (grad w . dpos_i + w ddet_i) L_i + w dL_i,    dW_p += grad w . dpos_i + w ddet_i
// into d_accum (H,W,4); the image's tangent is (dA - image dW) / W with the primal film.  d_film may be NULL (colour tangents:
// the samples do not move).  Lanes whose samples share a pixel sum over the group before the atomics, as epsm_film_splat_kernel
// does (one atomic per lane and pixel: 10.9 ms at 4.26 M samples, against 0.73 ms for the primal splat).
template <int G>
__device__ __forceinline__ void splat_tangent_groups(const FilmWindow<true> &w, const float *L, const float *T, const float *F, int W, int H,
                                                     float *d_accum) {
    const bool carrier = (threadIdx.x & (G - 1)) == G - 1;
#pragma unroll
    for (int jy = 0; jy < 5; ++jy) {
        const int y = w.Y + jy - 2;
#pragma unroll
        for (int jx = 0; jx < 5; ++jx) {
            const int x = w.X + jx - 2;
            const float w2 = w.wy[jy] * w.wx[jx];
            const float dw = w.wy[jy] * w.dwx[jx] * F[0] + w.dwy[jy] * w.wx[jx] * F[1] + w2 * F[2];      // d (w det)
            const float sr = group_total<G>(dw * L[0] + w2 * T[0]), sg = group_total<G>(dw * L[1] + w2 * T[1]),
                        sb = group_total<G>(dw * L[2] + w2 * T[2]), sw = group_total<G>(dw);
            // (the test for the film stays: a tangent may be anything, and weight 0 times a tangent that is not finite is not 0)
            if (carrier && x >= 0 && y >= 0 && x < W && y < H && (sr != 0.f || sg != 0.f || sb != 0.f || sw != 0.f)) {
                float *a = d_accum + 4 * ((int64_t) y * W + x);
                atomicAdd(a + 0, sr); atomicAdd(a + 1, sg); atomicAdd(a + 2, sb);
                if (sw != 0.f) atomicAdd(a + 3, sw);
            }
        }
    }
}
__global__ __launch_bounds__(256) void epsm_film_splat_tangent_kernel(int64_t N, const float *pos, const float *rad, const float *d_rad,
                                                                      const float *d_film, int W, int H, int rfilter, float *d_accum) {
    const int64_t i0 = (int64_t) blockIdx.x * 256 + threadIdx.x;
    const bool live = i0 < N;
    const int64_t i = live ? i0 : N - 1;                // lanes past the end take part in the sums with weight 0
    const float px = pos[2 * i], py = pos[2 * i + 1];
    const float T[3] = {d_rad[3 * i], d_rad[3 * i + 1], d_rad[3 * i + 2]};
    if (rfilter == EPSM_RFILTER_BOX) {                                    // (a box weight does not move with the sample)
        const int x = (int) floorf(px), y = (int) floorf(py);
        if (!live || x < 0 || y < 0 || x >= W || y >= H) return;
        float *a = d_accum + 4 * ((int64_t) y * W + x);
        atomicAdd(a + 0, T[0]); atomicAdd(a + 1, T[1]); atomicAdd(a + 2, T[2]);
        return;
    }
    const float L[3] = {rad[3 * i], rad[3 * i + 1], rad[3 * i + 2]};
    const float F[3] = {d_film ? d_film[3 * i] : 0.f, d_film ? d_film[3 * i + 1] : 0.f, d_film ? d_film[3 * i + 2] : 0.f};
    const FilmWindow<true> w = film_window<true>(px, py, W, H, live);
    for_pixel_group(w.X, w.Y, [&](auto G) { splat_tangent_groups<decltype(G)::value>(w, L, T, F, W, H, d_accum); });
}
__global__ __launch_bounds__(256) void epsm_film_develop_kernel(int64_t n, const float *accum, float *image) {
    const int64_t i = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float w = accum[4 * i + 3], iw = w != 0.f ? 1.f / w : 0.f;
    image[3 * i] = accum[4 * i] * iw; image[3 * i + 1] = accum[4 * i + 1] * iw; image[3 * i + 2] = accum[4 * i + 2] * iw;
}

}  // namespace

extern "C" int epsm_film_splat(int64_t N, const float *film_pos, const float *radiance, int width, int height,
                               int rfilter, float *accum, void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (N == 0) return EPSM_OK;
    if (N < 0 || !film_pos || !radiance || !accum || width < 1 || height < 1)
        return fail(EPSM_EINVAL, "epsm_film_splat: bad argument");
    return launch_checked("epsm_film_splat", epsm_film_splat_kernel, (N + 255) / 256, 256, stream,
                          N, film_pos, radiance, width, height, rfilter, accum);
}
extern "C" int epsm_film_adjoint_reparam(int64_t N, const float *film_pos, const float *radiance, const float *grad_img,
                                         int grad_channels, const float *accum, int width, int height, float *dL, float *adj,
                                         void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (N == 0) return EPSM_OK;
    if (N < 0 || !film_pos || !radiance || !grad_img || !accum || !dL || !adj || width < 1 || height < 1 || grad_channels < 3)
        return fail(EPSM_EINVAL, "epsm_film_adjoint_reparam: bad argument");
    return launch_checked("epsm_film_adjoint_reparam", epsm_film_adjoint_reparam_kernel, (N + 255) / 256, 256, stream,
                          N, film_pos, radiance, grad_img, grad_channels, accum, width, height, dL, adj);
}
extern "C" int epsm_film_develop(int width, int height, const float *accum, float *image, void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (!accum || !image || width < 1 || height < 1) return fail(EPSM_EINVAL, "epsm_film_develop: bad argument");
    const int64_t n = (int64_t) width * height;
    return launch_checked("epsm_film_develop", epsm_film_develop_kernel, (n + 255) / 256, 256, stream, n, accum, image);
}
extern "C" int epsm_film_splat_tangent(int64_t N, const float *film_pos, const float *radiance, const float *d_radiance,
                                       const float *d_film, int width, int height, int rfilter, float *d_accum, void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (N == 0) return EPSM_OK;
    if (N < 0 || !film_pos || !radiance || !d_radiance || !d_accum || width < 1 || height < 1)
        return fail(EPSM_EINVAL, "epsm_film_splat_tangent: bad argument");
    if (rfilter == EPSM_RFILTER_BOX && d_film)
        return fail(EPSM_EINVAL, "epsm_film_splat_tangent: a box filter has no derivative in the film position (d_film must be NULL)");
    return launch_checked("epsm_film_splat_tangent", epsm_film_splat_tangent_kernel, (N + 255) / 256, 256, stream,
                          N, film_pos, radiance, d_radiance, d_film, width, height, rfilter, d_accum);
}
