// epsm_trace_adjoint.h -- the device frame of the colour adjoint's replay passes ("the replay frame"): what the units
// epsm_trace_{texture,bsdf,material,alphamap}.hip share beyond the per-path code.  The lane prologue (replay_lane), the two
// ways a backward pass gets rid of its sums -- the atomic-free row reduction (SumSink, block_row_reduce, epsm_rows_sum_kernel)
// and the merged scatter into texel footprints (FootprintScatter) -- and the reducing pass's pair of launches (launch_reduced,
// on the checked launch of epsm_trace_launch.h).  Device only: hipcc, never the host harness.
//
// A unit describes its pass by a struct P:
//     Args                       the argument block (`A`, `adj`, what its sinks read)
//     Backward, Forward          the sinks; Forward is {T, i, has, d}
//     replay(T, i, has, s, th0, st, sink)    the pass's *_replay
// and keeps its __global__ kernels, their __launch_bounds__(128, 2) and their __shared__ arrays.
#pragma once

#include "epsm_common.h"
#include "epsm_trace_alphamap.h"         // tx::Item, am::NoItem: what a footprint sink is handed
#include "epsm_trace_launch.h"
#include "epsm_trace_packet.h"
#include "epsm_wave_scatter.h"           // make_runs / seg_sum: the merge before the atomics

namespace epsm {

// ---- the lane prologue ----
// One lane = one path, as epsm_trace_kernel traces it (the primary rays walked by the wave, the lane stacks in `s_stack`:
// kLaneStackLds * 128 words); lanes past N ride along without a path.  THE EXIT RULE belongs to the backward sink's type, so that
// no kernel can pick the wrong one:
//   * Backward::kReduces (SumSink): no early return.  Every wave of the workgroup reaches block_row_reduce's barrier, and a wave
//     without a path owes the reduction its zeros.  `has` is formed inside primary_hit.
//   * otherwise (FootprintScatter): a wave without a path returns; the others run whole, so that every lane reaches the merge.
//     `has` is formed here.
// (Both kernels of a pass follow its backward sink's rule: register allocation follows where `has` is formed, epsm_trace_packet.h.)
template <class P, bool BACKWARD>
__device__ __forceinline__ void replay_lane(const typename P::Args &T, uint32_t *s_stack, typename P::Backward &back) {
    uint32_t deep[kBvhStack - kLaneStackLds];
    const int64_t i = (int64_t) blockIdx.x * 128 + threadIdx.x;
    const BvhStack st = lane_stack(s_stack, deep, 128);
    constexpr bool kReduces = P::Backward::kReduces;
    const bool has = i < T.A.N;
    if constexpr (!kReduces) {
        if (__ballot(has) == 0ull) return;
    }
    // (initialised where it is declared: assigned in two branches, every kernel's instruction stream moved, MEASUREMENTS.md 23)
    PrimaryHit p = kReduces ? primary_hit(T.A, i, false, s_stack) : primary_hit(T.A, i, has, false, s_stack);
    if constexpr (BACKWARD) {
        back.begin(p.has ? ld3(T.adj + 3 * i) : zero3<float>());
        P::replay(T, p.i, p.has, p.s, p.th0, st, back);
    } else {
        typename P::Forward sink{T, p.i, p.has, zero3<float>()};
        P::replay(T, p.i, p.has, p.s, p.th0, st, sink);
    }
}

// ---- backward by reduction: a few numbers per launch, no atomics ----
// Per lane, `Sums` (ba::SlotSums, ma::MaterialSums: `adj`, `acc[ROW]`, clear(), item()) adds up the path's items.
template <class Sums>
struct SumSink {
    static constexpr bool kReduces = true;
    Sums sums;
    __device__ __forceinline__ void begin(F3 adj) { sums.adj = adj; sums.clear(); }
    template <class Item> __device__ __forceinline__ void item(const Item &it) { sums.item(it); }
    __device__ __forceinline__ void finish() {}
};

// the sum of v over the 64 lanes of the wave, in every lane (a butterfly: the same order of additions in every launch)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The workgroup's 128 lanes' acc[0 .. n_live) become one row of ROW partial sums (zeros from n_live on): a butterfly over each
// wave, the two waves through LDS, wave 0's sum + wave 1's.  All 128 threads call it (a barrier inside).  The order of the
// additions is part of the contract: results repeat bit for bit.
template <int ROW>
__device__ __forceinline__ void block_row_reduce(const float (&acc)[ROW], int n_live, float (&s_part)[2][ROW], float *partial_row) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < ROW; ++k) {
        const float v = k < n_live ? wave_sum(acc[k]) : 0.f;              // (wave-uniform condition)
        if (lane == 0) s_part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < ROW) partial_row[threadIdx.x] = s_part[0][threadIdx.x] + s_part[1][threadIdx.x];
}

// out[j] += sum over the rows of partial[row][j], in float64 and in a fixed order: thread t sums rows t, t + 256, ..., then a
// tree over the 256 threads.  One workgroup per live number j.
template <int ROW>
__global__ __launch_bounds__(256) void epsm_rows_sum_kernel(const float *partial, int64_t rows, float *out) {
    __shared__ double s_sum[256];
    const int j = blockIdx.x;
    double acc = 0.0;
    for (int64_t r = threadIdx.x; r < rows; r += 256) acc += (double) partial[r * ROW + j];
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int) threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[j] += (float) s_sum[0];
}

// ---- backward by scatter: the item of a bounce goes to the four texels of its footprint, CH floats each ----
// Lanes of a primary-ray wave are samples of one pixel: at the first vertex, and where the environment is seen
// directly, most of them share a footprint.  Adjacent lanes with the same (buffer, i0, j0) are summed first -- 4 CH segmented
// shuffle scans, one per texel and channel -- and the run's last lane issues the adds; a wave whose footprints are all distinct
// skips the scans (the test is one ballot).  P::value(adj, coef, g) forms the CH values of adj o coef.
template <int CH, class P>
struct FootprintScatter {
    static constexpr bool kReduces = false;
    const typename P::Args &T;
    F3 adj;
    __device__ __forceinline__ void begin(F3 a) { adj = a; }
    __device__ __forceinline__ void item(const tx::Item &it) {
        const unsigned long long on = __ballot(it.on);
        if (on == 0ull) return;                                           // (wave-uniform)
        float g[CH], v[4 * CH];
        P::value(adj, it.coef, g);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int c = 0; c < CH; ++c) v[CH * k + c] = g[c] * it.w[k];
        bool issue = it.on;
        const Runs r = make_runs(it.on, it.b, it.i0, it.j0);
        if (__ballot(r.tail) != on) {                                     // some footprint is shared: merge (wave-uniform branch)
#pragma unroll
            for (int q = 0; q < 4 * CH; ++q) v[q] = seg_sum(v[q], r.head);
            issue = r.tail;
        }
        if (!issue) return;
        float *p = T.buf[it.b];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float *t = p + CH * (int64_t) it.off[k];
#pragma unroll
            for (int c = 0; c < CH; ++c)
                if (adds_something(v[CH * k + c])) atomicAdd(t + c, v[CH * k + c]);     // (nearest: w[1..3] = 0, one texel's adds)
        }
    }
    __device__ __forceinline__ void item(const am::NoItem &) {}
    __device__ __forceinline__ void finish() {}
};

// ---- the host side of an entry point (workspace_ok, launch_checked: epsm_trace_launch.h) ----
// a reducing pass's backward kernel over `rows` workgroups, then the rows' sum into out[0 .. n_live)
template <int ROW, class Kernel, class Args>
int launch_reduced(const char *what, Kernel kernel, const Args &T, int64_t rows, int n_live, float *out, void *stream) {
    if (const int rc = launch_checked(what, kernel, rows, 128, stream, T)) return rc;
    return launch_checked(what, epsm_rows_sum_kernel<ROW>, n_live, 256, stream, (const float *) T.partial, rows, out);
}

}  // namespace epsm
