// epsm_trace.hip -- the tracer's kernels + C ABI (include/epsm_trace.h): the one-launch form and the wavefront form with its stages.
#include <stdio.h>
#include <string.h>

#include "epsm_common.h"
#include "epsm_trace_launch.h"
#include "epsm_trace_replay.h"
#include "epsm_trace_wavefront.h"
#include "epsm_trace_packet.h"
#include "epsm_wave_scatter.h"           // wave_total_lane63 (DPP sums): the first-hit stage

using namespace epsm;
using epsm_host::fail;

namespace {

// four waves per SIMD: 128 registers and 56 B/lane of scratch instead of 151 registers and three waves:
// -11 % / -17 % at 128 k / 512 k triangles (five waves, 96 registers + 184 B of scratch: +5 % / -2 %)
__global__ __launch_bounds__(128, 4) void epsm_trace_kernel(TraceArgs A) {
    // traversal stacks: one LDS column of 32 entries per path (16 KB: four waves per SIMD); the four-wide tree may push
    // 3 x 16 references: the rare entries beyond 32 go to a private array (scratch)
    __shared__ uint32_t s_stack[kLaneStackLds * 128];
    uint32_t deep[kBvhStack - kLaneStackLds];
    const int64_t i = (int64_t) blockIdx.x * 128 + threadIdx.x;
    const BvhStack st = lane_stack(s_stack, deep, 128);
    // trace_one_path with the PRIMARY rays walked by the wave (epsm_trace_packet.h: the lanes of a wave are the samples of one
    // pixel or of a few neighbours); the packet's LDS column is entry 0 of the wave's own per-lane stacks, not yet in use
    const bool has = i < A.N;
    if (__ballot(has) == 0ull) return;
    PrimaryHit p = primary_hit(A, i, has, true, s_stack);
    if (!has) return;
    PathState &s = p.s;
    InlineVis vis{st};
    const int max_depth = path_max_depth(A);
    for (int iteration = 0; iteration < max_depth; ++iteration) {
        TriHit th; th.hit = false; th.tri = 0; th.t = kInf; th.u = th.v = 0.f;
        if (iteration == 0) th = p.th0;
        else if (s.active) th = intersect<false>(A.S, s.ray, st);
        path_bounce(A, i, iteration, s, th, vis);
    }
    path_end(A, i, s);
}

// ---- the wavefront form (epsm_trace_wavefront.h): queues of live paths, three small kernels per bounce ----
constexpr int kWfThreads = 128;                         // traversal kernels
constexpr int kWfMaxBlocks = 16384;
constexpr int kWfMaxChunkBlocks = 8192;                 // compaction: workgroups of 256, each takes chunks in turn

// Internal flag (never a caller's): under EPSM_TRACE_FUSE_FIRST_HIT the primary rays' stage retires most paths itself, and the few
// it leaves are COMPACTED into a queue before bounce 0's shade stage (a scan + compaction pass numbered bounce -1) -- slot q of bounce 0
// is then path queue[0][q] of counters[0], not path q of N.
constexpr uint32_t kWfPreCompact = 0x80000000u;
// The slots a stage walks: `count` of them, slot q holding path queue[q] -- or path q itself (queue NULL).
struct WfSlots {
    const uint32_t *queue;
    int64_t count;
    __device__ __forceinline__ int64_t path(int64_t q) const { return queue ? (int64_t) queue[q] : q; }
};
// the paths alive into bounce b (bounce 0 and the pass numbered -1: every path, unless the survivors were compacted before bounce 0)
__device__ __forceinline__ WfSlots wf_alive_slots(const TraceArgs &A, const WfState &W, int b) {
    const bool identity = b < 0 || (b == 0 && !(A.flags & kWfPreCompact));
    return identity ? WfSlots{nullptr, A.N} : WfSlots{W.queue[b & 1], (int64_t) W.counters[wf_alive_counter(b)]};
}
__device__ __forceinline__ WfSlots wf_shadow_slots(const WfState &W, int b) { return WfSlots{W.shadow_queue, (int64_t) W.counters[wf_shadow_counter(b)]}; }
// every slot, grid-stride over workgroups of THREADS: body(path)
template <int THREADS, class Body>
__device__ __forceinline__ void wf_for_each_slot(const WfSlots &Q, Body body) {
    for (int64_t q = (int64_t) blockIdx.x * THREADS + threadIdx.x; q < Q.count; q += (int64_t) gridDim.x * THREADS) body(Q.path(q));
}
// Traversal kernels: 8 KB of LDS stacks per workgroup; extend 62 registers, shadow 67: 8 and 7 waves per SIMD.
// (Tried and dropped: persistent waves whose idle lanes fetch new rays between two traversal rounds -- from a shared
// queue head the ~10^5 same-address atomics serialise, from a static share per wave the primary rays lose their
// coherence: 667 -> 1226 us for bounce 0, -5..10 % for the later bounces, +1.1 ms per 4.2 M paths in all.
// And: ONE loop whose every turn runs one kind of step -- a node step or a triangle test -- chosen by majority among
// the unfinished lanes (the while-while loops run for the slowest lane: 27 % of the VALU lanes busy).  Same hits;
// 5.6-5.7 ms against 5.3-5.4 ms at 128 k triangles, 8.7 against 8.9 ms at 512 k: the step-wise traversal state
// (leaf cursor kept across turns) costs the while-while form 5-7 % where both share it, so it was not kept.)
// The closest hits of the bounces >= 1 (the primary rays are the packet kernel's, below).
__global__ __launch_bounds__(kWfThreads) void epsm_wf_extend_kernel(TraceArgs A, WfState W, int b) {
    __shared__ uint32_t s_stack[kWfStackLds * kWfThreads];
    const WfSlots Q = wf_alive_slots(A, W, b);
    if (wf_in_tail(A, b, Q.count)) return;
    // (a literal 1 for "a later bounce": with b the compiler keeps bounce 0's ray derivation in this kernel)
    wf_for_each_slot<kWfThreads>(Q, [&](int64_t i) { wf_extend(A, W, i, s_stack + threadIdx.x, kWfThreads, 1); });
}
// ---- the first-hit stage (EPSM_TRACE_FUSE_FIRST_HIT): wave_sum, first_hit_add, first_hit_scatter and the kernel that finishes it ----
// What the lanes of a wave -- at bounce 0 the samples of one pixel or of a few neighbouring ones -- give the
// backward pass: every path's grad_d into the wave's share of -sum grad_d, and the first-vertex rows of the paths retired at their
// first hit.  Lanes on the same triangle are summed first (butterfly over the wave, in up to four turns of "the first lane still
// owing and everybody on its triangle"), one lane adds the sum; what is left after four turns adds for itself.
// sum over the wave by six DPP adds (epsm_wave_scatter.h: the total lands in lane 63) + one readlane: no trip through the LDS crossbar
__device__ __forceinline__ float wave_sum(float v) { return lane63(wave_total_lane63(v)); }
__device__ __forceinline__ void first_hit_add(float *p, float v) { if (first_hit_addend_kept(v)) atomicAdd(p, v); }
__device__ __forceinline__ void first_hit_scatter(const TraceArgs &A, const WfState &W, const WfFirstHit &fh, unsigned wave_index) {
    const int lane = threadIdx.x & 63;
    if (A.fh.grad_o_sum) {
        // epsm.py:258-261: d / d ray.o = -sum grad_d.  One triple per WAVE on the three words themselves was 2 ms per 2^24 paths
        // (262 144 same-address float atomics retire one at a time); the waves add to one of 256 slots of the workspace, which
        // epsm_wf_first_hit_finish_kernel sums into the caller's three words.
        const float sx = wave_sum(fh.gd.x), sy = wave_sum(fh.gd.y), sz = wave_sum(fh.gd.z);
        if (lane < 3) first_hit_add(W.fh_partial + 4 * (wave_index % kWfFirstHitSlots) + lane,
                                    lane == 0 ? sx : lane == 1 ? sy : sz);
    }
    bool owing = fh.rows.on;
#pragma unroll 1
    for (int turn = 0; turn < 4; ++turn) {
        const unsigned long long m = __ballot(owing);
        if (m == 0ull) return;
        const int leader = __ffsll((long long) m) - 1;
        const uint32_t k0 = (uint32_t) __shfl((int) fh.rows.key[0], leader), k1 = (uint32_t) __shfl((int) fh.rows.key[1], leader),
                       k2 = (uint32_t) __shfl((int) fh.rows.key[2], leader);
        const bool mine = owing && fh.rows.key[0] == k0 && fh.rows.key[1] == k1 && fh.rows.key[2] == k2;
        float v[9];
#pragma unroll
        for (int j = 0; j < 3; ++j) { v[3 * j] = mine ? fh.rows.val[j].x : 0.f; v[3 * j + 1] = mine ? fh.rows.val[j].y : 0.f; v[3 * j + 2] = mine ? fh.rows.val[j].z : 0.f; }
#pragma unroll
        for (int c = 0; c < 9; ++c) v[c] = wave_sum(v[c]);
        // lanes 0..8 add one component each: x, y, z of a row side by side -> one atomic request per row
        if (lane < 9) {
            const int j = lane / 3, c = lane - 3 * j;
            const uint32_t row = j == 0 ? k0 : j == 1 ? k1 : k2;
            float val = v[0];
#pragma unroll
            for (int e = 1; e < 9; ++e) val = lane == e ? v[e] : val;
            first_hit_add(A.fh.grad_pos + 3 * (int64_t) row + c, val);
        }
        if (mine) owing = false;
    }
    if (owing) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float *p = A.fh.grad_pos + 3 * (int64_t) fh.rows.key[j];
            first_hit_add(p, fh.rows.val[j].x); first_hit_add(p + 1, fh.rows.val[j].y); first_hit_add(p + 2, fh.rows.val[j].z);
        }
    }
}
__global__ __launch_bounds__(kWfFirstHitSlots) void epsm_wf_first_hit_finish_kernel(TraceArgs A, WfState W) {
    __shared__ float s_sum[kWfFirstHitSlots / 64][3];
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = wave_sum(W.fh_partial[4 * threadIdx.x + c]);
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6][0] = v[0]; s_sum[threadIdx.x >> 6][1] = v[1]; s_sum[threadIdx.x >> 6][2] = v[2]; }
    __syncthreads();
    if (threadIdx.x < 3) {
        float t = 0.f;
        for (int w = 0; w < kWfFirstHitSlots / 64; ++w) t += s_sum[w][threadIdx.x];
        first_hit_add(A.fh.grad_o_sum + threadIdx.x, -t);
    }
}
// ---- (end of the first-hit stage) ----

// The closest hits of the PRIMARY rays, with the wave as the unit (epsm_trace_packet.h): a wave is the samples of one pixel or of a
// few neighbours.  Every path, whatever is compacted behind this stage.
__global__ __launch_bounds__(kWfThreads) void epsm_wf_extend_packet_kernel(TraceArgs A, WfState W) {
    __shared__ uint32_t s_stack[kPacketStack * (kWfThreads / 64)];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int64_t q0 = (int64_t) blockIdx.x * kWfThreads + wv * 64; q0 < A.N; q0 += (int64_t) gridDim.x * kWfThreads) {     // wave-uniform
        const int64_t q = q0 + lane;
        const bool has = q < A.N;
        const int64_t i = has ? q : q0;
        // EPSM_TRACE_FUSE_FIRST_HIT: the primary rays' stage has ray and hit in registers -- it retires the paths the rule retires at
        // their first vertex itself (first_hit_retires / first_hit_rows: the backward pass of a path without a chain, every path's
        // share of d / d ray.o) and marks their slots; the shade stage passes them by: of 2^24 paths of the clutter scene it shades 2 M.
        const bool fuse = (A.flags & EPSM_TRACE_FUSE_FIRST_HIT) != 0;          // (kernel-uniform)
        WfFirstHit fh = wf_no_first_hit();
        PrimaryRay pr;
        const Ray r = path_begin(A, i, false, &pr).ray;
        if (fuse && has) {
            float gx, gy;
            first_hit_pixel_grad(A, i, gx, gy);
            fh.gd = (pr.dx - pr.ray.d) * gx + (pr.dy - pr.ray.d) * gy;         // epsm.py:255, as tangent_from forms it
        }
        const TriHit th = packet_intersect(A.S, r, has, s_stack + wv * kPacketStack);
        bool done = false;
        if (fuse) {
            if (has) {
                uint32_t w;
                SurfHit lite;
                if (first_hit_retires(A, th, w, lite)) {
                    fh.rows = first_hit_rows(A, w, lite, r, fh.gd);
                    A.rec[0].pflags[i] = 0u;                             // no vertex: the backward kernel gives this path no lane
                    done = true;
                }
                W.flags[q] = done ? (uint8_t) 0 : kWfAlive;              // (the pass numbered bounce -1 compacts the survivors)
            }
            first_hit_scatter(A, W, fh, (unsigned) (q0 >> 6));           // (all lanes of the wave: the sums run over it)
            const unsigned long long ma = __ballot(has && !done);
            if (lane == 0 && ma != 0ull) {                               // the survivors of this quarter of a chunk, for the scan
                const int64_t chunk = q0 / kWfChunk;
                atomicAdd(&W.chunk_counts[chunk], (uint32_t) __popcll(ma));
                atomicAdd(&W.group_counts[chunk / kWfGroup], (uint32_t) __popcll(ma));
            }
        }
        if (has && !done) W.hit[i] = wf_hit_pack(th);
    }
}
// The rest of the loop of the paths alive into bounce b, once they are few (wf_tail, epsm_trace_wavefront.h).
__global__ __launch_bounds__(kWfThreads) void epsm_wf_tail_kernel(TraceArgs A, WfState W, int b) {
    __shared__ uint32_t s_stack[kWfStackLds * kWfThreads];
    const WfSlots Q = wf_alive_slots(A, W, b);
    if (!wf_in_tail(A, b, Q.count)) return;
    wf_for_each_slot<kWfThreads>(Q, [&](int64_t i) { wf_tail(A, W, i, b, s_stack + threadIdx.x, kWfThreads); });
}
// Every 256-slot chunk of `count` slots, the workgroups (of kWfChunk lanes) taking chunks in turn: flags(chunk, q) gives slot q's
// bits (kWfAlive | kWfShadow); the number of each among a wave's slots is left in LDS, n[which][wave], and then
// use(chunk, f, m, n) runs -- f the lane's bits, m the two ballots of its wave.
template <class Flags, class Use>
__device__ __forceinline__ void wf_for_each_chunk(int64_t count, Flags flags, Use use) {
    __shared__ uint32_t s_n[2][kWfChunk / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll 1
    for (int64_t chunk = blockIdx.x; chunk * kWfChunk < count; chunk += gridDim.x) {           // workgroup-uniform
        const uint8_t f = flags(chunk, chunk * kWfChunk + threadIdx.x);
        const unsigned long long m[2] = {__ballot((f & kWfAlive) != 0), __ballot((f & kWfShadow) != 0)};
        if (lane == 0) { s_n[0][wv] = (uint32_t) __popcll(m[0]); s_n[1][wv] = (uint32_t) __popcll(m[1]); }
        __syncthreads();
        use(chunk, f, m, s_n);
        __syncthreads();                                             // (the counts of this chunk are read before the next one writes its own)
    }
}
// (160 registers, 3 waves per SIMD; capped at 128 for 4 waves it spills 96 B/lane and is no faster.)
// One 256-slot chunk of the queue per workgroup.  Appending the survivors to the next queue with one atomic per
// wave on the queue's counter made this kernel 1.23 ms at 4.2 M paths whatever it computed (knock-outs: the log
// writes cost nothing, each of the two queues 0.6 ms: 65 536 same-address atomics, ~9 ns apiece at the memory
// side); it leaves a flag per slot and two counts per chunk instead.
__global__ __launch_bounds__(kWfChunk) void epsm_wf_shade_kernel(TraceArgs A, WfState W, int b) {
    const WfSlots Q = wf_alive_slots(A, W, b);
    if (wf_in_tail(A, b, Q.count)) return;
    // (A capped grid whose workgroups take chunks in turn, as the compaction does: the launch of a bounce nobody reaches 15 -> 5 us, but
    // a stage whose every chunk has work 1.08 -> 1.19 ms at 2^24 paths -- the hardware's dispatch order balances better.  So the
    // host caps the grid only where the queue is known to be short: behind the first-hit stage's compaction and from bounce 1 on.)
    // EPSM_TRACE_FUSE_FIRST_HIT: the primary rays' stage (packet kernel) has dealt with the paths that end at their first vertex and
    // the survivors come here compacted (kWfPreCompact); without that stage (the host harness) this one does it, wf_shade's `out`
    const bool fuse = b == 0 && (A.flags & EPSM_TRACE_FUSE_FIRST_HIT) && !(A.flags & kWfPreCompact);     // (kernel-uniform)
    wf_for_each_chunk(Q.count,
        [&](int64_t chunk, int64_t q) {
            bool alive = false, shadow = false;
            WfFirstHit fh = wf_no_first_hit();
            if (q < Q.count) {
                wf_shade(A, W, Q.path(q), b, alive, shadow, fuse ? &fh : nullptr);
                W.flags[q] = (uint8_t) ((alive ? kWfAlive : 0) | (shadow ? kWfShadow : 0));
            }
            if (fuse) first_hit_scatter(A, W, fh, (unsigned) chunk * (kWfChunk / 64) + (threadIdx.x >> 6));   // (all lanes of the wave: the sums run over it)
            return (uint8_t) ((alive ? kWfAlive : 0) | (shadow ? kWfShadow : 0));
        },
        [&](int64_t chunk, uint8_t, const unsigned long long *, const uint32_t (&n_wave)[2][kWfChunk / 64]) {
            if (threadIdx.x >= 2) return;
            uint32_t n = 0;
#pragma unroll
            for (int w = 0; w < kWfChunk / 64; ++w) n += n_wave[threadIdx.x][w];
            W.chunk_counts[threadIdx.x * W.chunks + chunk] = n;
            if (n) atomicAdd(&W.group_counts[threadIdx.x * W.groups + chunk / kWfGroup], n);     // (64 adds per address at most)
        });
}
// Exclusive scan of the chunk counts of both queues (<= 65 536 chunks each at 2^24 paths), one workgroup PER QUEUE, two
// levels: the counts of the GROUPS of 64 chunks (summed by the shade stage) are scanned over the workgroup -- one coalesced
// load per thread at 2^24 paths --, then every wave takes groups in turn: one count per lane, a wave scan, the group's offset
// added.  Publishes the queue length of the next stage and leaves the group counts zeroed for the next bounce.
// (One level -- thread t sums a strip of 64 counts, the strips' sums are scanned, the strip is rewritten -- took 100 us for
// the first bounce of a 2^24-path tile: two passes of strided, dependent loads by two workgroups.)
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t t = (uint32_t) __shfl_up((int) v, off); if (lane >= off) v += t; }
    return v;
}
__global__ __launch_bounds__(1024) void epsm_wf_scan_kernel(TraceArgs A, WfState W, int b) {
    const int64_t count = wf_alive_slots(A, W, b).count, n = (count + kWfChunk - 1) / kWfChunk, groups = (n + kWfGroup - 1) / kWfGroup;
    if (wf_in_tail(A, b, count)) return;                          // (the counters of the later bounces stay 0: their stages leave at once)
    __shared__ uint32_t s_w[16];
    __shared__ uint32_t s_carry;
    const int which = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *c = W.chunk_counts + which * W.chunks, *gc = W.group_counts + which * W.groups, *go = W.group_offsets + which * W.groups;
    if (threadIdx.x == 0) s_carry = 0u;
    __syncthreads();
    for (int64_t base = 0; base < groups; base += 1024) {         // (one turn up to 2^24 paths)
        const int64_t g = base + threadIdx.x;
        const uint32_t v = g < groups ? gc[g] : 0u;
        if (g < groups) gc[g] = 0u;
        const uint32_t inc = wave_inclusive_scan(v);
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        uint32_t before = s_carry, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const uint32_t t = s_w[w]; if (w < wv) before += t; all += t; }
        if (g < groups) go[g] = before + inc - v;
        __syncthreads();
        if (threadIdx.x == 0) s_carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) W.counters[which == 0 ? wf_alive_counter(b + 1) : wf_shadow_counter(b)] = s_carry;
    if (threadIdx.x == 0 && b < 0 && which == 0 && A.fh.survivor_count) *A.fh.survivor_count = s_carry;   // (the caller's copy: EpsmFirstHitBackward)
    constexpr int kBatch = 4;                                     // groups a wave has in flight
    for (int64_t g0 = (int64_t) wv * kBatch; g0 < groups; g0 += 16 * kBatch) {
        uint32_t v[kBatch], o[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int64_t k = (g0 + j) * kWfGroup + lane;
            v[j] = (g0 + j < groups && k < n) ? c[k] : 0u;
            o[j] = g0 + j < groups ? go[g0 + j] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const uint32_t inc = wave_inclusive_scan(v[j]);
            const int64_t k = (g0 + j) * kWfGroup + lane;
            if (g0 + j < groups && k < n) c[k] = o[j] + inc - v[j];
        }
    }
}
// Writes the queue of bounce b + 1 and the shadow queue of bounce b, in path order (stable).
// (Tried: grouping the survivors of a chunk by the octant of their new direction, 8-bucket counting sort in LDS --
// 4.95 -> 5.85 ms at 128 k triangles, 8.1 -> 9.3 ms at 512 k: path order keeps the samples of a pixel, which start
// from almost the same point, next to each other, and that is worth more than a shared direction octant.)
// (And in round 4: inside its 256-slot chunk, grouped by the triangle the rays LEAVE -- the pixel neighbourhood kept -- slower
// again, the shade stage's reads lose their coalescing: MEASUREMENTS.md 9.3, profiles/r04_j_tracer_rekey.txt.  Removed.)
__global__ __launch_bounds__(kWfChunk) void epsm_wf_compact_kernel(TraceArgs A, WfState W, int b) {
    const WfSlots Q = wf_alive_slots(A, W, b);
    if (wf_in_tail(A, b, Q.count)) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t i = 0u;                                                 // the slot's path, read beside its flag
    wf_for_each_chunk(Q.count,
        [&](int64_t, int64_t q) {
            i = q < Q.count ? (uint32_t) Q.path(q) : 0u;
            return q < Q.count ? W.flags[q] : (uint8_t) 0;
        },
        [&](int64_t chunk, uint8_t f, const unsigned long long *m, const uint32_t (&n_wave)[2][kWfChunk / 64]) {
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                if (!((f >> which) & 1)) continue;
                uint32_t off = W.chunk_counts[which * W.chunks + chunk];
                for (int w = 0; w < wv; ++w) off += n_wave[which][w];
                off += (uint32_t) __popcll(m[which] & ((1ull << lane) - 1ull));
                (which == 0 ? W.queue[(b + 1) & 1] : W.shadow_queue)[off] = i;
                if (b < 0 && which == 0 && A.fh.survivors) A.fh.survivors[off] = i;      // (the caller's copy: EpsmFirstHitBackward)
            }
        });
}
__global__ __launch_bounds__(kWfThreads) void epsm_wf_shadow_kernel(TraceArgs A, WfState W, int b) {
    __shared__ uint32_t s_stack[kWfStackLds * kWfThreads];
    wf_for_each_slot<kWfThreads>(wf_shadow_slots(W, b), [&](int64_t i) { wf_shadow(A, W, i, b, s_stack + threadIdx.x, kWfThreads); });
}
__global__ __launch_bounds__(256) void epsm_wf_finish_kernel(TraceArgs A, WfState W) {
    wf_for_each_slot<256>(WfSlots{nullptr, A.N}, [&](int64_t i) { wf_finish(A, W, i); });
}

}  // namespace

extern "C" int epsm_trace_paths(const EpsmScene *scene, const EpsmSensor *sensor,
                                uint32_t seed, int spp, int max_depth, int rr_depth,
                                int64_t path_offset, int64_t N, int K_log,
                                float *ray_o, float *ray_d, float *ray_dx, float *ray_dy,
                                float *film_pos, float *radiance, uint8_t *valid,
                                const EpsmRecordOut *recs, uint32_t flags, void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (scene && sensor && N == 0) return EPSM_OK;
    TraceArgs A;
    if (flags & EPSM_TRACE_FUSE_FIRST_HIT) return fail(EPSM_EINVAL, "epsm_trace_paths: EPSM_TRACE_FUSE_FIRST_HIT is the wavefront form's (epsm_trace_paths_wavefront)");
    if (const char *why = trace_args_fill(A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, K_log, ray_o, ray_d, ray_dx, ray_dy,
                                          film_pos, radiance, valid, recs, flags))
        return fail(EPSM_EINVAL, "epsm_trace_paths", why);
    return launch_checked("epsm_trace_paths", epsm_trace_kernel, (N + 127) / 128, 128, stream, A);
}

extern "C" int epsm_trace_paths_color(const EpsmScene *scene, const EpsmSensor *sensor,
                                      uint32_t seed, int spp, int max_depth, int rr_depth,
                                      int64_t path_offset, int64_t N,
                                      float *film_pos, float *radiance, uint8_t *valid,
                                      float *color_sum, int n_color, void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (scene && sensor && N == 0) return EPSM_OK;
    if (!color_sum || n_color < 1 || n_color > 4 || !radiance)
        return fail(EPSM_EINVAL, "epsm_trace_paths_color: need color_sum, radiance and 1 <= n_color <= 4");
    TraceArgs A;
    static float dummy_rays[12];                               // (the rays are not wanted: trace_args_fill only checks for NULL)
    if (const char *why = trace_args_fill(A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, 0, dummy_rays, dummy_rays,
                                          dummy_rays, dummy_rays, film_pos, radiance, valid, nullptr, 0))
        return fail(EPSM_EINVAL, "epsm_trace_paths_color", why);
    A.ray_o = A.ray_d = A.ray_dx = A.ray_dy = nullptr;
    A.color_sum = color_sum; A.n_color = n_color;
    const hipError_t e = hipMemsetAsync(color_sum, 0, (size_t) N * n_color * 3 * sizeof(float), (hipStream_t) stream);
    if (e != hipSuccess) return epsm_host::hip_fail("epsm_trace_paths_color", e);
    return launch_checked("epsm_trace_paths_color", epsm_trace_kernel, (N + 127) / 128, 128, stream, A);
}

extern "C" size_t epsm_trace_workspace_bytes(int64_t N) { return N > 0 ? wf_workspace_bytes(N) : 0; }

extern "C" int epsm_trace_paths_wavefront(const EpsmScene *scene, const EpsmSensor *sensor,
                                          uint32_t seed, int spp, int max_depth, int rr_depth,
                                          int64_t path_offset, int64_t N, int K_log,
                                          float *ray_o, float *ray_d, float *ray_dx, float *ray_dy,
                                          float *film_pos, float *radiance, uint8_t *valid,
                                          const EpsmRecordOut *recs, uint32_t flags, void *workspace, size_t workspace_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (scene && sensor && N == 0) return EPSM_OK;
    TraceArgs A;
    if (const char *why = trace_args_fill(A, scene, sensor, seed, spp, max_depth, rr_depth, path_offset, N, K_log, ray_o, ray_d, ray_dx, ray_dy,
                                          film_pos, radiance, valid, recs, flags))
        return fail(EPSM_EINVAL, "epsm_trace_paths_wavefront", why);
    if (!workspace || (((uintptr_t) workspace) & 15) || workspace_bytes < wf_workspace_bytes(N))
        return fail(EPSM_EINVAL, "epsm_trace_paths_wavefront: workspace NULL, not 16-byte aligned or smaller than epsm_trace_workspace_bytes(N)");
    if (N > 0xFFFFFFF0LL) return fail(EPSM_EINVAL, "epsm_trace_paths_wavefront: N must fit the 32-bit queues");
    hipStream_t s = (hipStream_t) stream;
    const WfState W = wf_carve(workspace, N);
    hipError_t e = hipMemsetAsync(W.counters, 0, wf_zeroed_bytes(N), s);          // the counters and the group counts behind them
    if (e != hipSuccess) return epsm_host::hip_fail("epsm_trace_paths_wavefront", e);
    if (A.flags & EPSM_TRACE_FUSE_FIRST_HIT) {
        A.flags |= kWfPreCompact;                                                  // (the packet stage ADDS its survivors to the chunk counts)
        e = hipMemsetAsync(W.chunk_counts, 0, (size_t) W.chunks * 8, s);
        if (e != hipSuccess) return epsm_host::hip_fail("epsm_trace_paths_wavefront", e);
    }
    // a stage: `kernel` over `grid` workgroups of `threads`, on (A, W) and what else it takes (the bounce)
    auto stage = [&](auto kernel, int64_t grid, int threads, auto... more) {
        hipLaunchKernelGGL(kernel, dim3((unsigned) grid), dim3((unsigned) threads), 0, s, A, W, more...);
    };
    auto at_most = [](int64_t n, int64_t cap) { return n < cap ? n : cap; };
    auto blocks = [&](int threads) { return at_most((N + threads - 1) / threads, kWfMaxBlocks); };
    const int depth = path_max_depth(A);
    const int64_t shade_short = at_most(W.chunks, 16384), chunk_blocks = at_most(W.chunks, kWfMaxChunkBlocks);
    const int64_t tail_blocks = (at_most(N, kWfTailBelow) + kWfThreads - 1) / kWfThreads;
    for (int b = 0; b < depth; ++b) {
        // the queue lengths of bounce b live on the device: every stage is launched for the worst case and its
        // surplus workgroups leave at once (no host round trip between the bounces)
        // (bounces >= 1: the tail first -- it runs once, when the queue has become short, and the stages behind it leave at once)
        if (b >= 1 && !(A.flags & EPSM_TRACE_NO_TAIL)) stage(epsm_wf_tail_kernel, tail_blocks, kWfThreads, b);
        if (b == 0) {
            stage(epsm_wf_extend_packet_kernel, blocks(kWfThreads), kWfThreads);
            if (A.flags & kWfPreCompact) {                       // the survivors of the primary rays' stage, compacted: "bounce -1"
                stage(epsm_wf_scan_kernel, 2, 1024, -1);
                stage(epsm_wf_compact_kernel, chunk_blocks, kWfChunk, -1);
            }
        }
        else stage(epsm_wf_extend_kernel, blocks(kWfThreads), kWfThreads, b);
        // (the whole grid where every chunk has work -- bounce 0 of an unfused trace --, a capped one where the queue is short)
        stage(epsm_wf_shade_kernel, (b == 0 && !(A.flags & kWfPreCompact)) ? W.chunks : shade_short, kWfChunk, b);
        if (b == 0 && (A.flags & EPSM_TRACE_FUSE_FIRST_HIT) && A.fh.grad_o_sum) stage(epsm_wf_first_hit_finish_kernel, 1, kWfFirstHitSlots);
        stage(epsm_wf_scan_kernel, 2, 1024, b);
        stage(epsm_wf_compact_kernel, chunk_blocks, kWfChunk, b);
        stage(epsm_wf_shadow_kernel, blocks(kWfThreads), kWfThreads, b);
    }
    // (radiance / valid not asked for and the native log: nothing is left to write -- the gradient-only trace of render_backward)
    if (A.radiance || A.valid || !(A.flags & EPSM_TRACE_PACKED_LOG)) stage(epsm_wf_finish_kernel, blocks(256), 256);
    e = hipGetLastError();
    if (e != hipSuccess) return epsm_host::hip_fail("epsm_trace_paths_wavefront", e);
    return EPSM_OK;
}
