// epsm_trace_scan.h -- the integer scan and the stable radix sort the scene-construction units share (epsm_trace_bvh.hip,
// epsm_trace_scene.hip).  Everything is in an anonymous namespace: each unit gets its own copy of the kernels.
#ifndef EPSM_TRACE_SCAN_H
#define EPSM_TRACE_SCAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int kBlock = 256;              // scan, sort, per-element kernels
constexpr int kScanTile = 4 * kBlock;    // items per workgroup of the scan
constexpr int kRadixBits = 4;

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint64_t lanes_below() { return (uint64_t(1) << lane_id()) - 1; }

// ------------------------------------------------------------------------------------------------ exclusive scan (int32)
// Tile scan + recursive scan of the tile sums + add-back; `total` receives the sum of all n inputs.
__device__ int block_exclusive_scan(int v, int *lds /* kBlock / 64 + 1 */, int *total) {
    const int w = threadIdx.x >> 6;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o);
        if ((int) lane_id() >= o) incl += u;
    }
    if (lane_id() == 63) lds[w] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int i = 0; i < (int) (blockDim.x >> 6); ++i) { const int t = lds[i]; lds[i] = s; s += t; }
        lds[blockDim.x >> 6] = s;
    }
    __syncthreads();
    const int r = lds[w] + incl - v;
    *total = lds[blockDim.x >> 6];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kBlock) void scan_tiles(const int *in, int *out, int *sums, int n) {
    __shared__ int lds[kBlock / 64 + 1];
    const int64_t base = (int64_t) blockIdx.x * kScanTile + threadIdx.x * 4;
    int v[4], s = 0;
    for (int j = 0; j < 4; ++j) { v[j] = base + j < n ? in[base + j] : 0; s += v[j]; }
    int tot;
    int run = block_exclusive_scan(s, lds, &tot);
    for (int j = 0; j < 4; ++j) {
        if (base + j < n) out[base + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void scan_add(int *out, const int *sums, int n) {
    const int64_t i = (int64_t) blockIdx.x * kScanTile + threadIdx.x;
    const int add = sums[blockIdx.x];
    for (int j = 0; j < 4; ++j)
        if (i + j * kBlock < n) out[i + j * kBlock] += add;
}

__global__ void scan_total(const int *in, const int *out, int n, int *total) {
    *total = n > 0 ? out[n - 1] + in[n - 1] : 0;
}

int64_t scan_scratch_ints(int64_t n) {          // tile sums of every recursion level
    int64_t s = 0;
    for (int64_t m = (n + kScanTile - 1) / kScanTile; ; m = (m + kScanTile - 1) / kScanTile) {
        s += 2 * m + 1;
        if (m <= 1) break;
    }
    return s;
}

void scan_rec(const int *in, int *out, int n, int *scratch, hipStream_t st) {
    const int tiles = (n + kScanTile - 1) / kScanTile;
    int *sums = scratch, *ssum = scratch + tiles;
    hipLaunchKernelGGL(scan_tiles, dim3(tiles), dim3(kBlock), 0, st, in, out, sums, n);
    if (tiles > 1) {
        scan_rec(sums, ssum, tiles, scratch + 2 * tiles + 1, st);
        hipLaunchKernelGGL(scan_add, dim3(tiles), dim3(kBlock), 0, st, out, ssum, n);
    }
}

void exclusive_scan(const int *in, int *out, int n, int *total, int *scratch, hipStream_t st) {
    if (n > 0) scan_rec(in, out, n, scratch, st);
    hipLaunchKernelGGL(scan_total, dim3(1), dim3(1), 0, st, in, out, n, total);
}

// stable LSD radix sort of (key, id): per pass a digit histogram per tile (digit-major), an exclusive scan, a stable scatter
__global__ __launch_bounds__(kBlock) void radix_hist(const uint32_t *keys, int64_t T, int shift, int *hist, int tiles) {
    __shared__ int h[1 << kRadixBits];
    if (threadIdx.x < (1 << kRadixBits)) h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i < T) atomicAdd(&h[(keys[i] >> shift) & ((1 << kRadixBits) - 1)], 1);
    __syncthreads();
    if (threadIdx.x < (1 << kRadixBits)) hist[threadIdx.x * tiles + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void radix_scatter(const uint32_t *kin, const uint32_t *vin, uint32_t *kout, uint32_t *vout,
                                                        int64_t T, int shift, const int *offs, int tiles) {
    constexpr int R = 1 << kRadixBits;
    __shared__ int wh[kBlock / 64][R];
    const int w = threadIdx.x >> 6;
    for (int j = threadIdx.x; j < (kBlock / 64) * R; j += kBlock) (&wh[0][0])[j] = 0;
    __syncthreads();
    const int64_t i = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i < T;
    const uint32_t key = valid ? kin[i] : 0u;
    const unsigned digit = valid ? (key >> shift) & (R - 1) : R;          // R: matches no valid lane
    uint64_t peers = __ballot(1);
    for (int b = 0; b <= kRadixBits; ++b) {
        const uint64_t m = __ballot((digit >> b) & 1u);
        peers &= ((digit >> b) & 1u) ? m : ~m;
    }
    const int rank = __popcll(peers & lanes_below());
    if (valid && rank == 0) wh[w][digit] = __popcll(peers);
    __syncthreads();
    if (!valid) return;
    int off = offs[digit * tiles + blockIdx.x] + rank;
    for (int v = 0; v < w; ++v) off += wh[v][digit];
    kout[off] = key;
    vout[off] = vin[i];
}

}  // namespace

#endif
