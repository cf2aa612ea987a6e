// epsm_trace_rigid.hip -- rigid-motion reductions of the per-vertex gradient rows and their transpose (include/epsm_trace.h,
// epsm_rigid_reduce / epsm_rigid_expand).  A slot is a vertex range [lo, hi) and a pivot c; its twist is a translation and a
// rotation about c (world axes).  Reduce: force F = sum g_pos[v], torque T = sum (x_v - c) x g_pos[v] + n_v x g_nrm[v].  Expand:
// dx_v += dt + dw x (x_v - c), dn_v += dw x n_v.  Streaming kernels: 24 B (48 with normals) per vertex in, nothing to tile.
#include <stdint.h>

#include "epsm_common.h"
#include "epsm_trace_launch.h"

using epsm::launch_checked;
using epsm::workspace_ok;
using epsm_host::fail;

namespace {

constexpr int kChunk = 1024;           // vertices per workgroup of the first launch: 256 lanes x 4
constexpr int kRow = 6;                // [F, T]
constexpr int64_t kMaxWorkgroups = (int64_t) 1 << 23;

int64_t max_chunks_of(int64_t V) { return (V + kChunk - 1) / kChunk; }

struct Range { int64_t lo, hi; };

// a slot's range clipped to the buffer: the kernels never index outside [0, V) whatever the table holds
__device__ __forceinline__ Range slot_range(const int64_t *ranges, int slot, int64_t V) {
    int64_t lo = ranges[2 * slot], hi = ranges[2 * slot + 1];
    lo = lo < 0 ? 0 : (lo > V ? V : lo);
    hi = hi < lo ? lo : (hi > V ? V : hi);
    return {lo, hi};
}

// the sum of v over the 64 lanes of the wave, in every lane (a butterfly: the same order of additions in every launch)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// First launch: workgroup (chunk, slot) sums its 1024 vertices in float64 -- a lane its four, the wave by shuffles, the four waves
// in order -- and writes one row of six doubles.  Workgroups past the slot's last chunk write nothing (the second launch reads
// only the rows of the slot's own chunks).
__global__ __launch_bounds__(256) void epsm_rigid_partial_kernel(const float *positions, const float *normals, const float *g_pos,
                                                                 const float *g_nrm, int64_t V, const int64_t *ranges,
                                                                 const float *pivots, int64_t max_chunks, double *partial) {
    __shared__ double s_part[4][kRow];
    const int slot = blockIdx.y;
    const Range r = slot_range(ranges, slot, V);
    const int64_t first = r.lo + (int64_t) blockIdx.x * kChunk;
    if (first >= r.hi) return;                                         // (uniform over the workgroup)
    const double cx = pivots[3 * slot], cy = pivots[3 * slot + 1], cz = pivots[3 * slot + 2];
    double acc[kRow] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kChunk / 256; ++j) {
        const int64_t v = first + j * 256 + threadIdx.x;
        if (v >= r.hi) continue;
        const double gx = g_pos[3 * v], gy = g_pos[3 * v + 1], gz = g_pos[3 * v + 2];
        const double px = (double) positions[3 * v] - cx, py = (double) positions[3 * v + 1] - cy, pz = (double) positions[3 * v + 2] - cz;
        acc[0] += gx; acc[1] += gy; acc[2] += gz;
        double tx = py * gz - pz * gy, ty = pz * gx - px * gz, tz = px * gy - py * gx;
        if (g_nrm) {
            const double hx = g_nrm[3 * v], hy = g_nrm[3 * v + 1], hz = g_nrm[3 * v + 2];
            const double nx = normals[3 * v], ny = normals[3 * v + 1], nz = normals[3 * v + 2];
            tx += ny * hz - nz * hy; ty += nz * hx - nx * hz; tz += nx * hy - ny * hx;
        }
        acc[3] += tx; acc[4] += ty; acc[5] += tz;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < kRow; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) s_part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kRow)
        partial[((int64_t) slot * max_chunks + blockIdx.x) * kRow + threadIdx.x] =
            ((s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + s_part[2][threadIdx.x]) + s_part[3][threadIdx.x];
}

// Second launch, one wave per slot: lane t adds the slot's chunk rows t, t + 64, ... in order, the lanes by the butterfly, and the
// six sums are ADDED to out[slot] in float32.
__global__ __launch_bounds__(64) void epsm_rigid_sum_kernel(const double *partial, int64_t V, const int64_t *ranges, int64_t max_chunks,
                                                            float *out) {
    const int slot = blockIdx.x;
    const Range r = slot_range(ranges, slot, V);
    const int64_t chunks = (r.hi - r.lo + kChunk - 1) / kChunk;
    double acc[kRow] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t c = threadIdx.x; c < chunks; c += 64) {
        const double *row = partial + ((int64_t) slot * max_chunks + c) * kRow;
#pragma unroll
        for (int k = 0; k < kRow; ++k) acc[k] += row[k];
    }
#pragma unroll
    for (int k = 0; k < kRow; ++k) {
        const double s = wave_sum(acc[k]);
        if ((int) threadIdx.x == k) out[(int64_t) slot * kRow + k] += (float) s;
    }
}

// The transpose: one lane per vertex walks the slots in order (the ranges may overlap -- the sensor's slot covers every vertex --
// so no ordering of them would serve a search; the table is read wave-uniformly) and adds its motion under every twist that
// contains it.
__global__ __launch_bounds__(256) void epsm_rigid_expand_kernel(const float *positions, const float *normals, int64_t V,
                                                                const int64_t *ranges, const float *pivots, const float *twists,
                                                                int n_slots, float *d_pos, float *d_nrm) {
    const int64_t v = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const float x = positions[3 * v], y = positions[3 * v + 1], z = positions[3 * v + 2];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (d_nrm) { nx = normals[3 * v]; ny = normals[3 * v + 1]; nz = normals[3 * v + 2]; }
    float dx = 0.f, dy = 0.f, dz = 0.f, ex = 0.f, ey = 0.f, ez = 0.f;
    bool any = false;
    for (int s = 0; s < n_slots; ++s) {
        const Range r = slot_range(ranges, s, V);
        if (v < r.lo || v >= r.hi) continue;
        any = true;
        const float *tw = twists + (int64_t) s * kRow;
        const float wx = tw[3], wy = tw[4], wz = tw[5];
        const float px = x - pivots[3 * s], py = y - pivots[3 * s + 1], pz = z - pivots[3 * s + 2];
        dx += tw[0] + (wy * pz - wz * py); dy += tw[1] + (wz * px - wx * pz); dz += tw[2] + (wx * py - wy * px);
        ex += wy * nz - wz * ny; ey += wz * nx - wx * nz; ez += wx * ny - wy * nx;
    }
    if (!any) return;
    d_pos[3 * v] += dx; d_pos[3 * v + 1] += dy; d_pos[3 * v + 2] += dz;
    if (d_nrm) { d_nrm[3 * v] += ex; d_nrm[3 * v + 1] += ey; d_nrm[3 * v + 2] += ez; }
}

const char *slots_invalid(int64_t V, const int64_t *ranges, const float *pivots, int32_t n_slots) {
    if (V < 0 || V >= ((int64_t) 1 << 31)) return "V outside 0 .. 2^31 - 1";
    if (n_slots < 0 || n_slots > 65535) return "n_slots outside 0 .. 65535";
    if (n_slots > 0 && (!ranges || !pivots)) return "NULL ranges or pivots";
    // the first launch of the reduce is a (chunks of the buffer, slots) grid of 256 lanes: 2^31 threads at the most
    if ((int64_t) n_slots * max_chunks_of(V) > kMaxWorkgroups) return "n_slots * ceil(V / 1024) above 2^23";
    return nullptr;
}

}  // namespace

extern "C" size_t epsm_rigid_workspace_bytes(int64_t V, int32_t n_slots) {
    if (V <= 0 || n_slots <= 0) return 0;
    return (size_t) n_slots * (size_t) max_chunks_of(V) * kRow * sizeof(double);
}

extern "C" int epsm_rigid_reduce(const float *positions, const float *normals, const float *g_pos, const float *g_nrm, int64_t V,
                                 const int64_t *ranges, const float *pivots, int32_t n_slots, float *out, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_rigid_reduce";
    if (const char *why = slots_invalid(V, ranges, pivots, n_slots)) return fail(EPSM_EINVAL, what, why);
    if (n_slots > 0 && !out) return fail(EPSM_EINVAL, what, "NULL out");
    if (V > 0 && n_slots > 0 && (!positions || !g_pos)) return fail(EPSM_EINVAL, what, "NULL positions or g_pos");
    if (g_nrm && !normals) return fail(EPSM_EINVAL, what, "g_nrm without normals");
    if (V == 0 || n_slots == 0) return EPSM_OK;
    if (!workspace_ok(workspace, workspace_bytes, epsm_rigid_workspace_bytes(V, n_slots)))
        return fail(EPSM_EINVAL, what, "workspace NULL, misaligned or smaller than epsm_rigid_workspace_bytes(V, n_slots)");
    const int64_t mc = max_chunks_of(V);
    if (const int rc = launch_checked(what, epsm_rigid_partial_kernel, dim3((unsigned) mc, (unsigned) n_slots), 256, stream, positions,
                                      normals, g_pos, g_nrm, V, ranges, pivots, mc, (double *) workspace))
        return rc;
    return launch_checked(what, epsm_rigid_sum_kernel, n_slots, 64, stream, (const double *) workspace, V, ranges, mc, out);
}

extern "C" int epsm_rigid_expand(const float *positions, const float *normals, int64_t V, const int64_t *ranges, const float *pivots,
                                 const float *twists, int32_t n_slots, float *d_pos, float *d_nrm, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_rigid_expand";
    if (const char *why = slots_invalid(V, ranges, pivots, n_slots)) return fail(EPSM_EINVAL, what, why);
    if (n_slots > 0 && !twists) return fail(EPSM_EINVAL, what, "NULL twists");
    if (V > 0 && n_slots > 0 && (!positions || !d_pos)) return fail(EPSM_EINVAL, what, "NULL positions or d_pos");
    if (d_nrm && !normals) return fail(EPSM_EINVAL, what, "d_nrm without normals");
    if (V == 0 || n_slots == 0) return EPSM_OK;
    return launch_checked(what, epsm_rigid_expand_kernel, (V + 255) / 256, 256, stream, positions, normals, V, ranges, pivots, twists,
                          (int) n_slots, d_pos, d_nrm);
}
