// epsm_trace_smooth.hip -- large-steps vertex updates (include/epsm_trace.h: epsm_mesh_laplacian, epsm_laplacian_apply,
// epsm_laplacian_solve): A = I + lambda L of a mesh, L its unique-edge combinatorial Laplacian, and conjugate gradients on A.
//   table     from the vertex -> corner adjacency (epsm_trace_topology.h): per vertex two candidate neighbours per corner, the
//             first occurrence of each kept at the front of the row, the rest 0xFFFFFFFF; the row's degree; the maximum degree;
//   apply     one lane per vertex: y_v = x_v + lambda (deg_v x_v - sum_w x_w) in float64, table order, rounded once;
//   solve     CG, three columns per gather.  GRID: two launches per iteration, chunks of 1024 vertices; a launch's dot product is
//             one row of doubles per chunk and the LAST workgroup to arrive (an integer counter; nobody waits) adds the rows in
//             chunk order and writes the column scalars the next launch reads.  ONE_GROUP: one workgroup of 1024 lanes runs the
//             whole solve, the search direction in LDS, a lane's rows in registers.
// Every sum runs in a fixed order (a lane's rows, the wave by a butterfly, the waves in order, the chunks in order): two calls on
// the same input give identical bits.  Nothing synchronises with the host and nothing allocates.
#include <math.h>
#include <stdint.h>

#include "epsm_common.h"
#include "epsm_trace_launch.h"
#include "epsm_trace_topology.h"

using epsm::launch_checked;
using epsm::table_align_up;
using epsm::workspace_ok;
using epsm_host::fail;

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 1024;                           // vertices per workgroup of the GRID form: 256 lanes x 4
constexpr int kOneThreads = 1024;                      // the ONE_GROUP form's workgroup
constexpr int kOneMaxRows = EPSM_SMOOTH_ONE_GROUP_MAX_V / kOneThreads;
constexpr int kOneRowsInRegisters = 4;                 // up to here x stays in registers too: 126 of the 128 VGPRs a lane of 1024 has
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int64_t kMaxTriangles = int64_t(1) << 28;    // the topology's own limits
constexpr int64_t kMaxVertices = int64_t(1) << 31;
constexpr int kMaxIters = 1 << 16;                     // the GRID form queues two launches per iteration up front

// The crossover of EPSM_SMOOTH_AUTO: ONE_GROUP up to this V, GRID above (MEASUREMENTS 33: at lambda = 19 the two curves meet at
// 7168 vertices, seven rows per lane -- 2.21 against 2.26 ms -- and ONE_GROUP is 1.4 times slower at 8192).
constexpr int64_t kAutoOneGroupMaxV = 7168;

static_assert(kOneMaxRows * kOneThreads == EPSM_SMOOTH_ONE_GROUP_MAX_V, "whole rows of the workgroup");
static_assert(12 * EPSM_SMOOTH_ONE_GROUP_MAX_V + 768 <= 160 * 1024, "the search direction and the reduction rows fit the LDS");

int64_t chunks_of(int64_t V) { return (V + kChunk - 1) / kChunk; }

// ------------------------------------------------------------------------------------------------ the table
// head (64 words: [0] maximum degree, [1] V), row (V + 1: the topology's corner offsets; a row's candidates start at 2 row[v]),
// deg (V), nbr (6 T)
struct Table { uint32_t *head, *row, *deg, *nbr; };

size_t table_carve(int64_t V, int64_t T, char *base, Table *t) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + o : nullptr; o += table_align_up(bytes); return (uint32_t *) p; };
    Table x;
    x.head = take(256);
    x.row = take(4 * (size_t) (V + 1));
    x.deg = take(4 * (size_t) V);
    x.nbr = take(24 * (size_t) T);
    if (t) *t = x;
    return o;
}
// (apply and solve know V only: nbr follows deg whatever T is)
Table table_of(int64_t V, const void *laplacian) {
    Table t;
    table_carve(V, 1, (char *) laplacian, &t);
    return t;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One lane per vertex: the row of v.  Its corners come in triangle order; each names the triangle's other two vertices.
__global__ __launch_bounds__(kBlock) void laplacian_rows_kernel(const uint32_t *tri, int64_t V, int64_t T, const uint32_t *top_row,
                                                                const uint32_t *top_adj, Table t) {
    const int64_t v = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    const uint32_t E = (uint32_t) (3 * T);
    uint32_t kept = 0;
    if (v < V) {
        uint32_t lo = top_row[v], hi = top_row[v + 1];                  // clipped: never a slot outside the table
        lo = lo > E ? E : lo;
        hi = hi < lo ? lo : (hi > E ? E : hi);
        uint32_t *out = t.nbr + 2 * (int64_t) lo;
        for (uint32_t e = lo; e < hi; ++e) {
            const uint32_t corner = top_adj[e];
            if (corner >= E) continue;
            const uint32_t tr = corner / 3, c = corner - 3 * tr;
#pragma unroll
            for (int s = 1; s <= 2; ++s) {
                const uint32_t w = tri[3 * (int64_t) tr + (c + s) % 3];
                bool keep = w < V && w != (uint32_t) v;
                for (uint32_t j = 0; keep && j < kept; ++j) keep = out[j] != w;
                if (keep) out[kept++] = w;
            }
        }
        for (uint32_t j = kept; j < 2 * (hi - lo); ++j) out[j] = kNone;
        t.row[v] = lo;
        t.deg[v] = kept;
        if (v == V - 1) t.row[V] = hi;
        if (v == 0) t.head[1] = (uint32_t) V;
    }
    uint32_t m = kept;                                                  // an integer maximum: any order gives the same word
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(m, o, 64); m = u > m ? u : m; }
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(t.head, m);
}

// (A p)_v in float64 from load(w, float[3]): the neighbours in table order, then the diagonal
template <class Load>
__device__ __forceinline__ void row_product(const Table &t, int64_t v, double lambda, Load load, double y[3]) {
    const uint32_t deg = t.deg[v];
    const uint32_t *nb = t.nbr + 2 * (int64_t) t.row[v];
    double s[3] = {0.0, 0.0, 0.0};
    float a[3];
    for (uint32_t j = 0; j < deg; ++j) {
        load(nb[j], a);
        s[0] += a[0]; s[1] += a[1]; s[2] += a[2];
    }
    load((uint32_t) v, a);
#pragma unroll
    for (int c = 0; c < 3; ++c) y[c] = (double) a[c] + lambda * ((double) deg * (double) a[c] - s[c]);
}

__device__ __forceinline__ void load_row(const float *x, uint32_t w, float a[3]) {
    a[0] = x[3 * (int64_t) w]; a[1] = x[3 * (int64_t) w + 1]; a[2] = x[3 * (int64_t) w + 2];
}

__global__ __launch_bounds__(kBlock) void laplacian_apply_kernel(Table t, int64_t V, double lambda, const float *x, float *y) {
    const int64_t v = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (t.head[1] != (uint32_t) V || v >= V) return;
    double r[3];
    row_product(t, v, lambda, [x](uint32_t w, float a[3]) { load_row(x, w, a); }, r);
    y[3 * v] = (float) r[0]; y[3 * v + 1] = (float) r[1]; y[3 * v + 2] = (float) r[2];
}

// ------------------------------------------------------------------------------------------------ CG, both forms
// the next search direction of one entry: the owner of v and every neighbour that recomputes it evaluate this same expression
__device__ __forceinline__ float direction(float r, float p, double beta) { return (float) ((double) r + beta * (double) p); }

// acc[K] of every lane -> the workgroup's totals in every lane: the wave by the butterfly, the waves in order.  rows: WAVES x K
// doubles of LDS, free again on return.
template <int K, int WAVES>
__device__ __forceinline__ void block_sum(double acc[K], double *rows) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) rows[wave * K + k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
#pragma unroll 4
    for (int w = 0; w < WAVES; ++w)                      // (four rows in flight: sixteen waves' rows at once would not fit the registers)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += rows[w * K + k];
    __syncthreads();
}

// A column's verdict after its residual changed: the relative residual, whether it still runs, its info entry.
__device__ __forceinline__ bool column_verdict(double rr, double bb, double tol, int iterations, EpsmSmoothInfo *info) {
    const double rel = sqrt(rr / bb);
    const bool converged = rel <= tol;
    info->iterations = iterations;
    info->converged = converged;
    info->residual = rel;
    return !converged;
}

// The table is another V's: nothing is solved, and info says so -- no iteration, not converged, a residual of -1.
__device__ __forceinline__ void refuse_table(EpsmSmoothInfo *info) {
    for (int c = 0; c < 3; ++c) { info[c].iterations = 0; info[c].converged = 0; info[c].residual = -1.0; }
}

// ------------------------------------------------------------------------------------------------ GRID
struct State {
    double bb[3], rr[3], alpha[3], beta[3];
    int32_t active[3], zero[3];
    uint32_t done, counter;
};

struct Grid {                       // the workspace
    State *state;
    double *partial;                // 6 doubles per chunk
    float *r, *p[2], *q;
};

size_t grid_carve(int64_t V, char *base, Grid *g) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + o : nullptr; o += table_align_up(bytes); return (void *) p; };
    Grid x;
    x.state = (State *) take(sizeof(State));
    x.partial = (double *) take(48 * (size_t) chunks_of(V));
    x.r = (float *) take(12 * (size_t) V);
    x.p[0] = (float *) take(12 * (size_t) V);
    x.p[1] = (float *) take(12 * (size_t) V);
    x.q = (float *) take(12 * (size_t) V);
    if (g) *g = x;
    return o;
}

// The chunk's row of K doubles goes to partial; true in the one workgroup that arrives last, with every row of the launch
// visible to it and acc holding their sums in chunk order (lane t adds the rows t, t + 256, ...).  The counter is back at 0 for
// the next launch.  rows: 4 x K doubles of LDS.
template <int K>
__device__ __forceinline__ bool sum_over_chunks(double acc[K], double *rows, double *partial, uint32_t *counter) {
    __shared__ bool s_last;
    block_sum<K, kBlock / 64>(acc, rows);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) partial[(int64_t) blockIdx.x * K + k] = acc[k];
        __threadfence();                                                 // the row before the arrival
        s_last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return false;
    __threadfence();                                                     // the arrivals before the rows
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int64_t c = threadIdx.x; c < (int64_t) gridDim.x; c += kBlock)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += partial[c * K + k];
    block_sum<K, kBlock / 64>(acc, rows);
    if (threadIdx.x == 0) *counter = 0;
    return true;
}

// r = b - A x; the last workgroup opens the columns: |b|^2, |r|^2, which are zero, which have converged as they stand.
__global__ __launch_bounds__(kBlock) void cg_init_kernel(Table t, int64_t V, double lambda, const float *b, const float *x, double tol,
                                                         Grid g, EpsmSmoothInfo *info) {
    __shared__ double s_rows[4 * 6];
    if (t.head[1] != (uint32_t) V) {                                     // not this table's V: the solve ends here, x as it was
        if (blockIdx.x == 0 && threadIdx.x == 0) { g.state->done = 1; refuse_table(info); }
        return;
    }
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kChunk / kBlock; ++j) {
        const int64_t v = (int64_t) blockIdx.x * kChunk + j * kBlock + threadIdx.x;
        if (v >= V) continue;
        double y[3];
        row_product(t, v, lambda, [x](uint32_t w, float a[3]) { load_row(x, w, a); }, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float bv = b[3 * v + c], r = (float) ((double) bv - y[c]);
            g.r[3 * v + c] = r;
            acc[c] += (double) r * (double) r;
            acc[3 + c] += (double) bv * (double) bv;
        }
    }
    if (!sum_over_chunks<6>(acc, s_rows, g.partial, &g.state->counter) || threadIdx.x != 0) return;
    State *s = g.state;
    bool any = false;
    for (int c = 0; c < 3; ++c) {
        s->rr[c] = acc[c]; s->bb[c] = acc[3 + c];
        s->alpha[c] = 0.0; s->beta[c] = 0.0;
        s->zero[c] = acc[3 + c] == 0.0;
        if (s->zero[c]) { info[c].iterations = 0; info[c].converged = 1; info[c].residual = 0.0; s->active[c] = 0; }
        else s->active[c] = column_verdict(acc[c], acc[3 + c], tol, 0, &info[c]);
        any = any || s->active[c];
    }
    s->done = !any;
}

// a column with b == 0: x = 0 exactly, whatever the guess was
__global__ __launch_bounds__(kBlock) void cg_zero_kernel(int64_t V, const State *s, float *x) {
    const int64_t v = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (v >= V) return;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (s->zero[c]) x[3 * v + c] = 0.f;
}

// First launch of an iteration: p = r + beta p_old (FIRST: p = r, p_old is not read), q = A p with the neighbours' p recomputed
// from r and p_old, the row p.q; the last workgroup sets alpha = r.r / p.q.
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void cg_direction_kernel(Table t, int64_t V, double lambda, Grid g, int parity) {
    __shared__ double s_rows[4 * 3];
    State *s = g.state;
    if (s->done) return;
    const double beta[3] = {s->beta[0], s->beta[1], s->beta[2]};
    const float *r = g.r, *p_old = g.p[parity ^ 1];
    float *p_new = g.p[parity];
    auto load = [r, p_old, &beta](uint32_t w, float a[3]) {
        load_row(r, w, a);
        if (!FIRST) {
            float o[3];
            load_row(p_old, w, o);
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] = direction(a[c], o[c], beta[c]);
        }
    };
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kChunk / kBlock; ++j) {
        const int64_t v = (int64_t) blockIdx.x * kChunk + j * kBlock + threadIdx.x;
        if (v >= V) continue;
        double y[3];
        float pv[3];
        row_product(t, v, lambda, load, y);
        load((uint32_t) v, pv);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float qv = (float) y[c];
            p_new[3 * v + c] = pv[c];
            g.q[3 * v + c] = qv;
            acc[c] += (double) pv[c] * (double) qv;
        }
    }
    if (!sum_over_chunks<3>(acc, s_rows, g.partial, &s->counter) || threadIdx.x != 0) return;
    for (int c = 0; c < 3; ++c) s->alpha[c] = s->active[c] && acc[c] != 0.0 ? s->rr[c] / acc[c] : 0.0;
}

// Second launch: x += alpha p, r -= alpha q for the columns that still run, the row r.r; the last workgroup gives the verdict
// and the next beta.
__global__ __launch_bounds__(kBlock) void cg_step_kernel(int64_t V, Grid g, int parity, float *x, double tol, int iteration,
                                                         EpsmSmoothInfo *info) {
    __shared__ double s_rows[4 * 3];
    State *s = g.state;
    if (s->done) return;
    const double alpha[3] = {s->alpha[0], s->alpha[1], s->alpha[2]};
    const bool active[3] = {s->active[0] != 0, s->active[1] != 0, s->active[2] != 0};
    const float *p = g.p[parity];
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kChunk / kBlock; ++j) {
        const int64_t v = (int64_t) blockIdx.x * kChunk + j * kBlock + threadIdx.x;
        if (v >= V) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float rv = g.r[3 * v + c];
            if (active[c]) {
                x[3 * v + c] = (float) ((double) x[3 * v + c] + alpha[c] * (double) p[3 * v + c]);
                rv = (float) ((double) rv - alpha[c] * (double) g.q[3 * v + c]);
                g.r[3 * v + c] = rv;
            }
            acc[c] += (double) rv * (double) rv;
        }
    }
    if (!sum_over_chunks<3>(acc, s_rows, g.partial, &s->counter) || threadIdx.x != 0) return;
    bool any = false;
    for (int c = 0; c < 3; ++c) {
        if (!s->active[c]) continue;
        s->active[c] = column_verdict(acc[c], s->bb[c], tol, iteration, &info[c]);
        s->beta[c] = s->active[c] ? acc[c] / s->rr[c] : 0.0;
        s->rr[c] = acc[c];
        any = any || s->active[c];
    }
    s->done = !any;
}

// ------------------------------------------------------------------------------------------------ ONE_GROUP
// Lane l owns the vertices l, l + 1024, ...: ROWS of them.  s_p is the search direction (the guess x before the first residual).
template <int ROWS>
__global__ __launch_bounds__(kOneThreads) void cg_one_group_kernel(Table t, int64_t V, double lambda, const float *b, float *x,
                                                                   int max_iters, double tol, EpsmSmoothInfo *info) {
    constexpr bool kXRegs = ROWS <= kOneRowsInRegisters;
    constexpr int kWaves = kOneThreads / 64;
    __shared__ float s_p[3 * ROWS * kOneThreads];
    __shared__ double s_rows[kWaves * 6];
    if (t.head[1] != (uint32_t) V) {
        if (threadIdx.x == 0) refuse_table(info);
        return;
    }
    const int n = (int) V;
    float xr[kXRegs ? ROWS : 1][3], r[ROWS][3], q[ROWS][3];
    auto load = [&](uint32_t w, float a[3]) { a[0] = s_p[3 * w]; a[1] = s_p[3 * w + 1]; a[2] = s_p[3 * w + 2]; };

#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int v = j * kOneThreads + threadIdx.x;
        if (v >= n) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float xv = x[3 * v + c];
            s_p[3 * v + c] = xv;
            if (kXRegs) xr[j][c] = xv;
        }
    }
    __syncthreads();
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int v = j * kOneThreads + threadIdx.x;
        if (v >= n) continue;
        double y[3];
        row_product(t, v, lambda, load, y);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float bv = b[3 * v + c];
            r[j][c] = (float) ((double) bv - y[c]);
            acc[c] += (double) r[j][c] * (double) r[j][c];
            acc[3 + c] += (double) bv * (double) bv;
        }
    }
    block_sum<6, kWaves>(acc, s_rows);                       // (every lane is past its gather of x here)
    double rr[3], bb[3], beta[3] = {0.0, 0.0, 0.0};
    bool active[3], zero[3];
    EpsmSmoothInfo mine[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        rr[c] = acc[c]; bb[c] = acc[3 + c];
        zero[c] = bb[c] == 0.0;
        mine[c].iterations = 0; mine[c].converged = 1; mine[c].residual = 0.0;
        active[c] = !zero[c] && column_verdict(rr[c], bb[c], tol, 0, &mine[c]);
    }
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int v = j * kOneThreads + threadIdx.x;
        if (v >= n) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) s_p[3 * v + c] = r[j][c];
    }
    __syncthreads();

    for (int k = 1; k <= max_iters && (active[0] || active[1] || active[2]); ++k) {      // (uniform: every lane holds the same scalars)
        double dot[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int v = j * kOneThreads + threadIdx.x;
            if (v >= n) continue;
            double y[3];
            row_product(t, v, lambda, load, y);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                q[j][c] = (float) y[c];
                dot[c] += (double) s_p[3 * v + c] * (double) q[j][c];
            }
        }
        block_sum<3, kWaves>(dot, s_rows);
        double alpha[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { alpha[c] = active[c] && dot[c] != 0.0 ? rr[c] / dot[c] : 0.0; dot[c] = 0.0; }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int v = j * kOneThreads + threadIdx.x;
            if (v >= n) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (active[c]) {
                    const double step = alpha[c] * (double) s_p[3 * v + c];
                    if (kXRegs) xr[j][c] = (float) ((double) xr[j][c] + step);
                    else x[3 * v + c] = (float) ((double) x[3 * v + c] + step);
                    r[j][c] = (float) ((double) r[j][c] - alpha[c] * (double) q[j][c]);
                }
                dot[c] += (double) r[j][c] * (double) r[j][c];
            }
        }
        block_sum<3, kWaves>(dot, s_rows);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (!active[c]) continue;
            active[c] = column_verdict(dot[c], bb[c], tol, k, &mine[c]);
            beta[c] = active[c] ? dot[c] / rr[c] : 0.0;
            rr[c] = dot[c];
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {                      // (every lane is past this iteration's gather: block_sum)
            const int v = j * kOneThreads + threadIdx.x;
            if (v >= n) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) s_p[3 * v + c] = direction(r[j][c], s_p[3 * v + c], beta[c]);
        }
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int v = j * kOneThreads + threadIdx.x;
        if (v >= n) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (zero[c]) x[3 * v + c] = 0.f;
            else if (kXRegs) x[3 * v + c] = xr[j][c];
        }
    }
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) info[c] = mine[c];
}

template <int ROWS>
int launch_one_group(const char *what, void *stream, Table t, int64_t V, double lambda, const float *b, float *x, int max_iters,
                     double tol, EpsmSmoothInfo *info) {
    return launch_checked(what, cg_one_group_kernel<ROWS>, 1, kOneThreads, stream, t, V, lambda, b, x, max_iters, tol, info);
}

const char *counts_invalid(int64_t V) {
    if (V < 0 || V >= kMaxVertices) return "V outside 0 .. 2^31 - 1";
    return nullptr;
}

const char *lambda_invalid(double lambda) { return !(lambda >= 0.0) || !isfinite(lambda) ? "lambda must be finite and >= 0" : nullptr; }

unsigned grid_of(int64_t n, int per) { return (unsigned) ((n + per - 1) / per); }

}  // namespace

extern "C" size_t epsm_mesh_laplacian_bytes(int64_t V, int64_t T) {
    return table_carve(V < 1 ? 1 : V, T < 1 ? 1 : T, nullptr, nullptr);
}

extern "C" int epsm_mesh_laplacian(const uint32_t *tri, int64_t V, int64_t T, const void *topology, void *laplacian,
                                   size_t laplacian_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_mesh_laplacian";
    if (T < 1 || T >= kMaxTriangles) return fail(EPSM_EINVAL, what, "T must be in 1 .. 2^28 - 1");
    if (V < 1 || V >= kMaxVertices) return fail(EPSM_EINVAL, what, "V must be in 1 .. 2^31 - 1");
    if (!tri || !topology || !laplacian) return fail(EPSM_EINVAL, what, "NULL argument");
    if ((uintptr_t) topology % 16) return fail(EPSM_EINVAL, what, "topology must be 16-byte aligned");
    if ((uintptr_t) laplacian % 16) return fail(EPSM_EINVAL, what, "laplacian must be 16-byte aligned");
    if (laplacian_bytes < epsm_mesh_laplacian_bytes(V, T)) return fail(EPSM_EINVAL, what, "laplacian smaller than epsm_mesh_laplacian_bytes(V, T)");
    Table t;
    table_carve(V, T, (char *) laplacian, &t);
    const epsm::Topology top = epsm::topology_carve(V, (char *) topology);
    const hipError_t e = hipMemsetAsync(t.head, 0, 256, (hipStream_t) stream);
    if (e != hipSuccess) return epsm_host::hip_fail(what, e);
    return launch_checked(what, laplacian_rows_kernel, grid_of(V, kBlock), kBlock, stream, tri, V, T, (const uint32_t *) top.row,
                          (const uint32_t *) top.adj, t);
}

extern "C" int epsm_laplacian_apply(const void *laplacian, int64_t V, double lambda, const float *x, float *y, void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_laplacian_apply";
    if (const char *why = counts_invalid(V)) return fail(EPSM_EINVAL, what, why);
    if (const char *why = lambda_invalid(lambda)) return fail(EPSM_EINVAL, what, why);
    if (!laplacian || !x || !y) return fail(EPSM_EINVAL, what, "NULL argument");
    if ((uintptr_t) laplacian % 16) return fail(EPSM_EINVAL, what, "laplacian must be 16-byte aligned");
    if (x == y) return fail(EPSM_EINVAL, what, "x and y must not overlap");
    if (V == 0) return EPSM_OK;
    return launch_checked(what, laplacian_apply_kernel, grid_of(V, kBlock), kBlock, stream, table_of(V, laplacian), V, lambda, x, y);
}

extern "C" size_t epsm_laplacian_solve_bytes(int64_t V) { return grid_carve(V < 1 ? 1 : V, nullptr, nullptr); }

extern "C" int epsm_laplacian_solve(const void *laplacian, int64_t V, double lambda, const float *b, float *x, int32_t max_iters,
                                    double rel_tol, int32_t form, EpsmSmoothInfo *info, void *workspace, size_t workspace_bytes,
                                    void *stream) {
    epsm_host::err_buf()[0] = 0;
    static const char *what = "epsm_laplacian_solve";
    if (const char *why = counts_invalid(V)) return fail(EPSM_EINVAL, what, why);
    if (const char *why = lambda_invalid(lambda)) return fail(EPSM_EINVAL, what, why);
    if (max_iters < 1 || max_iters > kMaxIters) return fail(EPSM_EINVAL, what, "max_iters must be in 1 .. 65536");
    if (!(rel_tol > 0.0 && rel_tol < 1.0)) return fail(EPSM_EINVAL, what, "rel_tol must be inside (0, 1)");
    if (form != EPSM_SMOOTH_AUTO && form != EPSM_SMOOTH_GRID && form != EPSM_SMOOTH_ONE_GROUP)
        return fail(EPSM_EINVAL, what, "form is not an EPSM_SMOOTH_* value");
    if (!laplacian || !b || !x || !info) return fail(EPSM_EINVAL, what, "NULL argument");
    if ((uintptr_t) laplacian % 16) return fail(EPSM_EINVAL, what, "laplacian must be 16-byte aligned");
    if (b == x) return fail(EPSM_EINVAL, what, "b and x must not overlap");
    if (form == EPSM_SMOOTH_ONE_GROUP && V > EPSM_SMOOTH_ONE_GROUP_MAX_V)
        return fail(EPSM_EINVAL, what, "EPSM_SMOOTH_ONE_GROUP serves V <= EPSM_SMOOTH_ONE_GROUP_MAX_V");
    if (!workspace_ok(workspace, workspace_bytes, epsm_laplacian_solve_bytes(V)))
        return fail(EPSM_EINVAL, what, "workspace NULL, misaligned or smaller than epsm_laplacian_solve_bytes(V)");
    if (V == 0) return EPSM_OK;
    if (form == EPSM_SMOOTH_AUTO) form = V <= kAutoOneGroupMaxV ? EPSM_SMOOTH_ONE_GROUP : EPSM_SMOOTH_GRID;
    const Table t = table_of(V, laplacian);

    if (form == EPSM_SMOOTH_ONE_GROUP) {
        const int rows = (int) ((V + kOneThreads - 1) / kOneThreads);
        if (rows <= 1) return launch_one_group<1>(what, stream, t, V, lambda, b, x, max_iters, rel_tol, info);
        if (rows <= 2) return launch_one_group<2>(what, stream, t, V, lambda, b, x, max_iters, rel_tol, info);
        if (rows <= 4) return launch_one_group<4>(what, stream, t, V, lambda, b, x, max_iters, rel_tol, info);
        if (rows <= 7) return launch_one_group<7>(what, stream, t, V, lambda, b, x, max_iters, rel_tol, info);
        return launch_one_group<kOneMaxRows>(what, stream, t, V, lambda, b, x, max_iters, rel_tol, info);
    }

    Grid g;
    grid_carve(V, (char *) workspace, &g);
    const unsigned chunks = (unsigned) chunks_of(V);
    // (the arrival counter starts at 0: cg_init_kernel is the first to count on it and the state is this call's own)
    hipError_t e = hipMemsetAsync(g.state, 0, sizeof(State), (hipStream_t) stream);
    if (e != hipSuccess) return epsm_host::hip_fail(what, e);
    if (const int rc = launch_checked(what, cg_init_kernel, chunks, kBlock, stream, t, V, lambda, b, (const float *) x, rel_tol, g, info)) return rc;
    if (const int rc = launch_checked(what, cg_zero_kernel, grid_of(V, kBlock), kBlock, stream, V, (const State *) g.state, x)) return rc;
    for (int k = 0; k < max_iters; ++k) {
        const int rc = k == 0 ? launch_checked(what, cg_direction_kernel<true>, chunks, kBlock, stream, t, V, lambda, g, k & 1)
                              : launch_checked(what, cg_direction_kernel<false>, chunks, kBlock, stream, t, V, lambda, g, k & 1);
        if (rc) return rc;
        if (const int rc2 = launch_checked(what, cg_step_kernel, chunks, kBlock, stream, V, g, k & 1, x, rel_tol, k + 1, info)) return rc2;
    }
    return EPSM_OK;
}
