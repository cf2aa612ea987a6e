// epsm_trace_scene.hip -- gfx950 scene tables (include/epsm_trace.h: epsm_scene_topology, epsm_vertex_normals,
// epsm_emitter_tables, epsm_environment_tables): what Scene._upload otherwise computes with numpy.
//   topology      the vertex -> (triangle, corner) adjacency in CSR form: a stable LSD radix sort of the 3 T corner entries by
//                 vertex (epsm_trace_scan.h), row offsets by binary search -- each vertex's corners in triangle order;
//   normals       one thread per vertex gathers its corners in that order (fp64): no float atomics, bit-reproducible;
//   emitter       per mesh, chunks of kChunk triangles: fp64 areas and an in-chunk scan, one workgroup per mesh scans its
//                 chunk sums, a last pass writes the normalised CDF; rounded to float32 once;
//   environment   one workgroup per row of cells scans the cell weights (fp64), one workgroup scans the row sums.
// Every sum runs in a fixed order (in-wave shuffles, then the waves in order, then the rounds in order): two calls on the same
// input give identical bits.  Nothing synchronises with the host and nothing allocates.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "epsm_common.h"
#include "epsm_trace_scan.h"
#include "epsm_trace_topology.h"
#include "../../include/epsm_trace.h"

using epsm_host::fail;

namespace {

constexpr int kChunk = 4 * kBlock;                     // triangles per workgroup of the area scan
constexpr int64_t kMaxTriangles = int64_t(1) << 28;    // 3 T corner entries and their sort offsets stay in int32
constexpr int64_t kMaxVertices = int64_t(1) << 31;
constexpr int kMaxEnvTexels = 1 << 26;                 // H (W + 1) 3 stays in int32

size_t align_up(size_t x) { return epsm::table_align_up(x); }
unsigned grid(int64_t n, int per = kBlock) { return (unsigned) ((n + per - 1) / per); }

// Inclusive scan of load(i), i in [0, n), by one workgroup of kBlock threads, kBlock items per round: in-wave shuffles, the
// four wave sums in order, the rounds in order.  store(i, prefix) for every i; returns the total.  lds: kBlock / 64 doubles.
template <class Load, class Store>
__device__ double block_scan_f64(int64_t n, Load load, Store store, double *lds) {
    const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    double carry = 0.0;
    for (int64_t base = 0; base < n; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        const double v = i < n ? load(i) : 0.0;
        double incl = v;
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_up(incl, o);
            if ((int) lane >= o) incl += u;
        }
        if (lane == 63) lds[w] = incl;
        __syncthreads();
        double before = carry, round = 0.0;
        for (unsigned q = 0; q < kBlock / 64; ++q) {
            if (q == w) before += round;
            round += lds[q];
        }
        if (i < n) store(i, before + incl);
        carry += round;
        __syncthreads();
    }
    return carry;
}

// A rounded product the compiler may not fuse into the add that follows.  The Makefile's -ffp-contract=fast (which overrides
// `#pragma clang fp contract`) would turn a x b - c x d into fma(a, b, -c x d): the cross product of two equal edges (a
// triangle that repeats a vertex) then leaves a rounding residue instead of 0, which the normalisation blows up into a unit
// face normal.  The host rules round every operation; so do these helpers.
__device__ __forceinline__ double mul(double a, double b) {
    double p = a * b;
    asm("" : "+v"(p));
    return p;
}
__device__ __forceinline__ void cross(const double a[3], const double b[3], double o[3]) {
    o[0] = mul(a[1], b[2]) - mul(a[2], b[1]);
    o[1] = mul(a[2], b[0]) - mul(a[0], b[2]);
    o[2] = mul(a[0], b[1]) - mul(a[1], b[0]);
}
__device__ __forceinline__ double dot(const double a[3], const double b[3]) {
    return mul(a[0], b[0]) + mul(a[1], b[1]) + mul(a[2], b[2]);
}

__device__ __forceinline__ void load_p(const float *pos, uint32_t v, double p[3]) {
    p[0] = pos[3 * (int64_t) v]; p[1] = pos[3 * (int64_t) v + 1]; p[2] = pos[3 * (int64_t) v + 2];
}

__device__ __forceinline__ double tri_area(const float *pos, const uint32_t *tri, int64_t t, int64_t V) {
    const uint32_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    if (i0 >= V || i1 >= V || i2 >= V) return 0.0;
    double a[3], b[3], c[3], x[3];
    load_p(pos, i0, a); load_p(pos, i1, b); load_p(pos, i2, c);
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    cross(e1, e2, x);
    return 0.5 * sqrt(dot(x, x));
}

// ------------------------------------------------------------------------------------------------ topology
using epsm::Topology;                                   // (epsm_trace_topology.h: the Laplacian table reads it too)
using epsm::topology_carve;
using epsm::topology_size;

struct SortSpace { uint32_t *keys0, *keys1, *vals; int *hist, *off, *scan_scratch, *total; };

size_t sort_carve(int64_t T, char *base, SortSpace *s) {
    const int64_t E = 3 * T, tiles = (E + kBlock - 1) / kBlock, H = 16 * tiles;
    size_t o = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + o : nullptr; o += align_up(bytes); return (void *) p; };
    SortSpace x;
    x.keys0 = (uint32_t *) take(4 * E); x.keys1 = (uint32_t *) take(4 * E); x.vals = (uint32_t *) take(4 * E);
    x.hist = (int *) take(4 * H); x.off = (int *) take(4 * H);
    x.scan_scratch = (int *) take(4 * scan_scratch_ints(H));
    x.total = (int *) take(4 * 16);
    if (s) *s = x;
    return o;
}

__global__ __launch_bounds__(kBlock) void corner_entries(const uint32_t *tri, int64_t E, uint32_t *keys, uint32_t *vals) {
    const int64_t e = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (e >= E) return;
    keys[e] = tri[e];
    vals[e] = (uint32_t) e;
}

__global__ __launch_bounds__(kBlock) void row_offsets(const uint32_t *keys, int64_t E, int64_t V, uint32_t *row) {
    const int64_t v = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (v > V) return;
    int64_t lo = 0, hi = E;                              // first sorted entry with key >= v
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t) keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    row[v] = (uint32_t) lo;
}

// ------------------------------------------------------------------------------------------------ vertex normals
// scene.vertex_normals: per corner the normalised face normal times the corner angle, summed per vertex in triangle order,
// normalised; (0, 0, 1) for a zero sum.
__global__ __launch_bounds__(kBlock) void vertex_normals_kernel(const float *pos, int64_t V, const uint32_t *tri, const uint32_t *row,
                                                                const uint32_t *adj, int64_t v_begin, int64_t v_end, float *nrm) {
    const int64_t v = v_begin + (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (v >= v_end) return;
    double n[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = row[v]; j < row[v + 1]; ++j) {
        const uint32_t e = adj[j], t = e / 3u, c = e - 3u * t;
        const uint32_t id[3] = {tri[3 * (int64_t) t], tri[3 * (int64_t) t + 1], tri[3 * (int64_t) t + 2]};
        if (id[0] >= V || id[1] >= V || id[2] >= V) continue;
        double p[3][3];
        for (int k = 0; k < 3; ++k) load_p(pos, id[k], p[k]);
        const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        double fn[3];
        cross(e1, e2, fn);
        const double ln = sqrt(dot(fn, fn));
        for (int k = 0; k < 3; ++k) fn[k] = ln > 0.0 ? fn[k] / fmax(ln, 1e-30) : 0.0;
        const double *pc = p[c], *pa = p[(c + 1) % 3], *pb = p[(c + 2) % 3];
        const double d0[3] = {pa[0] - pc[0], pa[1] - pc[1], pa[2] - pc[2]}, d1[3] = {pb[0] - pc[0], pb[1] - pc[1], pb[2] - pc[2]};
        const double cosang = dot(d0, d1) / fmax(mul(sqrt(dot(d0, d0)), sqrt(dot(d1, d1))), 1e-30);
        const double ang = acos(fmin(fmax(cosang, -1.0), 1.0));
        for (int k = 0; k < 3; ++k) n[k] += mul(fn[k], ang);
    }
    const double ln = sqrt(dot(n, n));
    float *o = nrm + 3 * v;
    if (ln > 0.0) {
        const double s = fmax(ln, 1e-30);
        o[0] = (float) (n[0] / s); o[1] = (float) (n[1] / s); o[2] = (float) (n[2] / s);
    } else {
        o[0] = 0.f; o[1] = 0.f; o[2] = 1.f;
    }
}

// ------------------------------------------------------------------------------------------------ vertex normals: derivative
// d n_v / d p_w of the rule above, both directions (epsm_vertex_normals_backward / _forward).  The primal's arithmetic is
// repeated operation for operation, so every cut falls where the primal's does; where the primal is cut to a constant the
// derivative is 0 (DESIGN 5h's rule): a face normal or a vertex sum whose length is on its floor (0, or below the 1e-30 of the
// fmax), a cosine on or outside [-1, 1], a corner whose edge lengths' product is on that floor, a triangle naming an index >= V.
// A launch covers one run [v_begin, v_end) of flagged vertex rows; positions outside the run are constants to it (a triangle of
// a mesh names that mesh's vertices), which keeps the two directions exact transposes.  Corners are picked with selects, not
// with indexed register arrays: no scratch.
constexpr double kFloor = 1e-30;

struct TriGeom {
    uint32_t id[3];
    double p[3][3], e1[3], e2[3], fn[3], ln;            // fn, ln: as vertex_normals_kernel forms them
};

__device__ __forceinline__ bool tri_geom(const float *pos, int64_t V, const uint32_t *tri, uint32_t t, TriGeom &g) {
    for (int k = 0; k < 3; ++k) g.id[k] = tri[3 * (int64_t) t + k];
    if (g.id[0] >= V || g.id[1] >= V || g.id[2] >= V) return false;
    for (int k = 0; k < 3; ++k) load_p(pos, g.id[k], g.p[k]);
    for (int k = 0; k < 3; ++k) { g.e1[k] = g.p[1][k] - g.p[0][k]; g.e2[k] = g.p[2][k] - g.p[0][k]; }
    cross(g.e1, g.e2, g.fn);
    g.ln = sqrt(dot(g.fn, g.fn));
    for (int k = 0; k < 3; ++k) g.fn[k] = g.ln > 0.0 ? g.fn[k] / fmax(g.ln, kFloor) : 0.0;
    return true;
}

__device__ __forceinline__ void pick(const double a[3][3], uint32_t c, double o[3]) {
    for (int k = 0; k < 3; ++k) {
        const double a0 = a[0][k], a1 = a[1][k], a2 = a[2][k];       // values, not addresses, go through the selects
        o[k] = c == 0u ? a0 : (c == 1u ? a1 : a2);
    }
}

// the corner at pc between d0 = pa - pc and d1 = pb - pc: the primal's angle, and d angle / d d0, d d1 (0 where it is cut)
struct Corner { double ang, g0[3], g1[3]; };

__device__ __forceinline__ Corner corner(const double pc[3], const double pa[3], const double pb[3], bool want_grad) {
    Corner r;
    const double d0[3] = {pa[0] - pc[0], pa[1] - pc[1], pa[2] - pc[2]}, d1[3] = {pb[0] - pc[0], pb[1] - pc[1], pb[2] - pc[2]};
    const double q0 = dot(d0, d0), q1 = dot(d1, d1), den = mul(sqrt(q0), sqrt(q1));
    const double cosang = dot(d0, d1) / fmax(den, kFloor);
    r.ang = acos(fmin(fmax(cosang, -1.0), 1.0));
    for (int k = 0; k < 3; ++k) r.g0[k] = r.g1[k] = 0.0;
    if (want_grad && den > kFloor && cosang > -1.0 && cosang < 1.0) {
        const double s = -1.0 / sqrt(mul(1.0 - cosang, 1.0 + cosang));          // d acos / d cos
        for (int k = 0; k < 3; ++k) {
            r.g0[k] = mul(s, d1[k] / den - mul(cosang, d0[k]) / q0);
            r.g1[k] = mul(s, d0[k] / den - mul(cosang, d1[k]) / q1);
        }
    }
    return r;
}

// N_v: the primal's sum over the CSR row of v, in its order
__device__ __forceinline__ void vertex_sum(const float *pos, int64_t V, const uint32_t *tri, const uint32_t *row, const uint32_t *adj,
                                           int64_t v, double n[3]) {
    n[0] = n[1] = n[2] = 0.0;
    for (uint32_t j = row[v]; j < row[v + 1]; ++j) {
        const uint32_t e = adj[j], t = e / 3u, c = e - 3u * t;
        TriGeom g;
        if (!tri_geom(pos, V, tri, t, g)) continue;
        double pc[3], pa[3], pb[3];
        pick(g.p, c, pc); pick(g.p, (c + 1u) % 3u, pa); pick(g.p, (c + 2u) % 3u, pb);
        const double ang = corner(pc, pa, pb, false).ang;
        for (int k = 0; k < 3; ++k) n[k] += mul(g.fn[k], ang);
    }
}

// backward, launch 1: a_v = (I - n_v n_v^T) g_nrm[v] / |N_v| (three doubles per vertex; 0 where the sum is cut)
__global__ __launch_bounds__(kBlock) void normals_adjoint_sum(const float *pos, int64_t V, const uint32_t *tri, const uint32_t *row,
                                                              const uint32_t *adj, int64_t v_begin, int64_t v_end, const float *g_nrm,
                                                              double *a) {
    const int64_t v = v_begin + (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (v >= v_end) return;
    double n[3], o[3] = {0.0, 0.0, 0.0};
    vertex_sum(pos, V, tri, row, adj, v, n);
    const double ln = sqrt(dot(n, n));
    if (ln > kFloor) {
        const double g[3] = {g_nrm[3 * v], g_nrm[3 * v + 1], g_nrm[3 * v + 2]};
        for (int k = 0; k < 3; ++k) n[k] /= ln;
        const double ng = dot(n, g);
        for (int k = 0; k < 3; ++k) o[k] = (g[k] - mul(n[k], ng)) / ln;
    }
    a[3 * v] = o[0]; a[3 * v + 1] = o[1]; a[3 * v + 2] = o[2];
}

// backward, launch 2: g_pos[w] += d / d p_w of sum_t sum_c a_{i_c} . (theta_c f_t) over the triangles at w, in triangle order
__global__ __launch_bounds__(kBlock) void normals_adjoint_positions(const float *pos, int64_t V, const uint32_t *tri, const uint32_t *row,
                                                                    const uint32_t *adj, int64_t v_begin, int64_t v_end, const double *a,
                                                                    float *g_pos) {
    const int64_t w = v_begin + (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (w >= v_end) return;
    double acc[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = row[w]; j < row[w + 1]; ++j) {
        const uint32_t e = adj[j], t = e / 3u, c = e - 3u * t;       // w is corner c of triangle t
        TriGeom g;
        if (!tri_geom(pos, V, tri, t, g)) continue;
        double av[3][3], b[3] = {0.0, 0.0, 0.0}, G[3] = {0.0, 0.0, 0.0};
        for (int i = 0; i < 3; ++i) {
            const bool in = (int64_t) g.id[i] >= v_begin && (int64_t) g.id[i] < v_end;
            for (int k = 0; k < 3; ++k) av[i][k] = in ? a[3 * (int64_t) g.id[i] + k] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {                                // the three angle parts (a_i . f) d theta_i / d p_w
            const int ia = (i + 1) % 3, ib = (i + 2) % 3;
            const Corner cr = corner(g.p[i], g.p[ia], g.p[ib], true);
            const double s = dot(av[i], g.fn);
            for (int k = 0; k < 3; ++k) {
                b[k] += mul(cr.ang, av[i][k]);
                const double d = c == (uint32_t) i ? -(cr.g0[k] + cr.g1[k]) : (c == (uint32_t) ia ? cr.g0[k] : cr.g1[k]);
                G[k] += mul(s, d);
            }
        }
        if (g.ln > kFloor) {                                         // the face-normal part with weight b = sum_i theta_i a_i
            const double fb = dot(g.fn, b);
            double gx[3], ge1[3], ge2[3];
            for (int k = 0; k < 3; ++k) gx[k] = (b[k] - mul(g.fn[k], fb)) / g.ln;
            cross(g.e2, gx, ge1);                                    // d (gx . (e1 x e2)) / d e1, / d e2
            cross(gx, g.e1, ge2);
            for (int k = 0; k < 3; ++k) G[k] += c == 0u ? -(ge1[k] + ge2[k]) : (c == 1u ? ge1[k] : ge2[k]);
        }
        for (int k = 0; k < 3; ++k) acc[k] += G[k];
    }
    float *o = g_pos + 3 * w;
    o[0] += (float) acc[0]; o[1] += (float) acc[1]; o[2] += (float) acc[2];
}

// forward: d_nrm[v] += (I - n n^T) / |N_v| sum over the corners at v of (d theta f + theta d f), in triangle order
__global__ __launch_bounds__(kBlock) void normals_tangent(const float *pos, int64_t V, const uint32_t *tri, const uint32_t *row,
                                                          const uint32_t *adj, int64_t v_begin, int64_t v_end, const float *d_pos,
                                                          float *d_nrm) {
    const int64_t v = v_begin + (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (v >= v_end) return;
    double n[3] = {0.0, 0.0, 0.0}, dn[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = row[v]; j < row[v + 1]; ++j) {
        const uint32_t e = adj[j], t = e / 3u, c = e - 3u * t;
        TriGeom g;
        if (!tri_geom(pos, V, tri, t, g)) continue;
        double tp[3][3];
        for (int i = 0; i < 3; ++i) {
            const bool in = (int64_t) g.id[i] >= v_begin && (int64_t) g.id[i] < v_end;
            for (int k = 0; k < 3; ++k) tp[i][k] = in ? (double) d_pos[3 * (int64_t) g.id[i] + k] : 0.0;
        }
        double df[3] = {0.0, 0.0, 0.0};
        if (g.ln > kFloor) {
            const double de1[3] = {tp[1][0] - tp[0][0], tp[1][1] - tp[0][1], tp[1][2] - tp[0][2]};
            const double de2[3] = {tp[2][0] - tp[0][0], tp[2][1] - tp[0][1], tp[2][2] - tp[0][2]};
            double x1[3], x2[3], dx[3];
            cross(de1, g.e2, x1);
            cross(g.e1, de2, x2);
            for (int k = 0; k < 3; ++k) dx[k] = x1[k] + x2[k];
            const double fx = dot(g.fn, dx);
            for (int k = 0; k < 3; ++k) df[k] = (dx[k] - mul(g.fn[k], fx)) / g.ln;
        }
        double pc[3], pa[3], pb[3], tc[3], ta[3], tb[3];
        pick(g.p, c, pc); pick(g.p, (c + 1u) % 3u, pa); pick(g.p, (c + 2u) % 3u, pb);
        pick(tp, c, tc); pick(tp, (c + 1u) % 3u, ta); pick(tp, (c + 2u) % 3u, tb);
        const Corner cr = corner(pc, pa, pb, true);
        const double dd0[3] = {ta[0] - tc[0], ta[1] - tc[1], ta[2] - tc[2]}, dd1[3] = {tb[0] - tc[0], tb[1] - tc[1], tb[2] - tc[2]};
        const double dang = dot(cr.g0, dd0) + dot(cr.g1, dd1);
        for (int k = 0; k < 3; ++k) {
            n[k] += mul(g.fn[k], cr.ang);
            dn[k] += mul(dang, g.fn[k]) + mul(cr.ang, df[k]);
        }
    }
    const double ln = sqrt(dot(n, n));
    if (!(ln > kFloor)) return;
    for (int k = 0; k < 3; ++k) n[k] /= ln;
    const double nd = dot(n, dn);
    float *o = d_nrm + 3 * v;
    for (int k = 0; k < 3; ++k) o[k] += (float) ((dn[k] - mul(n[k], nd)) / ln);
}

// ------------------------------------------------------------------------------------------------ emitter tables
struct EmitterSpace { double *local, *chunk_sum, *chunk_off, *mesh_total; int *chunk_begin; };

int64_t chunk_capacity(int64_t T, int64_t n_meshes) { return (T + kChunk - 1) / kChunk + n_meshes; }

size_t emitter_carve(int64_t T, int64_t n_meshes, char *base, EmitterSpace *s) {
    const int64_t C = chunk_capacity(T, n_meshes);
    size_t o = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + o : nullptr; o += align_up(bytes); return (void *) p; };
    EmitterSpace x;
    x.local = (double *) take(8 * T);
    x.chunk_sum = (double *) take(8 * C); x.chunk_off = (double *) take(8 * C);
    x.mesh_total = (double *) take(8 * n_meshes);
    x.chunk_begin = (int *) take(4 * (n_meshes + 1));
    if (s) *s = x;
    return o;
}

struct MeshRange { int64_t t0, n, cdf0; };

// the range the kernels use: the device table's, clipped to the arrays (the host copy was checked before the launch)
__device__ __forceinline__ MeshRange mesh_range(const EpsmMesh &m, int64_t T, int64_t cdf_len) {
    const int64_t t0 = m.tri_begin, c0 = m.cdf_begin;
    int64_t n = m.tri_count;
    if (t0 + n > T) n = T - t0;
    if (c0 + n > cdf_len) n = cdf_len - c0;
    return MeshRange{t0, n > 0 ? n : 0, c0};
}

__global__ __launch_bounds__(kBlock) void mesh_chunks(const EpsmMesh *meshes, int n_meshes, int64_t T, int64_t cdf_len, int cap,
                                                      int *chunk_begin) {
    __shared__ double lds[kBlock / 64];
    if (threadIdx.x == 0) chunk_begin[0] = 0;
    // chunk counts are small integers: the fp64 scan is exact
    block_scan_f64(n_meshes,
                   [&](int64_t m) { return (double) ((mesh_range(meshes[m], T, cdf_len).n + kChunk - 1) / kChunk); },
                   [&](int64_t m, double s) { chunk_begin[m + 1] = (int) fmin(s, (double) cap); }, lds);
}

__device__ __forceinline__ int find_mesh(const int *chunk_begin, int n_meshes, int c) {   // last m with chunk_begin[m] <= c
    int lo = 0, hi = n_meshes;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_begin[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void area_chunks(const float *pos, int64_t V, const uint32_t *tri, int64_t T, const EpsmMesh *meshes,
                                                      int n_meshes, int64_t cdf_len, EmitterSpace w) {
    __shared__ double lds[kBlock / 64];
    const int c = blockIdx.x;
    if (c >= w.chunk_begin[n_meshes]) return;
    const int m = find_mesh(w.chunk_begin, n_meshes, c);
    const MeshRange r = mesh_range(meshes[m], T, cdf_len);
    const int64_t t0 = r.t0 + (int64_t) (c - w.chunk_begin[m]) * kChunk;
    const int64_t n = r.t0 + r.n - t0 < kChunk ? r.t0 + r.n - t0 : kChunk;
    const double total = block_scan_f64(n, [&](int64_t i) { return tri_area(pos, tri, t0 + i, V); },
                                        [&](int64_t i, double s) { w.local[t0 + i] = s; }, lds);
    if (threadIdx.x == 0) w.chunk_sum[c] = total;
}

__global__ __launch_bounds__(kBlock) void mesh_totals(EpsmMesh *meshes, int n_meshes, EmitterSpace w) {
    __shared__ double lds[kBlock / 64];
    const int m = blockIdx.x, c0 = w.chunk_begin[m], nc = w.chunk_begin[m + 1] - c0;
    const double total = block_scan_f64(nc, [&](int64_t i) { return w.chunk_sum[c0 + i]; },
                                        [&](int64_t i, double s) { w.chunk_off[c0 + i] = s - w.chunk_sum[c0 + i]; }, lds);
    if (threadIdx.x == 0) {
        w.mesh_total[m] = total;
        meshes[m].area = (float) total;
    }
}

__global__ __launch_bounds__(kBlock) void cdf_chunks(const EpsmMesh *meshes, int n_meshes, int64_t T, int64_t cdf_len, EmitterSpace w,
                                                     float *cdf) {
    const int c = blockIdx.x;
    if (c >= w.chunk_begin[n_meshes]) return;
    const int m = find_mesh(w.chunk_begin, n_meshes, c);
    const MeshRange r = mesh_range(meshes[m], T, cdf_len);
    const int64_t k0 = (int64_t) (c - w.chunk_begin[m]) * kChunk;
    const int64_t n = r.n - k0 < kChunk ? r.n - k0 : kChunk;
    const double off = w.chunk_off[c], norm = fmax(w.mesh_total[m], 1e-30);
    for (int64_t i = threadIdx.x; i < n; i += kBlock)
        cdf[r.cdf0 + k0 + i] = (float) ((off + w.local[r.t0 + k0 + i]) / norm);
}

// ------------------------------------------------------------------------------------------------ environment tables
struct EnvSpace { double *w, *cum, *rows, *total; };

size_t env_carve(int64_t W, int64_t H, char *base, EnvSpace *s) {
    const int64_t cells = (H - 1) * W;
    size_t o = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + o : nullptr; o += align_up(bytes); return (void *) p; };
    EnvSpace x;
    x.w = (double *) take(8 * cells); x.cum = (double *) take(8 * cells);
    x.rows = (double *) take(8 * (H - 1)); x.total = (double *) take(8);
    if (s) *s = x;
    return o;
}

__global__ __launch_bounds__(kBlock) void env_texels(const float *bitmap, int W, int H, float *texels) {
    const int64_t i = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t) H * (W + 1) * 3) return;
    const int64_t k = i % 3, col = (i / 3) % (W + 1), row = i / (3 * (W + 1));
    texels[i] = bitmap[(row * W + (col == W ? 0 : col)) * 3 + k];
}

__device__ __forceinline__ double env_lum(const float *bitmap, int W, int H, int j, int i) {   // luminance x sin(theta), i wraps
    const float *t = bitmap + ((int64_t) j * W + (i == W ? 0 : i)) * 3;
    return mul(mul(0.212671, t[0]) + mul(0.715160, t[1]) + mul(0.072169, t[2]), sin(j * M_PI / (H - 1)));
}

// numpy.linspace(1 / n, 1, n)[k]: start + k step, the last entry exactly 1
__device__ __forceinline__ double linspace_unit(int64_t k, int64_t n) {
    if (k == n - 1) return 1.0;
    const double start = 1.0 / n;
    return k * ((1.0 - start) / (n - 1)) + start;
}

__global__ __launch_bounds__(kBlock) void env_rows(const float *bitmap, int W, int H, EnvSpace s) {
    __shared__ double lds[kBlock / 64];
    const int j = blockIdx.x;
    double *w = s.w + (int64_t) j * W, *cum = s.cum + (int64_t) j * W;
    const double total = block_scan_f64(W, [&](int64_t i) {
            const double x = 0.25 * (env_lum(bitmap, W, H, j, i) + env_lum(bitmap, W, H, j, i + 1) + env_lum(bitmap, W, H, j + 1, i) +
                                     env_lum(bitmap, W, H, j + 1, i + 1));
            w[i] = x;
            return x;
        }, [&](int64_t i, double v) { cum[i] = v; }, lds);
    if (threadIdx.x == 0) s.rows[j] = total;
}

__global__ __launch_bounds__(kBlock) void env_row_cdf(int H, EnvSpace s, float *row_cdf) {
    __shared__ double lds[kBlock / 64];
    __shared__ double total;
    const int n = H - 1;
    // pass 1: the total; pass 2: the normalised prefix (the same fixed order, so the last prefix equals the total)
    const double t = block_scan_f64(n, [&](int64_t j) { return s.rows[j]; }, [&](int64_t, double) {}, lds);
    if (threadIdx.x == 0) { total = t; *s.total = t; }
    __syncthreads();
    block_scan_f64(n, [&](int64_t j) { return s.rows[j]; },
                   [&](int64_t j, double v) { row_cdf[j] = (float) (j == n - 1 ? 1.0 : total > 0.0 ? v / total : linspace_unit(j, n)); },
                   lds);
}

__global__ __launch_bounds__(kBlock) void env_cells(int W, int H, EnvSpace s, float *col_cdf, float *cell_pdf) {
    const int64_t i = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t) (H - 1) * W) return;
    const int64_t j = i / W, k = i % W;
    const double rows = s.rows[j], total = *s.total;
    col_cdf[i] = (float) (k == W - 1 ? 1.0 : rows > 0.0 ? s.cum[i] / rows : linspace_unit(k, W));
    cell_pdf[i] = (float) (total > 0.0 ? s.w[i] / total * ((double) W * (H - 1)) : 0.0);
}

int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? EPSM_OK : epsm_host::hip_fail(what, e);
}

// Non-empty ranges [begin, begin + count) must not overlap: two chunks would then write the same scratch and CDF entries.
bool ranges_overlap(std::vector<std::pair<int64_t, int64_t>> &r) {
    std::sort(r.begin(), r.end());
    for (size_t i = 1; i < r.size(); ++i)
        if (r[i].first < r[i - 1].first + r[i - 1].second) return true;
    return false;
}

// what the entry points taking the host copy of a mesh table check of it
int check_meshes(const char *what, const EpsmMesh *meshes, int32_t n_meshes, int64_t T) {
    std::vector<std::pair<int64_t, int64_t>> r;
    for (int32_t m = 0; m < n_meshes; ++m) {
        if ((int64_t) meshes[m].tri_begin + meshes[m].tri_count > T) return fail(EPSM_EINVAL, what, "a mesh's triangle range ends beyond T");
        if (meshes[m].tri_count) r.emplace_back(meshes[m].tri_begin, meshes[m].tri_count);
    }
    if (ranges_overlap(r)) return fail(EPSM_EINVAL, what, "the meshes' triangle ranges overlap");
    return EPSM_OK;
}

}  // namespace

extern "C" {

size_t epsm_scene_topology_bytes(int64_t V, int64_t T) {
    if (V < 1) V = 1;
    if (T < 1) T = 1;
    return topology_size(V, T);
}

size_t epsm_scene_topology_workspace_bytes(int64_t T) {
    if (T < 1) T = 1;
    return sort_carve(T, nullptr, nullptr);
}

int epsm_scene_topology(const uint32_t *tri, int64_t V, int64_t T, void *topology, size_t topology_bytes,
                        void *workspace, size_t workspace_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    const char *what = "epsm_scene_topology";
    if (T < 1 || T >= kMaxTriangles) return fail(EPSM_EINVAL, what, "T must be in 1 .. 2^28 - 1");
    if (V < 1 || V >= kMaxVertices) return fail(EPSM_EINVAL, what, "V must be in 1 .. 2^31 - 1");
    if (!tri || !topology || !workspace) return fail(EPSM_EINVAL, what, "NULL argument");
    if (topology_bytes < epsm_scene_topology_bytes(V, T)) return fail(EPSM_EINVAL, what, "topology smaller than epsm_scene_topology_bytes(V, T)");
    if (workspace_bytes < epsm_scene_topology_workspace_bytes(T))
        return fail(EPSM_EINVAL, what, "workspace smaller than epsm_scene_topology_workspace_bytes(T)");
    if ((uintptr_t) topology % 16 || (uintptr_t) workspace % 16) return fail(EPSM_EINVAL, what, "topology and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
    const Topology top = topology_carve(V, (char *) topology);
    SortSpace w;
    sort_carve(T, (char *) workspace, &w);
    const int64_t E = 3 * T;
    int bits = 1;
    while (bits < 32 && (int64_t(1) << bits) < V) ++bits;        // keys < V
    const int passes = (bits + kRadixBits - 1) / kRadixBits;
    // the values end in top.adj: start there after an even number of passes, in the scratch copy after an odd one
    uint32_t *kin = w.keys0, *kout = w.keys1, *vin = passes % 2 ? w.vals : top.adj, *vout = passes % 2 ? top.adj : w.vals;
    const int tiles = (int) grid(E);
    hipLaunchKernelGGL(corner_entries, dim3(tiles), dim3(kBlock), 0, st, tri, E, kin, vin);
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(radix_hist, dim3(tiles), dim3(kBlock), 0, st, kin, E, p * kRadixBits, w.hist, tiles);
        exclusive_scan(w.hist, w.off, 16 * tiles, w.total, w.scan_scratch, st);
        hipLaunchKernelGGL(radix_scatter, dim3(tiles), dim3(kBlock), 0, st, kin, vin, kout, vout, E, p * kRadixBits, w.off, tiles);
        uint32_t *t = kin; kin = kout; kout = t;
        t = vin; vin = vout; vout = t;
    }
    hipLaunchKernelGGL(row_offsets, dim3(grid(V + 1)), dim3(kBlock), 0, st, kin, E, V, top.row);
    return launched(what);
}

int epsm_vertex_normals(const float *positions, int64_t V, const uint32_t *tri, int64_t T, const void *topology,
                        const EpsmMesh *meshes, const int64_t *vertex_begin, int32_t n_meshes, float *normals, void *stream) {
    epsm_host::err_buf()[0] = 0;
    const char *what = "epsm_vertex_normals";
    if (T < 1 || T >= kMaxTriangles) return fail(EPSM_EINVAL, what, "T must be in 1 .. 2^28 - 1");
    if (V < 1 || V >= kMaxVertices) return fail(EPSM_EINVAL, what, "V must be in 1 .. 2^31 - 1");
    if (n_meshes < 0) return fail(EPSM_EINVAL, what, "n_meshes must be >= 0");
    if (!positions || !tri || !topology || !normals || (n_meshes > 0 && (!meshes || !vertex_begin)))
        return fail(EPSM_EINVAL, what, "NULL argument");
    if ((uintptr_t) topology % 16) return fail(EPSM_EINVAL, what, "topology must be 16-byte aligned");
    int rc = check_meshes(what, meshes, n_meshes, T);
    if (rc != EPSM_OK) return rc;
    for (int32_t m = 0; m < n_meshes; ++m)
        if (vertex_begin[m] < 0 || vertex_begin[m + 1] < vertex_begin[m] || vertex_begin[m + 1] > V)
            return fail(EPSM_EINVAL, what, "vertex_begin must not decrease and must stay inside 0 .. V");
    if (n_meshes == 0) return EPSM_OK;
    const Topology top = topology_carve(V, (char *) topology);
    hipStream_t st = (hipStream_t) stream;
    for (int32_t m = 0; m < n_meshes;) {                      // one launch per run of consecutive flagged meshes
        if (!(meshes[m].flags & EPSM_MESH_VERTEX_NORMALS)) { ++m; continue; }
        const int64_t v0 = vertex_begin[m];
        while (m < n_meshes && (meshes[m].flags & EPSM_MESH_VERTEX_NORMALS)) ++m;
        const int64_t v1 = vertex_begin[m];
        if (v1 > v0)
            hipLaunchKernelGGL(vertex_normals_kernel, dim3(grid(v1 - v0)), dim3(kBlock), 0, st, positions, V, tri, top.row, top.adj,
                               v0, v1, normals);
    }
    return launched(what);
}

size_t epsm_vertex_normals_backward_bytes(int64_t V) {
    if (V < 1) V = 1;
    return align_up(24 * (size_t) V);
}

}  // extern "C"

namespace {

// What both directions check of their host arguments, in this order: the counts, then (nothing to do: *done) V == 0, T == 0 or
// an empty table, then the pointers and the host tables.
int check_normals_derivative(const char *what, int64_t V, int64_t T, int32_t n_meshes, bool pointers, const void *topology,
                             const EpsmMesh *meshes, const int64_t *vertex_begin, bool *done) {
    *done = false;
    if (T < 0 || T >= kMaxTriangles) return fail(EPSM_EINVAL, what, "T must be in 0 .. 2^28 - 1");
    if (V < 0 || V >= kMaxVertices) return fail(EPSM_EINVAL, what, "V must be in 0 .. 2^31 - 1");
    if (n_meshes < 0) return fail(EPSM_EINVAL, what, "n_meshes must be >= 0");
    if (V == 0 || T == 0 || n_meshes == 0) { *done = true; return EPSM_OK; }
    if (!pointers || !topology || !meshes || !vertex_begin) return fail(EPSM_EINVAL, what, "NULL argument");
    if ((uintptr_t) topology % 16) return fail(EPSM_EINVAL, what, "topology must be 16-byte aligned");
    int rc = check_meshes(what, meshes, n_meshes, T);
    if (rc != EPSM_OK) return rc;
    for (int32_t m = 0; m < n_meshes; ++m)
        if (vertex_begin[m] < 0 || vertex_begin[m + 1] < vertex_begin[m] || vertex_begin[m + 1] > V)
            return fail(EPSM_EINVAL, what, "vertex_begin must not decrease and must stay inside 0 .. V");
    return EPSM_OK;
}

// f(v0, v1) for every run of consecutive meshes flagged EPSM_MESH_VERTEX_NORMALS that holds a vertex
template <class F>
void for_flagged_runs(const EpsmMesh *meshes, const int64_t *vertex_begin, int32_t n_meshes, F f) {
    for (int32_t m = 0; m < n_meshes;) {
        if (!(meshes[m].flags & EPSM_MESH_VERTEX_NORMALS)) { ++m; continue; }
        const int64_t v0 = vertex_begin[m];
        while (m < n_meshes && (meshes[m].flags & EPSM_MESH_VERTEX_NORMALS)) ++m;
        if (vertex_begin[m] > v0) f(v0, vertex_begin[m]);
    }
}

}  // namespace

extern "C" {

int epsm_vertex_normals_backward(const float *positions, int64_t V, const uint32_t *tri, int64_t T, const void *topology,
                                 const EpsmMesh *meshes, const int64_t *vertex_begin, int32_t n_meshes, const float *g_nrm,
                                 float *g_pos, void *workspace, size_t workspace_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    const char *what = "epsm_vertex_normals_backward";
    bool done;
    int rc = check_normals_derivative(what, V, T, n_meshes, positions && tri && g_nrm && g_pos && workspace, topology, meshes,
                                      vertex_begin, &done);
    if (rc != EPSM_OK || done) return rc;
    if (workspace_bytes < epsm_vertex_normals_backward_bytes(V))
        return fail(EPSM_EINVAL, what, "workspace smaller than epsm_vertex_normals_backward_bytes(V)");
    if ((uintptr_t) workspace % 16) return fail(EPSM_EINVAL, what, "workspace must be 16-byte aligned");
    const Topology top = topology_carve(V, (char *) topology);
    hipStream_t st = (hipStream_t) stream;
    double *a = (double *) workspace;
    for_flagged_runs(meshes, vertex_begin, n_meshes, [&](int64_t v0, int64_t v1) {
        hipLaunchKernelGGL(normals_adjoint_sum, dim3(grid(v1 - v0)), dim3(kBlock), 0, st, positions, V, tri, top.row, top.adj, v0, v1,
                           g_nrm, a);
        hipLaunchKernelGGL(normals_adjoint_positions, dim3(grid(v1 - v0)), dim3(kBlock), 0, st, positions, V, tri, top.row, top.adj,
                           v0, v1, (const double *) a, g_pos);
    });
    return launched(what);
}

int epsm_vertex_normals_forward(const float *positions, int64_t V, const uint32_t *tri, int64_t T, const void *topology,
                                const EpsmMesh *meshes, const int64_t *vertex_begin, int32_t n_meshes, const float *d_pos,
                                float *d_nrm, void *stream) {
    epsm_host::err_buf()[0] = 0;
    const char *what = "epsm_vertex_normals_forward";
    bool done;
    int rc = check_normals_derivative(what, V, T, n_meshes, positions && tri && d_pos && d_nrm, topology, meshes, vertex_begin, &done);
    if (rc != EPSM_OK || done) return rc;
    const Topology top = topology_carve(V, (char *) topology);
    hipStream_t st = (hipStream_t) stream;
    for_flagged_runs(meshes, vertex_begin, n_meshes, [&](int64_t v0, int64_t v1) {
        hipLaunchKernelGGL(normals_tangent, dim3(grid(v1 - v0)), dim3(kBlock), 0, st, positions, V, tri, top.row, top.adj, v0, v1, d_pos,
                           d_nrm);
    });
    return launched(what);
}

size_t epsm_emitter_tables_bytes(int64_t T, int32_t n_meshes) {
    if (T < 1) T = 1;
    if (n_meshes < 1) n_meshes = 1;
    return emitter_carve(T, n_meshes, nullptr, nullptr);
}

int epsm_emitter_tables(const float *positions, int64_t V, const uint32_t *tri, int64_t T, const EpsmMesh *meshes,
                        EpsmMesh *meshes_device, int32_t n_meshes, float *emitter_cdf, int64_t cdf_len,
                        void *workspace, size_t workspace_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    const char *what = "epsm_emitter_tables";
    if (T < 1 || T >= kMaxTriangles) return fail(EPSM_EINVAL, what, "T must be in 1 .. 2^28 - 1");
    if (V < 1 || V >= kMaxVertices) return fail(EPSM_EINVAL, what, "V must be in 1 .. 2^31 - 1");
    if (n_meshes < 0) return fail(EPSM_EINVAL, what, "n_meshes must be >= 0");
    if (cdf_len < 0) return fail(EPSM_EINVAL, what, "cdf_len must be >= 0");
    if (!positions || !tri || !emitter_cdf || !workspace || (n_meshes > 0 && (!meshes || !meshes_device)))
        return fail(EPSM_EINVAL, what, "NULL argument");
    if (workspace_bytes < epsm_emitter_tables_bytes(T, n_meshes))
        return fail(EPSM_EINVAL, what, "workspace smaller than epsm_emitter_tables_bytes(T, n_meshes)");
    if ((uintptr_t) workspace % 16) return fail(EPSM_EINVAL, what, "workspace must be 16-byte aligned");
    int rc = check_meshes(what, meshes, n_meshes, T);
    if (rc != EPSM_OK) return rc;
    int64_t chunks = 0;
    std::vector<std::pair<int64_t, int64_t>> cdf_ranges;
    for (int32_t m = 0; m < n_meshes; ++m) {
        if ((int64_t) meshes[m].cdf_begin + meshes[m].tri_count > cdf_len)
            return fail(EPSM_EINVAL, what, "a mesh's CDF range ends beyond cdf_len");
        if (meshes[m].tri_count) cdf_ranges.emplace_back(meshes[m].cdf_begin, meshes[m].tri_count);
        chunks += (meshes[m].tri_count + kChunk - 1) / kChunk;
    }
    if (ranges_overlap(cdf_ranges)) return fail(EPSM_EINVAL, what, "the meshes' CDF ranges overlap");
    if (n_meshes == 0) return EPSM_OK;
    hipStream_t st = (hipStream_t) stream;
    EmitterSpace w;
    emitter_carve(T, n_meshes, (char *) workspace, &w);
    const int cap = (int) chunk_capacity(T, n_meshes);
    hipLaunchKernelGGL(mesh_chunks, dim3(1), dim3(kBlock), 0, st, meshes_device, n_meshes, T, cdf_len, cap, w.chunk_begin);
    if (chunks > 0)
        hipLaunchKernelGGL(area_chunks, dim3((unsigned) chunks), dim3(kBlock), 0, st, positions, V, tri, T, meshes_device, n_meshes,
                           cdf_len, w);
    hipLaunchKernelGGL(mesh_totals, dim3(n_meshes), dim3(kBlock), 0, st, meshes_device, n_meshes, w);
    if (chunks > 0)
        hipLaunchKernelGGL(cdf_chunks, dim3((unsigned) chunks), dim3(kBlock), 0, st, meshes_device, n_meshes, T, cdf_len, w,
                           emitter_cdf);
    return launched(what);
}

size_t epsm_environment_tables_bytes(int32_t width, int32_t height) {
    if (width < 2) width = 2;
    if (height < 2) height = 2;
    return env_carve(width, height, nullptr, nullptr);
}

int epsm_environment_tables(const float *bitmap, int32_t width, int32_t height, float *texels, float *row_cdf, float *col_cdf,
                            float *cell_pdf, void *workspace, size_t workspace_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    const char *what = "epsm_environment_tables";
    if (width < 2 || height < 2) return fail(EPSM_EINVAL, what, "width and height must be >= 2");
    if ((int64_t) height * (width + 1) * 3 > kMaxEnvTexels) return fail(EPSM_EINVAL, what, "more than 2^26 texel values");
    if (!bitmap || !texels || !row_cdf || !col_cdf || !cell_pdf || !workspace) return fail(EPSM_EINVAL, what, "NULL argument");
    if (workspace_bytes < epsm_environment_tables_bytes(width, height))
        return fail(EPSM_EINVAL, what, "workspace smaller than epsm_environment_tables_bytes(width, height)");
    if ((uintptr_t) workspace % 16) return fail(EPSM_EINVAL, what, "workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
    EnvSpace s;
    env_carve(width, height, (char *) workspace, &s);
    const int64_t W = width, H = height;
    hipLaunchKernelGGL(env_texels, dim3(grid(H * (W + 1) * 3)), dim3(kBlock), 0, st, bitmap, width, height, texels);
    hipLaunchKernelGGL(env_rows, dim3(height - 1), dim3(kBlock), 0, st, bitmap, width, height, s);
    hipLaunchKernelGGL(env_row_cdf, dim3(1), dim3(kBlock), 0, st, height, s, row_cdf);
    hipLaunchKernelGGL(env_cells, dim3(grid((H - 1) * W)), dim3(kBlock), 0, st, width, height, s, col_cdf, cell_pdf);
    return launched(what);
}

}  // extern "C"
