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
#include "../../include/epsm_trace.h"

using epsm_host::fail;

namespace {

constexpr int kChunk = 4 * kBlock;                     // triangles per workgroup of the area scan
constexpr int64_t kMaxTriangles = int64_t(1) << 28;    // 3 T corner entries and their sort offsets stay in int32
constexpr int64_t kMaxVertices = int64_t(1) << 31;
constexpr int kMaxEnvTexels = 1 << 26;                 // H (W + 1) 3 stays in int32

constexpr size_t kAlign = 256;
size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }
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
struct Topology { uint32_t *row, *adj; };               // row (V + 1), adj (3 T): corner entries 3 t + c

Topology topology_carve(int64_t V, char *base) {
    return Topology{(uint32_t *) base, base ? (uint32_t *) (base + align_up(4 * (size_t) (V + 1))) : nullptr};
}
size_t topology_size(int64_t V, int64_t T) { return align_up(4 * (size_t) (V + 1)) + align_up(12 * (size_t) T); }

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
