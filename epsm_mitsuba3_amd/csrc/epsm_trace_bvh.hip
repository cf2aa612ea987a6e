// epsm_trace_bvh.hip -- gfx950 build and refit of the four-wide BVH (include/epsm_trace.h: epsm_bvh_build / epsm_bvh_refit).
//
// The same rules as the host builder (scene.py build_bvh), run top-down one binary level per launch:
//   presort    triangle boxes, a 30-bit Morton code of every centroid inside the scene's centroid bounds, one stable LSD
//              radix sort of the triangle ids by that code (4-bit digits, ranks within a wave by ballot);
//   split      one workgroup per node of the level: ranges of <= kLeafSize triangles are leaves; binned SAH (16 bins per axis
//              over the node's centroid extent, cost area(L) nL + area(R) nR) while d + 1 + ceil(log2 n) <= 32, a STABLE
//              partition by a block scan; otherwise, or without a plane, the middle of the range (still in Morton order);
//   collapse   one thread per wide node, one launch per wide level: the host's rule for opening binary children;
//   refit      one thread per wide node, one launch per wide level, deepest first (also the last step of the build).
// Float min / max go through order-preserving uint atomics (LDS and global), counts are integers, child indices come from
// scans: no float atomic adds, two builds of the same input are bit-identical.
#include <hip/hip_runtime.h>
#include <string.h>

#include "epsm_common.h"
#include "epsm_trace_scan.h"
#include "../../include/epsm_trace.h"

using epsm_host::fail;

namespace {

constexpr int kLeafSize = 6;             // scene.py LEAF_SIZE
constexpr int kBins = 16;                // scene.py _sah_split
constexpr int kMaxBinaryHeight = 32;     // scene.py kMaxBinaryHeight
constexpr int kMaxWideDepth = 16;        // scene.py kMaxWideDepth (kBvhStack = 3 x 16)
constexpr int kAbsent = 0x7fffffff;
constexpr int kSplitBlock = 512;         // split kernel: one workgroup per node
constexpr int kRadixPasses = 8;          // 32 bits >= the 30-bit Morton code
constexpr int64_t kMaxTriangles = int64_t(1) << 28;   // a leaf reference holds first << 3 in 31 bits

__device__ __forceinline__ unsigned f2u(float f) {     // order-preserving float -> uint
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float u2f(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

template <typename T>
__device__ __forceinline__ T wave_min(T v) {
    for (int o = 32; o > 0; o >>= 1) { const T w = __shfl_xor(v, o); v = w < v ? w : v; }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
    for (int o = 32; o > 0; o >>= 1) { const T w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}

struct BNode {                           // binary node over ids[a, b); left child at `left`, right at left + 1; -1: leaf
    int a, b, left, height;
};

// ------------------------------------------------------------------------------------------------ presort
struct Bounds { unsigned lo[3], hi[3]; };   // order-preserving uint images of the scene's centroid bounds

__global__ void init_bounds(Bounds *b) {
    for (int k = 0; k < 3; ++k) { b->lo[k] = 0xffffffffu; b->hi[k] = 0u; }
}

__global__ __launch_bounds__(kBlock) void tri_boxes(const float *pos, const uint32_t *tri, int64_t T, float4 *blo, float4 *bhi,
                                                     Bounds *cb) {
    const int64_t t = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    float c[3] = {__int_as_float(0x7f800000), __int_as_float(0x7f800000), __int_as_float(0x7f800000)};
    float d[3] = {-c[0], -c[1], -c[2]};
    if (t < T) {
        float lo[3], hi[3];
        for (int k = 0; k < 3; ++k) { lo[k] = pos[3 * (int64_t) tri[3 * t] + k]; hi[k] = lo[k]; }
        for (int v = 1; v < 3; ++v)
            for (int k = 0; k < 3; ++k) {
                const float p = pos[3 * (int64_t) tri[3 * t + v] + k];
                lo[k] = fminf(lo[k], p); hi[k] = fmaxf(hi[k], p);
            }
        blo[t] = make_float4(lo[0], lo[1], lo[2], 0.f);
        bhi[t] = make_float4(hi[0], hi[1], hi[2], 0.f);
        for (int k = 0; k < 3; ++k) { c[k] = d[k] = __fmul_rn(0.5f, __fadd_rn(lo[k], hi[k])); }
    }
    for (int k = 0; k < 3; ++k) {
        const unsigned l = wave_min(f2u(c[k])), h = wave_max(f2u(d[k]));
        if (lane_id() == 0) { atomicMin(&cb->lo[k], l); atomicMax(&cb->hi[k], h); }
    }
}

__device__ __forceinline__ unsigned spread10(unsigned x) {     // 10 bits -> every third bit
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__global__ __launch_bounds__(kBlock) void morton_codes(const float4 *blo, const float4 *bhi, int64_t T, const Bounds *cb,
                                                       uint32_t *keys, uint32_t *ids) {
    const int64_t t = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (t >= T) return;
    const float4 l = blo[t], h = bhi[t];
    const float c[3] = {__fmul_rn(0.5f, __fadd_rn(l.x, h.x)), __fmul_rn(0.5f, __fadd_rn(l.y, h.y)), __fmul_rn(0.5f, __fadd_rn(l.z, h.z))};
    unsigned code = 0;
    for (int k = 0; k < 3; ++k) {
        const float lo = u2f(cb->lo[k]), ext = __fsub_rn(u2f(cb->hi[k]), lo);
        float q = ext > 0.f ? __fmul_rn(__fsub_rn(c[k], lo), __fdiv_rn(1024.f, ext)) : 0.f;
        q = fminf(fmaxf(q, 0.f), 1023.f);
        code |= spread10((unsigned) q) << (2 - k);
    }
    keys[t] = code;
    ids[t] = (uint32_t) t;
}

// ------------------------------------------------------------------------------------------------ binary levels
struct SplitArgs {
    const float4 *blo, *bhi;
    uint32_t *ids, *tmp;
    BNode *bn;
    int level_begin, depth;
    int *split;                          // per node of the level: 1 = inner (two children)
    int *mid;                            // per node of the level: size of the left child
};

__device__ __forceinline__ float centroid(const float4 &l, const float4 &h, int k) {
    const float a = k == 0 ? l.x : k == 1 ? l.y : l.z, b = k == 0 ? h.x : k == 1 ? h.y : h.z;
    return __fmul_rn(0.5f, __fadd_rn(a, b));
}

__device__ __forceinline__ int bin_of(float c, float lo, float scale) {
    const int b = (int) __fmul_rn(__fsub_rn(c, lo), scale);
    return b < kBins - 1 ? (b > 0 ? b : 0) : kBins - 1;
}

__device__ __forceinline__ float half_area(const float *lo, const float *hi) {
    const float d0 = fmaxf(hi[0] - lo[0], 0.f), d1 = fmaxf(hi[1] - lo[1], 0.f), d2 = fmaxf(hi[2] - lo[2], 0.f);
    return __fadd_rn(__fadd_rn(__fmul_rn(d0, d1), __fmul_rn(d1, d2)), __fmul_rn(d2, d0));
}

__global__ __launch_bounds__(kSplitBlock) void split_level(SplitArgs A) {
    __shared__ unsigned cmin[3], cmax[3];
    __shared__ int cnt[3][kBins];
    __shared__ unsigned blo_u[3][kBins][3], bhi_u[3][kBins][3];
    __shared__ int choice[2];
    __shared__ int wsum[kSplitBlock / 64 + 1];
    const int local = blockIdx.x, node = A.level_begin + local;
    const BNode nd = A.bn[node];
    const int a = nd.a, b = nd.b, n = b - a, tid = threadIdx.x;
    if (n <= kLeafSize) {
        if (tid == 0) { A.split[local] = 0; A.mid[local] = 0; }
        return;
    }
    const int clog = 32 - __clz(n - 1);
    const bool sah = A.depth + 1 + clog <= kMaxBinaryHeight;
    if (tid == 0) { choice[0] = -1; choice[1] = 0; }
    if (sah) {
        if (tid < 3) { cmin[tid] = 0xffffffffu; cmax[tid] = 0u; }
        for (int j = tid; j < 3 * kBins; j += kSplitBlock) {
            (&cnt[0][0])[j] = 0;
            for (int k = 0; k < 3; ++k) { (&blo_u[0][0][0])[3 * j + k] = 0xffffffffu; (&bhi_u[0][0][0])[3 * j + k] = 0u; }
        }
        __syncthreads();
        unsigned l[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, h[3] = {0u, 0u, 0u};
        for (int i = a + tid; i < b; i += kSplitBlock) {
            const uint32_t t = A.ids[i];
            const float4 lo = A.blo[t], hi = A.bhi[t];
            for (int k = 0; k < 3; ++k) { const unsigned u = f2u(centroid(lo, hi, k)); l[k] = min(l[k], u); h[k] = max(h[k], u); }
        }
        for (int k = 0; k < 3; ++k) {
            const unsigned wl = wave_min(l[k]), wh = wave_max(h[k]);
            if (lane_id() == 0) { atomicMin(&cmin[k], wl); atomicMax(&cmax[k], wh); }
        }
        __syncthreads();
        float clo[3], scale[3];
        bool live[3];
        for (int k = 0; k < 3; ++k) {
            clo[k] = u2f(cmin[k]);
            const float ext = __fsub_rn(u2f(cmax[k]), clo[k]);
            live[k] = ext > 0.f;
            scale[k] = live[k] ? __fdiv_rn((float) kBins, ext) : 0.f;
        }
        for (int i = a + tid; i < b; i += kSplitBlock) {
            const uint32_t t = A.ids[i];
            const float4 lo = A.blo[t], hi = A.bhi[t];
            const float tl[3] = {lo.x, lo.y, lo.z}, th[3] = {hi.x, hi.y, hi.z};
            for (int ax = 0; ax < 3; ++ax) {
                if (!live[ax]) continue;
                const int bi = bin_of(centroid(lo, hi, ax), clo[ax], scale[ax]);
                atomicAdd(&cnt[ax][bi], 1);
                for (int k = 0; k < 3; ++k) { atomicMin(&blo_u[ax][bi][k], f2u(tl[k])); atomicMax(&bhi_u[ax][bi][k], f2u(th[k])); }
            }
        }
        __syncthreads();
        if (tid == 0) {                  // scene.py _sah_split: first minimum per axis, an axis wins only by a strictly lower cost
            float best = __int_as_float(0x7f800000);
            for (int ax = 0; ax < 3; ++ax) {
                if (!live[ax]) continue;
                float rlo[kBins][3], rhi[kBins][3];
                const float inf = __int_as_float(0x7f800000);
                float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
                for (int q = kBins - 1; q >= 0; --q) {
                    for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], u2f(blo_u[ax][q][k])); hi[k] = fmaxf(hi[k], u2f(bhi_u[ax][q][k])); }
                    for (int k = 0; k < 3; ++k) { rlo[q][k] = lo[k]; rhi[q][k] = hi[k]; }
                }
                for (int k = 0; k < 3; ++k) { lo[k] = inf; hi[k] = -inf; }
                int nl = 0, kbest = -1;
                float cbest = inf;
                for (int q = 0; q < kBins - 1; ++q) {
                    for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], u2f(blo_u[ax][q][k])); hi[k] = fmaxf(hi[k], u2f(bhi_u[ax][q][k])); }
                    nl += cnt[ax][q];
                    if (nl <= 0 || nl >= n) continue;
                    const float cost = __fadd_rn(__fmul_rn(half_area(lo, hi), (float) nl),
                                                 __fmul_rn(half_area(rlo[q + 1], rhi[q + 1]), (float) (n - nl)));
                    if (kbest < 0 || cost < cbest) { cbest = cost; kbest = q; }
                }
                if (kbest >= 0 && cbest < best) {
                    best = cbest;
                    int left = 0;
                    for (int q = 0; q <= kbest; ++q) left += cnt[ax][q];
                    choice[0] = ax * kBins + kbest; choice[1] = left;
                }
            }
        }
        __syncthreads();
    } else {
        __syncthreads();
    }
    const int ch = choice[0];
    int m = n / 2;
    if (ch >= 0) {                       // stable partition: bins <= kb to the left, in order; the rest behind them, in order
        const int ax = ch / kBins, kb = ch % kBins, nL = choice[1];
        const float clo = u2f(cmin[ax]), scale = __fdiv_rn((float) kBins, __fsub_rn(u2f(cmax[ax]), clo));
        int baseL = 0;
        for (int i0 = a; i0 < b; i0 += kSplitBlock) {
            const int i = i0 + tid;
            uint32_t t = 0;
            int isl = 0;
            if (i < b) {
                t = A.ids[i];
                isl = bin_of(centroid(A.blo[t], A.bhi[t], ax), clo, scale) <= kb;
            }
            int tot;
            const int r = block_exclusive_scan(isl, wsum, &tot);
            if (i < b) A.tmp[isl ? a + baseL + r : a + nL + (i0 - a - baseL) + (tid - r)] = t;
            baseL += tot;
        }
        __syncthreads();
        for (int i = a + tid; i < b; i += kSplitBlock) A.ids[i] = A.tmp[i];
        m = nL;
    }
    if (tid == 0) { A.split[local] = 1; A.mid[local] = m; }
}

__global__ __launch_bounds__(kBlock) void emit_children(BNode *bn, int level_begin, int level_n, int next_begin, const int *split,
                                                        const int *mid, const int *off) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= level_n) return;
    BNode &p = bn[level_begin + i];
    if (!split[i]) { p.left = -1; return; }
    const int c = next_begin + 2 * off[i];
    p.left = c;
    bn[c] = BNode{p.a, p.a + mid[i], -1, 0};
    bn[c + 1] = BNode{p.a + mid[i], p.b, -1, 0};
}

// bottom-up: boxes (for the collapse's half-areas) and heights of one binary level
__global__ __launch_bounds__(kBlock) void binary_boxes(BNode *bn, float4 *nlo, float4 *nhi, int begin, int count, const uint32_t *ids,
                                                       const float4 *blo, const float4 *bhi) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const int j = begin + i;
    BNode nd = bn[j];
    float4 lo, hi;
    if (nd.left < 0) {
        lo = blo[ids[nd.a]]; hi = bhi[ids[nd.a]];
        for (int q = nd.a + 1; q < nd.b; ++q) {
            const float4 l = blo[ids[q]], h = bhi[ids[q]];
            lo.x = fminf(lo.x, l.x); lo.y = fminf(lo.y, l.y); lo.z = fminf(lo.z, l.z);
            hi.x = fmaxf(hi.x, h.x); hi.y = fmaxf(hi.y, h.y); hi.z = fmaxf(hi.z, h.z);
        }
        nd.height = 0;
    } else {
        const float4 l0 = nlo[nd.left], l1 = nlo[nd.left + 1], h0 = nhi[nd.left], h1 = nhi[nd.left + 1];
        lo = make_float4(fminf(l0.x, l1.x), fminf(l0.y, l1.y), fminf(l0.z, l1.z), 0.f);
        hi = make_float4(fmaxf(h0.x, h1.x), fmaxf(h0.y, h1.y), fmaxf(h0.z, h1.z), 0.f);
        nd.height = 1 + max(bn[nd.left].height, bn[nd.left + 1].height);
    }
    nlo[j] = lo; nhi[j] = hi;
    bn[j].height = nd.height;
}

// ------------------------------------------------------------------------------------------------ four-wide collapse
__global__ __launch_bounds__(kBlock) void collapse_pick(const BNode *bn, const float4 *nlo, const float4 *nhi, const int *wide_bin,
                                                        int begin, int count, int wide_depth, int4 *kids_out, int *inner) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const int allowed = 2 * (kMaxWideDepth - 1 - wide_depth);
    const BNode root = bn[wide_bin[begin + i]];
    int kids[4] = {root.left, root.left + 1, -1, -1}, nk = 2;
    while (nk < 4) {                     // scene.py build_bvh: open the tallest child if one is too tall, else the largest box
        int pick = -1, ph = -1;
        float pa = 0.f;
        bool any_tall = false;
        for (int s = 0; s < nk; ++s) {
            const BNode c = bn[kids[s]];
            if (c.left < 0) continue;
            if (c.height > allowed) {
                if (!any_tall || c.height > ph) { pick = s; ph = c.height; }
                any_tall = true;
            } else if (!any_tall) {
                const float4 l = nlo[kids[s]], h = nhi[kids[s]];
                const float lo[3] = {l.x, l.y, l.z}, hi[3] = {h.x, h.y, h.z};
                const float ha = half_area(lo, hi);
                if (pick < 0 || ha > pa) { pick = s; pa = ha; }
            }
        }
        if (pick < 0) break;
        const int k = kids[pick];
        for (int s = nk; s > pick + 1; --s) kids[s] = kids[s - 1];
        kids[pick] = bn[k].left; kids[pick + 1] = bn[k].left + 1;
        ++nk;
    }
    int ni = 0;
    for (int s = 0; s < nk; ++s) ni += bn[kids[s]].left >= 0;
    kids_out[i] = make_int4(kids[0], kids[1], kids[2], kids[3]);
    inner[i] = ni;
}

__global__ __launch_bounds__(kBlock) void collapse_emit(const BNode *bn, int *wide_bin, int begin, int count, const int4 *kids_in,
                                                        const int *off, EpsmBvhNode *nodes) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const int4 k4 = kids_in[i];
    const int kids[4] = {k4.x, k4.y, k4.z, k4.w};
    int next = begin + count + off[i];
    EpsmBvhNode &o = nodes[begin + i];
    for (int s = 0; s < 4; ++s) {
        int c = kAbsent, n = 0;
        if (kids[s] >= 0) {
            const BNode k = bn[kids[s]];
            if (k.left < 0) { n = k.b - k.a; c = ~((k.a << 3) | n); }
            else { c = next; wide_bin[next++] = kids[s]; }
        }
        o.c[s] = c; o.n[s] = n;
    }
}

__global__ void single_leaf(EpsmBvhNode *nodes, int T) {
    EpsmBvhNode &o = nodes[0];
    for (int s = 0; s < 4; ++s) { o.c[s] = s == 0 ? ~(0 << 3 | T) : kAbsent; o.n[s] = s == 0 ? T : 0; }
}

__global__ void set_int(int *p, int v) { *p = v; }

// ------------------------------------------------------------------------------------------------ refit
__global__ __launch_bounds__(kBlock) void gather_tri_verts(const float *pos, const uint32_t *tri, const uint32_t *prim, int64_t T,
                                                           float *tv) {
    const int64_t j = (int64_t) blockIdx.x * kBlock + threadIdx.x;
    if (j >= T) return;
    const int64_t t = prim[j];
    for (int v = 0; v < 3; ++v) {
        const int64_t p = tri[3 * t + v];
        for (int k = 0; k < 3; ++k) tv[9 * j + 3 * v + k] = pos[3 * p + k];
    }
}

__device__ __forceinline__ float pad_lo(float lo) {   // DeviceBvh.refit: lo - 1e-6 (1 + |lo|), rounded step by step as torch does
    return __fsub_rn(lo, __fmul_rn(__fadd_rn(fabsf(lo), 1.0f), 1e-6f));
}
__device__ __forceinline__ float pad_hi(float hi) {
    return __fadd_rn(hi, __fmul_rn(__fadd_rn(fabsf(hi), 1.0f), 1e-6f));
}

__global__ __launch_bounds__(kBlock) void refit_level(EpsmBvhNode *nodes, int begin, int count, const float *tv) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    EpsmBvhNode &o = nodes[begin + i];
    const float inf = __int_as_float(0x7f800000);
    for (int s = 0; s < 4; ++s) {
        const int c = o.c[s];
        float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
        if (c == kAbsent) {
        } else if (c < 0) {
            const int first = (~c) >> 3, n = (~c) & 7;
            for (int q = first; q < first + n; ++q)
                for (int v = 0; v < 3; ++v)
                    for (int k = 0; k < 3; ++k) {
                        const float p = tv[9 * (int64_t) q + 3 * v + k];
                        lo[k] = fminf(lo[k], p); hi[k] = fmaxf(hi[k], p);
                    }
            for (int k = 0; k < 3; ++k) { lo[k] = pad_lo(lo[k]); hi[k] = pad_hi(hi[k]); }
        } else {
            const EpsmBvhNode &ch = nodes[c];
            for (int q = 0; q < 4; ++q) {
                lo[0] = fminf(lo[0], ch.lox[q]); lo[1] = fminf(lo[1], ch.loy[q]); lo[2] = fminf(lo[2], ch.loz[q]);
                hi[0] = fmaxf(hi[0], ch.hix[q]); hi[1] = fmaxf(hi[1], ch.hiy[q]); hi[2] = fmaxf(hi[2], ch.hiz[q]);
            }
        }
        o.lox[s] = lo[0]; o.loy[s] = lo[1]; o.loz[s] = lo[2];
        o.hix[s] = hi[0]; o.hiy[s] = hi[1]; o.hiz[s] = hi[2];
    }
}

// ------------------------------------------------------------------------------------------------ workspace
struct Workspace {
    float4 *blo, *bhi, *nlo, *nhi;
    uint32_t *keys0, *keys1, *ids0, *ids1;
    BNode *bn;
    int4 *kids;
    int *flag, *off, *aux, *wide_bin, *scan_scratch, *total;
};

constexpr size_t kAlign = 256;
size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

int64_t scan_capacity(int64_t T) { return T + 16 * ((T + kBlock - 1) / kBlock) + 1; }

size_t carve(int64_t T, char *base, Workspace *w) {
    const int64_t NB = 2 * T;            // binary nodes: <= 2 T - 1
    const int64_t SC = scan_capacity(T);
    size_t o = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + o : nullptr; o += align_up(bytes); return (void *) p; };
    Workspace x;
    x.blo = (float4 *) take(16 * T); x.bhi = (float4 *) take(16 * T);
    x.nlo = (float4 *) take(16 * NB); x.nhi = (float4 *) take(16 * NB);
    x.keys0 = (uint32_t *) take(4 * T); x.keys1 = (uint32_t *) take(4 * T);
    x.ids0 = (uint32_t *) take(4 * T); x.ids1 = (uint32_t *) take(4 * T);
    x.bn = (BNode *) take(sizeof(BNode) * NB);
    x.kids = (int4 *) take(16 * T);
    x.flag = (int *) take(4 * SC); x.off = (int *) take(4 * SC); x.aux = (int *) take(4 * T);
    x.wide_bin = (int *) take(4 * T);
    x.scan_scratch = (int *) take(4 * scan_scratch_ints(SC));
    x.total = (int *) take(4 * 16);
    if (w) *w = x;
    return o;
}

int read_total(const int *d_total, hipStream_t st, int *h, const char *what) {
    hipError_t e = hipMemcpyAsync(h, d_total, sizeof(int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return epsm_host::hip_fail(what, e);
    return EPSM_OK;
}

unsigned grid(int64_t n, int per = kBlock) { return (unsigned) ((n + per - 1) / per); }

int refit_impl(const float *positions, const uint32_t *tri, const uint32_t *prim_index, int64_t T, EpsmBvhNode *nodes,
               const int32_t *level_begin, int32_t n_levels, float *tri_verts, hipStream_t st) {
    hipLaunchKernelGGL(gather_tri_verts, dim3(grid(T)), dim3(kBlock), 0, st, positions, tri, prim_index, T, tri_verts);
    for (int l = n_levels - 1; l >= 0; --l) {
        const int cnt = level_begin[l + 1] - level_begin[l];
        if (cnt > 0) hipLaunchKernelGGL(refit_level, dim3(grid(cnt)), dim3(kBlock), 0, st, nodes, level_begin[l], cnt, tri_verts);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? EPSM_OK : epsm_host::hip_fail("epsm_bvh_refit", e);
}

}  // namespace

extern "C" {

int64_t epsm_bvh_max_nodes(int64_t T) { return T > 1 ? T - 1 : 1; }

size_t epsm_bvh_workspace_bytes(int64_t T) {
    if (T < 1) T = 1;
    return carve(T, nullptr, nullptr);
}

int epsm_bvh_build(const float *positions, int64_t V, const uint32_t *tri, int64_t T,
                   EpsmBvhNode *nodes, uint32_t *prim_index, float *tri_verts,
                   int32_t *n_nodes, int32_t *level_begin, int32_t *n_levels,
                   void *workspace, size_t workspace_bytes, void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (T < 1) return fail(EPSM_EINVAL, "epsm_bvh_build: T must be >= 1");
    if (T >= kMaxTriangles) return fail(EPSM_EINVAL, "epsm_bvh_build: T must be < 2^28 (leaf references hold first << 3 in 31 bits)");
    if (V < 1) return fail(EPSM_EINVAL, "epsm_bvh_build: V must be >= 1");
    if (!positions || !tri || !nodes || !prim_index || !tri_verts || !n_nodes || !level_begin || !n_levels || !workspace)
        return fail(EPSM_EINVAL, "epsm_bvh_build: NULL argument");
    if (workspace_bytes < epsm_bvh_workspace_bytes(T))
        return fail(EPSM_EINVAL, "epsm_bvh_build: workspace smaller than epsm_bvh_workspace_bytes(T)");
    if ((uintptr_t) workspace % 16) return fail(EPSM_EINVAL, "epsm_bvh_build: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t) stream;
    Workspace w;
    carve(T, (char *) workspace, &w);
    int rc;

    // presort: boxes, Morton codes, stable radix sort of the ids
    Bounds *cb = (Bounds *) w.total;
    hipLaunchKernelGGL(init_bounds, dim3(1), dim3(1), 0, st, cb);
    hipLaunchKernelGGL(tri_boxes, dim3(grid(T)), dim3(kBlock), 0, st, positions, tri, T, w.blo, w.bhi, cb);
    hipLaunchKernelGGL(morton_codes, dim3(grid(T)), dim3(kBlock), 0, st, w.blo, w.bhi, T, cb, w.keys0, w.ids0);
    const int tiles = (int) grid(T);
    uint32_t *kin = w.keys0, *vin = w.ids0, *kout = w.keys1, *vout = w.ids1;
    for (int p = 0; p < kRadixPasses; ++p) {
        hipLaunchKernelGGL(radix_hist, dim3(tiles), dim3(kBlock), 0, st, kin, T, p * kRadixBits, w.flag, tiles);
        exclusive_scan(w.flag, w.off, 16 * tiles, w.total + 8, w.scan_scratch, st);
        hipLaunchKernelGGL(radix_scatter, dim3(tiles), dim3(kBlock), 0, st, kin, vin, kout, vout, T, p * kRadixBits, w.off, tiles);
        uint32_t *t = kin; kin = kout; kout = t;
        t = vin; vin = vout; vout = t;
    }
    uint32_t *ids = vin, *tmp = vout;    // an even number of passes: back in ids0

    // binary tree, one level per launch; node ranges of a level are contiguous in w.bn
    {
        BNode root{0, (int) T, -1, 0};
        hipError_t e = hipMemcpyAsync(w.bn, &root, sizeof(BNode), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return epsm_host::hip_fail("epsm_bvh_build", e);
    }
    int blev[kMaxBinaryHeight + 2];
    int nblev = 0, begin = 0, count = 1;
    blev[0] = 0;
    for (int depth = 0; count > 0; ++depth) {
        if (depth > kMaxBinaryHeight) return fail(EPSM_ELAUNCH, "epsm_bvh_build: binary tree deeper than 32 levels (internal error)");
        SplitArgs A{w.blo, w.bhi, ids, tmp, w.bn, begin, depth, w.flag, w.aux};
        hipLaunchKernelGGL(split_level, dim3(count), dim3(kSplitBlock), 0, st, A);
        exclusive_scan(w.flag, w.off, count, w.total + 8, w.scan_scratch, st);
        hipLaunchKernelGGL(emit_children, dim3(grid(count)), dim3(kBlock), 0, st, w.bn, begin, count, begin + count, w.flag, w.aux, w.off);
        int inner = 0;
        if ((rc = read_total(w.total + 8, st, &inner, "epsm_bvh_build")) != EPSM_OK) return rc;
        begin += count;
        count = 2 * inner;
        blev[++nblev] = begin;
    }
    for (int l = nblev - 1; l >= 0; --l)
        hipLaunchKernelGGL(binary_boxes, dim3(grid(blev[l + 1] - blev[l])), dim3(kBlock), 0, st, w.bn, w.nlo, w.nhi, blev[l],
                           blev[l + 1] - blev[l], ids, w.blo, w.bhi);

    // four-wide collapse, one wide level per launch
    int nl = 0, wb = 0, wc = 1;
    level_begin[0] = 0;
    if (nblev == 1) {                    // T <= 6: node 0 holds one leaf in slot 0
        hipLaunchKernelGGL(single_leaf, dim3(1), dim3(1), 0, st, nodes, (int) T);
        nl = 1;
        level_begin[1] = 1;
    } else {
        hipLaunchKernelGGL(set_int, dim3(1), dim3(1), 0, st, w.wide_bin, 0);
        while (wc > 0) {
            if (nl >= kMaxWideDepth) return fail(EPSM_ELAUNCH, "epsm_bvh_build: more than 16 wide levels (internal error)");
            hipLaunchKernelGGL(collapse_pick, dim3(grid(wc)), dim3(kBlock), 0, st, w.bn, w.nlo, w.nhi, w.wide_bin, wb, wc, nl, w.kids, w.flag);
            exclusive_scan(w.flag, w.off, wc, w.total + 8, w.scan_scratch, st);
            hipLaunchKernelGGL(collapse_emit, dim3(grid(wc)), dim3(kBlock), 0, st, w.bn, w.wide_bin, wb, wc, w.kids, w.off, nodes);
            int next = 0;
            if ((rc = read_total(w.total + 8, st, &next, "epsm_bvh_build")) != EPSM_OK) return rc;
            wb += wc;
            wc = next;
            level_begin[++nl] = wb;
        }
    }
    hipError_t e = hipMemcpyAsync(prim_index, ids, 4 * T, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return epsm_host::hip_fail("epsm_bvh_build", e);
    *n_nodes = level_begin[nl];
    *n_levels = nl;
    // boxes and tri_verts by the refit that later updates them
    if ((rc = refit_impl(positions, tri, prim_index, T, nodes, level_begin, nl, tri_verts, st)) != EPSM_OK) return rc;
    e = hipStreamSynchronize(st);
    return e == hipSuccess ? EPSM_OK : epsm_host::hip_fail("epsm_bvh_build", e);
}

int epsm_bvh_refit(const float *positions, int64_t V, const uint32_t *tri, const uint32_t *prim_index, int64_t T,
                   EpsmBvhNode *nodes, int32_t n_nodes, const int32_t *level_begin, int32_t n_levels,
                   float *tri_verts, void *stream) {
    epsm_host::err_buf()[0] = 0;
    if (T < 1) return fail(EPSM_EINVAL, "epsm_bvh_refit: T must be >= 1");
    if (T >= kMaxTriangles) return fail(EPSM_EINVAL, "epsm_bvh_refit: T must be < 2^28");
    if (V < 1) return fail(EPSM_EINVAL, "epsm_bvh_refit: V must be >= 1");
    if (!positions || !tri || !prim_index || !nodes || !level_begin || !tri_verts)
        return fail(EPSM_EINVAL, "epsm_bvh_refit: NULL argument");
    if (n_levels < 1 || n_levels > kMaxWideDepth) return fail(EPSM_EINVAL, "epsm_bvh_refit: n_levels must be in 1..16");
    if (n_nodes < 1 || level_begin[0] != 0 || level_begin[n_levels] != n_nodes)
        return fail(EPSM_EINVAL, "epsm_bvh_refit: level_begin must run from 0 to n_nodes");
    for (int l = 0; l < n_levels; ++l)
        if (level_begin[l + 1] < level_begin[l]) return fail(EPSM_EINVAL, "epsm_bvh_refit: level_begin must not decrease");
    return refit_impl(positions, tri, prim_index, T, nodes, level_begin, n_levels, tri_verts, (hipStream_t) stream);
}

}  // extern "C"
