// epsm_scene_driver.cpp -- the whole route of a traced scene from C++ through the C ABI (no Python in the process): read a scene
// bundle of plain parameters, build the BVH and the scene tables on the device, render the primal image, run render_backward
// as the Python route does with the wavefront tracer, move the named meshes (an emitting one included) on the device and run
// render_backward again.  Prints per-phase milliseconds (HIP events) and OK.
//   make -C examples && examples/build/epsm_scene_driver <bundle> <output directory>
//
// Scene bundle: little-endian, packed, no padding; i32 = int32, u32 = uint32, f32 = float, f64 = double.
//   char[8]  "EPSMSCN1"
//   i32      n_meshes, n_bsdfs, n_emitters, n_sensors
//   n_bsdfs times     i32 type (EPSM_BSDF_*_T), twosided, distr (EPSM_DISTR_*), sample_visible
//                     f32 reflectance[3], alpha, eta[3], k[3], int_ior, ext_ior
//                     i32 alpha_slot (-1: roughness not optimised; slots are 0 .. B - 1)
//   n_emitters times  i32 type (EPSM_EMITTER_AREA or _POINT), mesh; f32 radiance[3], position[3]
//   n_sensors times   f64 to_world[16] (row-major 4x4 camera-to-world), fov_x (degrees), near_clip, far_clip
//                     i32 width, height, rfilter (EPSM_RFILTER_*)    (no crop window, no sample border)
//   n_meshes times    i32 n_vertices, n_triangles; u32 flags (EPSM_MESH_*: a mesh flagged EPSM_MESH_VERTEX_NORMALS gets the
//                     angle-weighted normals of epsm_vertex_normals); i32 bsdf, emitter (-1: none), moves (1: translated in
//                     step 4); f32 positions[n_vertices][3]; i32 faces[n_triangles][3] (indices into this mesh's vertices)
//   run               i32 variant (0 manifold, 1 manifold_caustic), seed, primal_sensor, primal_spp, backward_sensor,
//                     backward_spp, max_depth (>= 4: the first-hit fusion has no occluder record), rr_depth, max_log_depth
//                     f32 clip (outlier clamp of calc_grad), translation[3] (added to the positions of every mesh with moves = 1)
//   f32      grad_img[res][res][5]   the gradient image of the backward pass, res = the backward sensor's width (= its height)
// Output directory: sensor_primal.bin, sensor_backward.bin (the EpsmSensor structs), image.bin (height, width, 3) f32, and
// grads_before.bin / grads_after.bin: f32 [grad_pos (V,3) | grad_nrm (V,3) | grad_alpha (B) | d / d camera origin (3)], V the
// vertices of all meshes in bundle order.  The environment is empty (no constant or envmap emitter), no textures.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "epsm.h"
#include "epsm_trace.h"

#define HIP_OK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); }  \
    } while (0)
#define EPSM_OK_OR_DIE(x)                                                                           \
    do {                                                                                            \
        int rc_ = (x);                                                                              \
        if (rc_ != 0) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, epsm_last_error()); exit(3); }   \
    } while (0)

namespace {

struct Reader {
    FILE *f;
    template <class T> T get() {
        T v;
        if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "bundle: truncated\n"); exit(4); }
        return v;
    }
    template <class T> void get(T *p, size_t n) {
        if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "bundle: truncated\n"); exit(4); }
    }
};

struct SensorDesc { double to_world[16], fov, near_clip, far_clip; int width, height, rfilter; };
struct MeshDesc { int nv, nt; uint32_t flags; int bsdf, emitter, moves; std::vector<float> v; std::vector<int32_t> f; };

// ---- the camera matrices as Sensor.c_struct computes them: in double, rounded to float once
typedef double M4[4][4];
void mat_mul(const M4 a, const M4 b, M4 o) {
    M4 t;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[i][k] * b[k][j];
            t[i][j] = s;
        }
    memcpy(o, t, sizeof(M4));
}
bool mat_inv(const M4 a, M4 o) {                // Gauss-Jordan with partial pivoting
    double m[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 8; ++j) m[i][j] = j < 4 ? a[i][j] : (j - 4 == i ? 1.0 : 0.0);
    for (int c = 0; c < 4; ++c) {
        int p = c;
        for (int r = c + 1; r < 4; ++r)
            if (fabs(m[r][c]) > fabs(m[p][c])) p = r;
        if (m[p][c] == 0.0) return false;
        for (int j = 0; j < 8; ++j) { double t = m[c][j]; m[c][j] = m[p][j]; m[p][j] = t; }
        const double d = m[c][c];
        for (int j = 0; j < 8; ++j) m[c][j] /= d;
        for (int r = 0; r < 4; ++r)
            if (r != c) {
                const double s = m[r][c];
                for (int j = 0; j < 8; ++j) m[r][j] -= s * m[c][j];
            }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) o[i][j] = m[i][j + 4];
    return true;
}
void xform_point(const M4 m, const double p[3], double o[3]) {
    double q[4];
    for (int i = 0; i < 4; ++i) q[i] = m[i][0] * p[0] + m[i][1] * p[1] + m[i][2] * p[2] + m[i][3];
    for (int i = 0; i < 3; ++i) o[i] = q[i] / q[3];
}

EpsmSensor sensor_struct(const SensorDesc &d) {   // perspective_projection + Sensor.c_struct (scene.py)
    const double aspect = (double) d.width / d.height, recip = 1.0 / (d.far_clip - d.near_clip);
    const double cot = 1.0 / tan(d.fov * 0.5 * M_PI / 180.0);
    M4 persp = {{cot, 0, 0, 0}, {0, cot, 0, 0}, {0, 0, d.far_clip * recip, -d.near_clip * d.far_clip * recip}, {0, 0, 1, 0}};
    M4 sc = {{-0.5, 0, 0, 0}, {0, -0.5 * aspect, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    M4 tr = {{1, 0, 0, -1.0}, {0, 1, 0, -1.0 / aspect}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    M4 c2s, s2c;
    mat_mul(sc, tr, c2s);
    mat_mul(c2s, persp, c2s);
    if (!mat_inv(c2s, s2c)) { fprintf(stderr, "sensor: singular projection\n"); exit(4); }
    EpsmSensor s;
    memset(&s, 0, sizeof(s));
    for (int i = 0; i < 12; ++i) s.to_world[i] = (float) d.to_world[i];
    for (int i = 0; i < 16; ++i) s.sample_to_camera[i] = (float) s2c[i / 4][i % 4];
    const double o[3] = {0, 0, 0}, ux[3] = {1.0 / d.width, 0, 0}, uy[3] = {0, 1.0 / d.height, 0};
    double p0[3], px[3], py[3];
    xform_point(s2c, o, p0); xform_point(s2c, ux, px); xform_point(s2c, uy, py);
    for (int k = 0; k < 3; ++k) { s.dx[k] = (float) (px[k] - p0[k]); s.dy[k] = (float) (py[k] - p0[k]); }
    s.near_clip = (float) d.near_clip; s.far_clip = (float) d.far_clip;
    s.width = d.width; s.height = d.height; s.border = 0;
    return s;
}

template <class T> T *dev_alloc(size_t n) {
    void *p = nullptr;
    HIP_OK(hipMalloc(&p, n * sizeof(T) > 0 ? n * sizeof(T) : 16));
    return (T *) p;
}
template <class T> T *dev_copy(const std::vector<T> &h) {
    T *p = dev_alloc<T>(h.size());
    if (!h.empty()) HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return p;
}

void write_file(const std::string &path, const void *p, size_t bytes) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(5); }
    fclose(f);
}

struct Timer {
    hipEvent_t a, b;
    hipStream_t st;
    explicit Timer(hipStream_t s) : st(s) { HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b)); HIP_OK(hipEventRecord(a, st)); }
    float ms() {
        HIP_OK(hipEventRecord(b, st));
        HIP_OK(hipEventSynchronize(b));
        float t = 0.f;
        HIP_OK(hipEventElapsedTime(&t, a, b));
        HIP_OK(hipEventDestroy(a)); HIP_OK(hipEventDestroy(b));
        return t;
    }
};

// tiles of a pass, as Scene.iter_traces / render_primal cut them for the wavefront tracer on one rank
int64_t tile_paths(int64_t n_total) {
    const int64_t lo = int64_t(1) << 20, hi = int64_t(1) << 24;
    return n_total < lo ? lo : (n_total > hi ? hi : n_total);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <bundle> <output directory>\n", argv[0]); return 1; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fprintf(stderr, "no HIP device\n"); return 1; }
    const std::string out = argv[2];

    // ---------------------------------------------------------------- the bundle
    FILE *bf = fopen(argv[1], "rb");
    if (!bf) { fprintf(stderr, "cannot open %s\n", argv[1]); return 4; }
    Reader rd{bf};
    char magic[8];
    rd.get(magic, 8);
    if (memcmp(magic, "EPSMSCN1", 8)) { fprintf(stderr, "bundle: bad magic\n"); return 4; }
    const int n_meshes = rd.get<int32_t>(), n_bsdfs = rd.get<int32_t>(), n_emitters = rd.get<int32_t>(), n_sensors = rd.get<int32_t>();
    if (n_meshes < 1 || n_bsdfs < 1 || n_emitters < 0 || n_sensors < 1) { fprintf(stderr, "bundle: bad counts\n"); return 4; }
    std::vector<EpsmBsdf> bsdfs(n_bsdfs);
    int B = 0;
    for (auto &b : bsdfs) {
        memset(&b, 0, sizeof(b));
        b.type = rd.get<int32_t>(); b.twosided = rd.get<int32_t>(); b.distr = rd.get<int32_t>(); b.sample_visible = rd.get<int32_t>();
        rd.get(b.reflectance, 3); b.alpha = rd.get<float>(); rd.get(b.eta, 3); rd.get(b.k, 3);
        b.int_ior = rd.get<float>(); b.ext_ior = rd.get<float>();
        b.alpha_slot = rd.get<int32_t>(); b.color_slot = -1; b.texture = -1;
        if (b.alpha_slot + 1 > B) B = b.alpha_slot + 1;
    }
    std::vector<EpsmEmitter> emitters(n_emitters > 0 ? n_emitters : 1);
    for (int i = 0; i < n_emitters; ++i) {
        EpsmEmitter &e = emitters[i];
        memset(&e, 0, sizeof(e));
        e.type = rd.get<int32_t>(); e.mesh = rd.get<int32_t>(); rd.get(e.radiance, 3); rd.get(e.position, 3); e.color_slot = -1;
    }
    std::vector<SensorDesc> sensors(n_sensors);
    for (auto &s : sensors) {
        rd.get(s.to_world, 16); s.fov = rd.get<double>(); s.near_clip = rd.get<double>(); s.far_clip = rd.get<double>();
        s.width = rd.get<int32_t>(); s.height = rd.get<int32_t>(); s.rfilter = rd.get<int32_t>();
    }
    std::vector<MeshDesc> meshes(n_meshes);
    for (auto &m : meshes) {
        m.nv = rd.get<int32_t>(); m.nt = rd.get<int32_t>(); m.flags = rd.get<uint32_t>();
        m.bsdf = rd.get<int32_t>(); m.emitter = rd.get<int32_t>(); m.moves = rd.get<int32_t>();
        if (m.nv < 1 || m.nt < 1 || m.bsdf < 0 || m.bsdf >= n_bsdfs || m.emitter >= n_emitters) { fprintf(stderr, "bundle: bad mesh\n"); return 4; }
        m.v.resize(3 * (size_t) m.nv); m.f.resize(3 * (size_t) m.nt);
        rd.get(m.v.data(), m.v.size()); rd.get(m.f.data(), m.f.size());
    }
    const int variant = rd.get<int32_t>();
    const uint32_t seed = (uint32_t) rd.get<int32_t>();
    const int primal_sensor = rd.get<int32_t>(), primal_spp = rd.get<int32_t>(), backward_sensor = rd.get<int32_t>();
    const int backward_spp = rd.get<int32_t>(), max_depth_in = rd.get<int32_t>(), rr_depth = rd.get<int32_t>();
    const int max_log_depth = rd.get<int32_t>();
    const float clip = rd.get<float>();
    float translation[3];
    rd.get(translation, 3);
    if (primal_sensor < 0 || primal_sensor >= n_sensors || backward_sensor < 0 || backward_sensor >= n_sensors) {
        fprintf(stderr, "bundle: bad sensor index\n"); return 4;
    }
    const SensorDesc &bsd = sensors[backward_sensor];
    if (bsd.width != bsd.height) { fprintf(stderr, "the backward sensor must be square\n"); return 4; }
    const int res = bsd.width;
    std::vector<float> grad_img((size_t) res * res * 5);
    rd.get(grad_img.data(), grad_img.size());
    fclose(bf);
    const int max_depth = max_depth_in < 0 ? 6 : (max_depth_in > 6 ? 6 : max_depth_in);     // Integrator.tracer_depth
    int K = max_log_depth < max_depth ? max_log_depth : max_depth;
    if (K > 5) K = 5;
    if (max_depth <= 3 || K < 1 || (variant != 0 && variant != 1)) {
        fprintf(stderr, "max_depth must be >= 4 (the first-hit fusion has no occluder record) and the variant 0 or 1\n"); return 4;
    }

    // ---------------------------------------------------------------- host tables (the layout of Scene._upload)
    std::vector<float> pos;
    std::vector<uint32_t> tri, tri_mesh, tri_table;
    std::vector<EpsmMesh> mesh_table(n_meshes);
    std::vector<int64_t> vertex_begin(1, 0);
    int64_t V = 0, T = 0;
    for (int i = 0; i < n_meshes; ++i) {
        const MeshDesc &m = meshes[i];
        EpsmMesh &c = mesh_table[i];
        memset(&c, 0, sizeof(c));
        c.tri_begin = (uint32_t) T; c.tri_count = (uint32_t) m.nt; c.flags = m.flags; c.bsdf = m.bsdf; c.emitter = m.emitter;
        c.cdf_begin = (uint32_t) T;
        const uint32_t mode = (m.flags & 0xFu) | ((uint32_t) (bsdfs[m.bsdf].alpha_slot + 1) << 8);
        for (int t = 0; t < m.nt; ++t) {
            for (int k = 0; k < 3; ++k) {
                const int32_t j = m.f[3 * t + k];
                if (j < 0 || j >= m.nv) { fprintf(stderr, "bundle: face index out of range\n"); return 4; }
                tri.push_back((uint32_t) (V + j)); tri_table.push_back((uint32_t) (V + j));
            }
            tri_table.push_back(mode);
            tri_mesh.push_back((uint32_t) i);
        }
        pos.insert(pos.end(), m.v.begin(), m.v.end());
        V += m.nv; T += m.nt;
        vertex_begin.push_back(V);
    }

    hipStream_t st;
    HIP_OK(hipStreamCreate(&st));
    float *d_pos = dev_copy(pos), *d_nrm = dev_alloc<float>(3 * V), *d_cdf = dev_alloc<float>(T);
    uint32_t *d_tri = dev_copy(tri), *d_tri_mesh = dev_copy(tri_mesh), *d_table = dev_copy(tri_table);
    EpsmMesh *d_meshes = dev_copy(mesh_table);
    EpsmBsdf *d_bsdfs = dev_copy(bsdfs);
    EpsmEmitter *d_emitters = dev_copy(emitters);
    float *d_grad_img = dev_copy(grad_img);
    HIP_OK(hipMemset(d_nrm, 0, 3 * V * sizeof(float)));          // rows of meshes without vertex normals stay zero
    HIP_OK(hipDeviceSynchronize());

    // ---------------------------------------------------------------- 1. BVH and scene tables
    EpsmBvhNode *d_nodes = dev_alloc<EpsmBvhNode>(epsm_bvh_max_nodes(T));
    uint32_t *d_prim = dev_alloc<uint32_t>(T);
    float *d_tri_verts = dev_alloc<float>(9 * T);
    int32_t n_nodes = 0, n_levels = 0, level_begin[17];
    size_t ws_bytes = epsm_bvh_workspace_bytes(T);
    const size_t top_ws = epsm_scene_topology_workspace_bytes(T), em_ws = epsm_emitter_tables_bytes(T, n_meshes);
    if (top_ws > ws_bytes) ws_bytes = top_ws;
    if (em_ws > ws_bytes) ws_bytes = em_ws;
    char *d_ws = dev_alloc<char>(ws_bytes);
    const size_t top_bytes = epsm_scene_topology_bytes(V, T);
    char *d_top = dev_alloc<char>(top_bytes);
    Timer t_build(st);
    EPSM_OK_OR_DIE(epsm_bvh_build(d_pos, V, d_tri, T, d_nodes, d_prim, d_tri_verts, &n_nodes, level_begin, &n_levels, d_ws, ws_bytes, st));
    EPSM_OK_OR_DIE(epsm_scene_topology(d_tri, V, T, d_top, top_bytes, d_ws, ws_bytes, st));
    EPSM_OK_OR_DIE(epsm_vertex_normals(d_pos, V, d_tri, T, d_top, mesh_table.data(), vertex_begin.data(), n_meshes, d_nrm, st));
    EPSM_OK_OR_DIE(epsm_emitter_tables(d_pos, V, d_tri, T, mesh_table.data(), d_meshes, n_meshes, d_cdf, T, d_ws, ws_bytes, st));
    const float ms_build = t_build.ms();

    EpsmScene scene;
    memset(&scene, 0, sizeof(scene));
    scene.positions = d_pos; scene.normals = d_nrm; scene.tri = d_tri; scene.tri_mesh = d_tri_mesh;
    scene.meshes = d_meshes; scene.n_meshes = n_meshes;
    scene.bsdfs = d_bsdfs; scene.n_bsdfs = n_bsdfs;
    scene.emitters = d_emitters; scene.n_emitters = n_emitters;
    scene.emitter_cdf = d_cdf;
    scene.bvh = d_nodes; scene.n_nodes = n_nodes; scene.prim_index = d_prim; scene.tri_verts = d_tri_verts;
    scene.n_vertices = V; scene.n_triangles = T;
    scene.env.kind = EPSM_ENV_NONE;

    // ---------------------------------------------------------------- 2. primal image (Scene.render_primal)
    const SensorDesc &psd = sensors[primal_sensor];
    const EpsmSensor ps = sensor_struct(psd), bs = sensor_struct(bsd);
    write_file(out + "/sensor_primal.bin", &ps, sizeof(ps));
    write_file(out + "/sensor_backward.bin", &bs, sizeof(bs));
    const int64_t n_primal = (int64_t) psd.width * psd.height * primal_spp, n_back = (int64_t) res * res * backward_spp;
    const int64_t tile_p = tile_paths(n_primal), tile_b = tile_paths(n_back);
    const int64_t max_tile = tile_p > tile_b ? tile_p : tile_b;
    const size_t trace_ws = epsm_trace_workspace_bytes(max_tile);
    char *d_trace_ws = dev_alloc<char>(trace_ws);
    float *d_accum = dev_alloc<float>((size_t) psd.width * psd.height * 4), *d_img = dev_alloc<float>((size_t) psd.width * psd.height * 3);
    float ms_primal;
    {
        const int64_t n = tile_p < n_primal ? tile_p : n_primal;
        float *d_rays = dev_alloc<float>(12 * n), *d_film = dev_alloc<float>(2 * n), *d_rad = dev_alloc<float>(3 * n);
        uint8_t *d_valid = dev_alloc<uint8_t>(n);
        EpsmRecordOut recs[1];
        memset(recs, 0, sizeof(recs));
        Timer t(st);
        HIP_OK(hipMemsetAsync(d_accum, 0, (size_t) psd.width * psd.height * 4 * sizeof(float), st));
        for (int64_t lo = 0; lo < n_primal; lo += tile_p) {
            const int64_t m = n_primal - lo < tile_p ? n_primal - lo : tile_p;
            EPSM_OK_OR_DIE(epsm_trace_paths_wavefront(&scene, &ps, seed, primal_spp, max_depth, rr_depth, lo, m, 0, d_rays, d_rays + 3 * n,
                                                      d_rays + 6 * n, d_rays + 9 * n, d_film, d_rad, d_valid, recs, 0u, d_trace_ws, trace_ws, st));
            EPSM_OK_OR_DIE(epsm_film_splat(m, d_film, d_rad, psd.width, psd.height, psd.rfilter, d_accum, st));
        }
        EPSM_OK_OR_DIE(epsm_film_develop(psd.width, psd.height, d_accum, d_img, st));
        ms_primal = t.ms();
        std::vector<float> img((size_t) psd.width * psd.height * 3);
        HIP_OK(hipMemcpy(img.data(), d_img, img.size() * sizeof(float), hipMemcpyDeviceToHost));
        write_file(out + "/image.bin", img.data(), img.size() * sizeof(float));
        HIP_OK(hipFree(d_rays)); HIP_OK(hipFree(d_film)); HIP_OK(hipFree(d_rad)); HIP_OK(hipFree(d_valid));
    }

    // ---------------------------------------------------------------- 3. render_backward (wavefront, native log, first-hit fusion)
    const size_t n_grads = 6 * (size_t) V + B + 3;
    float *d_grads = dev_alloc<float>(n_grads);
    float *g_pos = d_grads, *g_nrm = d_grads + 3 * V, *g_alpha = d_grads + 6 * V, *g_origin = d_grads + 6 * V + B;
    const int64_t nb = tile_b < n_back ? tile_b : n_back;
    float *d_lrays = dev_alloc<float>(12 * nb), *d_verts = dev_alloc<float>((size_t) nb * K * 32);
    uint32_t *d_flags = dev_alloc<uint32_t>(nb), *d_surv = dev_alloc<uint32_t>(nb), *d_surv_n = dev_alloc<uint32_t>(1);
    const uint32_t trace_flags = EPSM_TRACE_SPARSE_LOG | EPSM_TRACE_PACKED_LOG | EPSM_TRACE_GRADIENT_ONLY |
                                 (variant == 1 ? EPSM_TRACE_GRADIENT_CAUSTIC : 0u) | EPSM_TRACE_FUSE_FIRST_HIT;
    auto backward = [&](const char *file) -> float {
        Timer t(st);
        HIP_OK(hipMemsetAsync(d_grads, 0, n_grads * sizeof(float), st));
        for (int64_t lo = 0; lo < n_back; lo += tile_b) {
            const int64_t n = n_back - lo < tile_b ? n_back - lo : tile_b;
            HIP_OK(hipMemsetAsync(d_surv_n, 0, sizeof(uint32_t), st));
            EpsmFirstHitBackward fh;
            memset(&fh, 0, sizeof(fh));
            fh.grad_img = d_grad_img; fh.img_width = res; fh.img_channels = 5; fh.res = res; fh.clip = clip;
            fh.tri_table = d_table; fh.T = T; fh.V = V; fh.grad_pos = g_pos; fh.grad_o_sum = g_origin;
            fh.survivors = d_surv; fh.survivor_count = d_surv_n;
            EpsmRecordOut recs[5];
            memset(recs, 0, sizeof(recs));
            recs[0].packed = d_verts; recs[0].pflags = d_flags;
            if (n > 1) { recs[0].ray_stride = 12; recs[0].packed_stride = 32 * K; }
            recs[0].first_hit = &fh;
            EPSM_OK_OR_DIE(epsm_trace_paths_wavefront(&scene, &bs, seed, backward_spp, max_depth, rr_depth, lo, n, K, d_lrays, nullptr, nullptr,
                                                      nullptr, nullptr, nullptr, nullptr, recs, trace_flags, d_trace_ws, trace_ws, st));
            EpsmPackedLog log;
            memset(&log, 0, sizeof(log));
            log.rays = d_lrays; log.flags = d_flags; log.verts = d_verts; log.shadow = nullptr;
            log.ray_stride = n > 1 ? 12 : 0; log.path_stride = n > 1 ? 32 * K : 0;
            log.path_list = d_surv; log.path_count = d_surv_n;
            // d / d ray.o and the paths without a chain are in the buffers already: no grad_o_sum here
            EPSM_OK_OR_DIE(epsm_backward_pass_packed(variant, n, K, lo, backward_spp, res, &log, d_grad_img, res, 5, d_table, T, clip,
                                                     g_pos, g_nrm, B ? g_alpha : nullptr, nullptr, V, B, st));
        }
        const float ms = t.ms();
        std::vector<float> g(n_grads);
        HIP_OK(hipMemcpy(g.data(), d_grads, n_grads * sizeof(float), hipMemcpyDeviceToHost));
        write_file(out + "/" + file, g.data(), n_grads * sizeof(float));
        return ms;
    };
    const float ms_back0 = backward("grads_before.bin");

    // ---------------------------------------------------------------- 4. move the named meshes on the device
    Timer t_move(st);
    for (int i = 0; i < n_meshes; ++i) {
        if (!meshes[i].moves) continue;
        const int64_t v0 = vertex_begin[i], nv = meshes[i].nv;
        for (int64_t j = 0; j < 3 * nv; ++j) pos[3 * v0 + j] += translation[j % 3];
        HIP_OK(hipMemcpyAsync(d_pos + 3 * v0, pos.data() + 3 * v0, 3 * nv * sizeof(float), hipMemcpyHostToDevice, st));
        EPSM_OK_OR_DIE(epsm_vertex_normals(d_pos, V, d_tri, T, d_top, &mesh_table[i], &vertex_begin[i], 1, d_nrm, st));
        EPSM_OK_OR_DIE(epsm_emitter_tables(d_pos, V, d_tri, T, &mesh_table[i], d_meshes + i, 1, d_cdf, T, d_ws, ws_bytes, st));
    }
    EPSM_OK_OR_DIE(epsm_bvh_refit(d_pos, V, d_tri, d_prim, T, d_nodes, n_nodes, level_begin, n_levels, d_tri_verts, st));
    const float ms_move = t_move.ms();
    const float ms_back1 = backward("grads_after.bin");

    printf("scene: %lld vertices, %lld triangles, %d meshes, %d BVH nodes\n", (long long) V, (long long) T, n_meshes, n_nodes);
    printf("phase ms: build %.3f  primal %.3f  backward %.3f  move %.3f  backward_after_move %.3f\n", ms_build, ms_primal, ms_back0,
           ms_move, ms_back1);
    HIP_OK(hipStreamDestroy(st));
    printf("OK\n");
    return 0;
}
