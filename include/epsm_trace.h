/*
 * epsm_trace.h -- C ABI of the wavefront path tracer that PRODUCES the EPSM path records.
 *
 * Replaces, for triangle-mesh scenes, what the reference obtains from Mitsuba 3 + Dr.Jit:
 *   EPSMIntegrator.sample_path (Primal, log_path=True)   epsm.py:503-742   (records: :547, :648-654)
 *   ADIntegrator.prepare / sample_rays                    common.py:291-480 (PCG32 + TEA seeding:
 *                                                         src/render/sampler.cpp:115-134)
 *   PerspectiveCamera::sample_ray_differential            src/sensors/perspective.cpp:238-279
 *   Mesh::compute_surface_interaction (EPSM fields)       src/render/mesh.cpp:632-892
 *   diffuse / conductor / roughconductor / dielectric     src/bsdfs/{...}.cpp (+ the fork's BSDFSample3::hf,
 *                                                         roughconductor.cpp:255, and its forced
 *                                                         non-visible microfacet sampling, microfacet.h `if (true)`)
 *   area / point emitters, Scene::sample_emitter_direction src/emitters/{area,point}.cpp, src/render/scene.cpp:226-300
 *   film splat (box / gaussian) for the primal image      src/render/imageblock.cpp, src/rfilters/gaussian.cpp
 *
 * One lane = one path; bounces run in lock step inside ONE launch (no per-bounce host sync,
 * no .torch() round trips); every logged vertex is written in the record layout of epsm.h
 * together with the parameter addressing (EpsmScatterRecord), so the reference's second,
 * Backward-mode trace is not needed.
 *
 * PARITY UNPINNED: Mitsuba/Dr.Jit can be neither built nor imported here and the reference
 * has no test for these functions; they are pinned by analytic
 * known-answer tests (tests/test_tracer_*.py).
 */
#ifndef EPSM_TRACE_H
#define EPSM_TRACE_H

#include <stdint.h>
#include "epsm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mesh flags (the low four match EPSM_MODE_*) */
#define EPSM_MESH_VERTEX_NORMALS 0x1u
#define EPSM_MESH_FLIP_NORMALS   0x2u
#define EPSM_MESH_POS_ATTACHED   0x4u
#define EPSM_MESH_NRM_ATTACHED   0x8u
#define EPSM_MESH_IS_MESH        0x10u   /* 0: tessellated analytic shape (rectangle): si.ismesh stays 0 */
#define EPSM_MESH_HAS_UV         0x20u   /* EpsmScene.texcoords holds its vertices' (u, v); otherwise si.uv = (b1, b2) (mesh.cpp:736-745) */

enum { EPSM_BSDF_DIFFUSE_T = 0, EPSM_BSDF_CONDUCTOR_T = 1, EPSM_BSDF_ROUGHCONDUCTOR_T = 2, EPSM_BSDF_DIELECTRIC_T = 3 };
enum { EPSM_DISTR_BECKMANN = 0, EPSM_DISTR_GGX = 1 };
enum { EPSM_EMITTER_AREA = 0, EPSM_EMITTER_POINT = 1, EPSM_EMITTER_CONSTANT = 2, EPSM_EMITTER_ENVMAP = 3 };
enum { EPSM_RFILTER_BOX = 0, EPSM_RFILTER_GAUSSIAN = 1 };

/* Tracer flags.
 * EPSM_TRACE_SPARSE_LOG: for a bounce a path did NOT reach, only the four fields the gradient kernels' masks read
 *   (bsdf = 0, active = active_em = ismesh = 0) are written; every other array keeps its previous contents at that
 *   (path, bounce).  The reference logs masked lanes as zeros (epsm.py:551, 648-654) and so does the default; the
 *   zeros are 203 B per dead (path, bounce) that epsm_manifold_grad / _scatter / epsm_backward_pass never read. */
#define EPSM_TRACE_SPARSE_LOG 0x1u
/* EPSM_TRACE_PACKED_LOG: the vertex log is written in the NATIVE layout of the backward kernel (include/epsm.h,
 * EpsmPackedLog) instead of the per-field arrays: recs[0].packed = (N, K_log, 32) words, one 128-byte record per
 * (path, bounce) written with eight 16-byte stores, recs[0].pflags = (N) flag words (5 bits per bounce); bounces a path
 * did not reach are not touched (the flag word says so).  ray_o must then point to an (N,12) array that receives
 * o, d, d_x, d_y of a path side by side (ray_d / ray_dx / ray_dy are ignored); only `shadow` of the per-field pointers is
 * still used.  recs[0].ray_stride / packed_stride (words per path, multiples of 4) place both in one interleaved block per path.  The alpha slot of a vertex's BSDF is NOT in the record: the consumer takes it from the triangle table
 * (bits 8.. of the mode word). */
#define EPSM_TRACE_PACKED_LOG 0x2u
/* EPSM_TRACE_GRADIENT_ONLY: the trace feeds calc_grad and nothing else (render_backward's 5-channel branch, epsm.py:235-297:
 * the image of that pass is never used, :729-732) -- a path is RETIRED after the bounce that logs vertex k as soon as no
 * later vertex can produce, or be read by, a term of calc_grad, i.e. when the masks of epsm.py:793-803, 852-856, 916-921
 * (`valid`: every vertex so far is a mesh hit; `hasdiffuse == 0`) can no longer hold for any id >= k:
 *     manifold           goes on while every vertex so far is a mesh hit and none is Diffuse
 *     manifold_caustic   (with EPSM_TRACE_GRADIENT_CAUSTIC) goes on while vertex 1 is Diffuse, every vertex so far is a
 *                        mesh hit and fewer than two are Diffuse (epsm.py:998-999, 1172-1183)
 * and after vertex K_log in any case.  The visibility ray of an emitter sample is traced only where its answer is read: it
 * decides the logged weight eweight = sum Lr_dir, which calc_grad uses in the light-sampling term of a vertex behind which a
 * `manifold` path goes on (epsm.py:622-627, 852-855) and nowhere in manifold_caustic (its light terms are identically zero);
 * the occluder record of vertex 1 (max_depth <= 3, epsm.py:609-620) is traced as always.  With the native log a vertex that
 * retires its path by the rule -- a chain's end point, a diffuse first hit: only ever LOOKED at -- gets the first sector of its
 * record and its Diffuse / Null / active / mesh bits, nothing else (no emitter or BSDF sample is drawn for it; its active_em
 * bit stays 0).  Every word calc_grad reads is the one the full trace writes, so the gradients are identical; `radiance`,
 * the eweight words nobody reads and the second sector / active_em bit of such vertices are NOT those of the full trace: pass
 * radiance = valid = film_pos = NULL (with the native log nothing is then written for them and the finishing pass is skipped).  bench.py's real_scene leg: trace + log 14.3 -> see DESIGN.md 5b. */
#define EPSM_TRACE_GRADIENT_ONLY    0x4u
#define EPSM_TRACE_GRADIENT_CAUSTIC 0x8u
/* EPSM_TRACE_NO_TAIL (epsm_trace_paths_wavefront only; diagnostics): keep the three stages for EVERY bounce.  Without it the
 * paths still alive into a bounce >= 1 are carried through the rest of their loop by ONE launch as soon as fewer than 2^19 of
 * them are left (a stage cannot take less than one traversal's chain of cache misses, ~0.1 ms, however short its queue) --
 * same arithmetic per path, same results; the queue-length counters of the bounces behind that point then stay 0. */
#define EPSM_TRACE_NO_TAIL          0x10u
/* EPSM_TRACE_FUSE_FIRST_HIT (with EPSM_TRACE_GRADIENT_ONLY + EPSM_TRACE_PACKED_LOG, wavefront form only; recs[0].first_hit names the
 * backward pass's inputs): what epsm_backward_pass_packed would do for a path WITHOUT a chain is done by the stage that finds its
 * first hit (the primary rays' packet stage), and nothing of such a path is logged --
 *   - every path's share of d loss / d ray.o = -sum grad_d (epsm.py:255-261) goes into first_hit->grad_o_sum (when not NULL);
 *   - a path the rule retires at its first vertex (a diffuse, non-mesh or missed first hit: 94 % of the paths of the clutter scene)
 *     gives its first-vertex tangent's rows -- si_follow.p * diffuse_grad[0] = clamp(dldp) b_j into the hit triangle's vertex rows of
 *     first_hit->grad_pos (epsm.py:250-272, 561-562, 791-792) -- there, summed over the wave first, and its flag word is written as 0:
 *     the backward kernel, called with grad_o_sum = NULL for this log, gives it no lane and reads nothing of it.
 * Same sums as the unfused pair of calls (float order aside).  Not with the occluder record (max_depth <= 3). */
#define EPSM_TRACE_FUSE_FIRST_HIT   0x20u

typedef struct EpsmMesh {
    uint32_t tri_begin, tri_count;   /* this mesh's range in the triangle arrays */
    uint32_t flags;                  /* EPSM_MESH_* */
    int32_t bsdf;                    /* index into bsdfs */
    int32_t emitter;                 /* index into emitters, -1 = none */
    float area;                      /* total surface area (emitter sampling pdf) */
    uint32_t cdf_begin;              /* first entry of this mesh's triangle-area CDF in emitter_cdf (tri_count entries) */
    uint32_t pad;
} EpsmMesh;

typedef struct EpsmBsdf {
    uint32_t type;                   /* EPSM_BSDF_*_T */
    uint32_t twosided;
    uint32_t distr;                  /* EPSM_DISTR_* (roughconductor) */
    uint32_t sample_visible;         /* roughconductor: selects the weight/pdf formulas (roughconductor.cpp:258-262) */
    float reflectance[3];            /* diffuse reflectance / specular_reflectance */
    float alpha;                     /* roughconductor roughness */
    float eta[3], k[3];              /* conductor complex IOR; eta = 0,k = 1 is the '100 % reflecting mirror' */
    float int_ior, ext_ior;          /* dielectric */
    int32_t alpha_slot;              /* slot of this BSDF's alpha in grad_alpha, -1 = not optimised */
    int32_t color_slot;              /* diffuse: slot of `reflectance` in the colour adjoint of epsm_trace_paths_color,
                                        -1 = not optimised */
    int32_t texture;                 /* diffuse: index into EpsmScene.textures of the `bitmap` its reflectance is (a texture whose
                                        channels are 0 or 3) or of the per-vertex table it is (EPSM_TEXTURE_VERTEX_RGB), -1 = `reflectance`.  roughconductor: index of the 1-channel `bitmap`
                                        its alpha is (channels = 1), -1 = `alpha`; such a BSDF has alpha_slot = -1.  A texture of the
                                        other kind is ignored, never read through; no table written so far sets this word on
                                        anything but a diffuse BSDF */
    uint32_t material;               /* conductor / roughconductor: 0 = eta, k, specular_reflectance not optimised, s + 1 = material
                                        slot s of epsm_trace_paths_material_backward (the word that was padding: 0 in every table) */
} EpsmBsdf;

/* A `bitmap` texture (src/textures/bitmap.cpp): linear RGB texels -- or scalar ones, the roughness map of a roughconductor
 * (roughconductor.cpp:195-198) -- looked up at si.uv as there: uv * (width, height) - 0.5, bilinear between the four texels
 * around it (or the nearest one), indices wrapped (`repeat`).
 * Or, with channels = EPSM_TEXTURE_VERTEX_RGB, no bitmap at all but a per-vertex table: the `mesh_attribute` texture
 * (src/textures/mesh_attribute.cpp) of ONE mesh's `vertex_color`, the reflectance of a diffuse BSDF.  texels is then (count, 3),
 * the mesh's vertices in its own order (any `scale` applied), and the two size words say which rows of EpsmScene's vertex arrays
 * the table covers: width = EPSM_TEXTURE_VERTEX_FIRST, the first row; height = EPSM_TEXTURE_VERTEX_COUNT, how many.  A hit on
 * triangle (vi0, vi1, vi2) with barycentrics (b0, b1, b2) reads b0 c[vi0 - first] + b1 c[vi1 - first] + b2 c[vi2 - first]; a row
 * outside [first, first + count) makes the lookup ignored (EpsmBsdf.reflectance stays).  nearest is 0.  Such a table is never
 * walked as a bitmap: every bitmap reader ignores it, as a 1-channel texture is ignored where three are expected. */
#define EPSM_TEXTURE_RGB 3u          /* channels: RGB texels (0 means the same) */
#define EPSM_TEXTURE_SCALAR 1u       /* channels: scalar texels */
#define EPSM_TEXTURE_VERTEX_RGB 4u   /* channels: not a bitmap -- a per-vertex RGB table (above) */
#define EPSM_TEXTURE_VERTEX_FIRST(T) ((T).width)     /* per-vertex table: first row of the scene's vertex arrays it covers */
#define EPSM_TEXTURE_VERTEX_COUNT(T) ((T).height)    /* per-vertex table: number of rows */
typedef struct EpsmTexture {
    const float *texels;             /* (height, width, 3), or (height, width) when channels = 1; row 0 at v = 0.  Per-vertex table:
                                        (count, 3) */
    int32_t width, height;           /* per-vertex table: first row, count */
    uint32_t nearest;                /* filter_type: 0 bilinear, 1 nearest */
    uint32_t channels;               /* 0 or 3: RGB texels; 1: scalar texels (the word that was padding: 0 in every table);
                                        EPSM_TEXTURE_VERTEX_RGB: a per-vertex RGB table, width / height as above */
} EpsmTexture;

typedef struct EpsmEmitter {
    uint32_t type;                   /* EPSM_EMITTER_* */
    int32_t mesh;                    /* area: emitting mesh */
    float radiance[3];               /* area, constant: radiance; point: intensity; envmap: unused (EpsmEnvironment.texels) */
    float position[3];               /* point */
    int32_t color_slot;              /* slot of `radiance` in the colour adjoint, -1 = not optimised */
    uint32_t pad;
} EpsmEmitter;

typedef struct EpsmBvhNode {         /* 128 bytes: the boxes of up to FOUR children, one component of all four per 16-byte quad */
    float lox[4], loy[4], loz[4];    /* lower corners (absent child: +inf) */
    float hix[4], hiy[4], hiz[4];    /* upper corners (absent child: -inf) */
    int32_t c[4];                    /* child reference: >= 0 node index; < 0 leaf ~((first << 3) | count) with `first`
                                        the leaf's first triangle in tri_verts / prim_index and count <= 7;
                                        0x7fffffff = absent */
    int32_t n[4];                    /* build-side copy of the leaf counts (0 = inner); not read by the traversal */
} EpsmBvhNode;

typedef struct EpsmSensor {
    float to_world[12];              /* 3x4 row-major camera-to-world (rotation | translation) */
    float sample_to_camera[16];      /* 4x4 row-major, perspective.cpp:171-176 */
    float dx[3], dy[3];              /* position differentials on the near plane, perspective.cpp:178-182 */
    float near_clip, far_clip;
    int32_t width, height;
    int32_t border;                  /* film.sample_border: samples are also generated for `border` pixels around the film
                                        (rfilter.border_size(): 2 for the gaussian, 0 for the box), common.py:309-336; the
                                        wavefront is then (width + 2 border) (height + 2 border) spp paths */
    int32_t pad;
} EpsmSensor;

/* The scene's environment emitter (src/emitters/constant.cpp, envmap.cpp): at most one, `kind` says which (0: none) and
 * `emitter` = its index in EpsmScene.emitters.  Every tracer entry point checks: kind in {0, 1, 2}; kind != 0 => 0 <= emitter <
 * n_emitters; kind == ENVMAP => the four tables non-NULL and width, height >= 2; n_textures > 0 => textures non-NULL (EPSM_EINVAL).  A ray that leaves the scene sees its radiance (MIS against emitter sampling as for an area
 * light); an emitter sample is the point ref + 2 max(radius, |ref - center|) d (constant.cpp:113-116, envmap.cpp:398-399) -- what
 * the vertex log records as `light` -- with d uniform on the sphere (constant) or drawn from the map.
 * envmap: `texels` is the (height, width + 1, 3) lat-long map, `scale` applied, column `width` a copy of column 0; texel (i, j)
 * sits at phi = 2 pi (i + 1/2) / width, theta = pi j / (height - 1) (envmap.cpp:387-395, 416-422), direction
 * (sin phi sin theta, cos theta, -cos phi sin theta) in the emitter's frame; radiance is bilinear in between.  Sampling is by
 * CELL (the width x (height - 1) bilinear patches): weight = mean over the four corners of luminance x sin theta, rows by
 * `row_cdf`, columns by `col_cdf`, uniform inside a cell -- a piecewise-constant stand-in for the reference's hierarchical
 * sample warp (same support, same estimator up to variance). */
enum { EPSM_ENV_NONE = 0, EPSM_ENV_CONSTANT = 1, EPSM_ENV_ENVMAP = 2 };
typedef struct EpsmEnvironment {
    int32_t kind;                    /* EPSM_ENV_*: 0 = the scene has no environment emitter, so a zero-initialised EpsmScene is
                                        safe (ABI 6; until ABI 5 `emitter = -1` said so and 0 named emitter 0).  `kind`, not
                                        emitters[emitter].type, decides which tables the device code touches. */
    int32_t emitter;                 /* kind != 0: its index in EpsmScene.emitters (radiance, colour slot, emitter choice) */
    int32_t width, height;           /* envmap only */
    const float *texels;             /* (height, width + 1, 3) */
    const float *row_cdf;            /* (height - 1) cumulative, normalised */
    const float *col_cdf;            /* (height - 1, width) cumulative per row, normalised */
    const float *cell_pdf;           /* (height - 1, width) density of a cell in (u, v) in [0,1)^2 */
    float to_local[9];               /* world -> emitter frame, row-major rotation */
    float center[3], radius;         /* bounding sphere of shapes and sensors */
} EpsmEnvironment;

typedef struct EpsmScene {           /* host struct holding DEVICE pointers */
    const float *positions;          /* (V,3) world space */
    const float *normals;            /* (V,3) (zero rows for meshes without vertex normals) */
    const uint32_t *tri;             /* (T,3) rows of the triangle's vertices in positions/normals, mesh by mesh */
    const uint32_t *tri_mesh;        /* (T)   owning mesh */
    const EpsmMesh *meshes;          int32_t n_meshes;
    const EpsmBsdf *bsdfs;           int32_t n_bsdfs;
    const EpsmEmitter *emitters;     int32_t n_emitters;
    const float *emitter_cdf;        /* concatenated normalised area CDFs of the emitting meshes */
    const EpsmBvhNode *bvh;          int32_t n_nodes;   /* node 0 is the root; depth <= 16 (four-wide) */
    const uint32_t *prim_index;      /* leaf entries: BVH order -> triangle id (triangles stay mesh-contiguous) */
    const float *tri_verts;          /* (T,9) p0,p1,p2 of the triangles in BVH (leaf) order */
    int64_t n_vertices, n_triangles;
    EpsmEnvironment env;
    const float *texcoords;          /* (V,2) per-vertex (u, v) of the meshes flagged EPSM_MESH_HAS_UV (zero rows elsewhere), or NULL */
    const EpsmTexture *textures;     int32_t n_textures;
} EpsmScene;

/* EPSM_TRACE_FUSE_FIRST_HIT: the arguments epsm_backward_pass_packed takes for the same tile (include/epsm.h) */
typedef struct EpsmFirstHitBackward {
    const float *grad_img;           /* (.., img_width, img_channels): channels 3, 4 = d loss / d film position */
    int img_width, img_channels, res;
    float clip;                      /* outlier clamp of calc_grad (0.1 in the reference); <= 0 or non-finite: none */
    const uint32_t *tri_table;       /* (T,4) [v0, v1, v2, mode] */
    int64_t T, V;
    float *grad_pos;                 /* (V,3), accumulated */
    float *grad_o_sum;               /* (3), accumulated; may be NULL */
    uint32_t *survivors;             /* (N) or NULL: receives, in path order, the indices of the paths this stage did NOT retire -- the only
                                        ones of which the log holds anything -- and *survivor_count their number: EpsmPackedLog.path_list /
                                        path_count of the backward pass that follows (its windows then run over these paths alone) */
    uint32_t *survivor_count;        /* (1) or NULL (both or neither) */
} EpsmFirstHitBackward;

/* Writable twin of EpsmVertexRecord + EpsmScatterRecord for one logged bounce. */
typedef struct EpsmRecordOut {
    float *p0, *p1, *p2, *p;         /* (N,3) */
    float *n0, *n1, *n2, *normal;    /* (N,3) */
    float *b0, *b1, *eta;            /* (N) */
    float *hf, *light;               /* (N,3) */
    uint32_t *bsdf;                  /* (N) */
    uint8_t *active, *active_em, *ismesh;  /* (N) */
    uint32_t *tri, *aux, *emit;      /* (N) (N,4) (N,4): EpsmScatterRecord (tri = triangle id, emit = [etri, eb0, eb1, ew]) */
    float *packed;                   /* EPSM_TRACE_PACKED_LOG, recs[0] only: (N, K_log, 32) words */
    uint32_t *pflags;                /* EPSM_TRACE_PACKED_LOG, recs[0] only: (N) flag words */
    uint32_t *shadow;                /* (N,4): EpsmScatterRecord.shadow [stri, sb0, sb1, dis]; written for the first logged vertex only and
                                        only meaningful when max_depth <= 3 (epsm.py:610); may be NULL */
    int64_t ray_stride, packed_stride; /* EPSM_TRACE_PACKED_LOG, recs[0] only (ABI v7): words between the rays (at ray_o) / the first
                                        records (at packed) of consecutive paths; 0 = dense, 12 and 32 K_log.  The interleaved block
                                        of include/epsm.h (EpsmPackedLog): ray_o = block, packed = block + 16, both 32 (K_log + 1) */
    const EpsmFirstHitBackward *first_hit; /* EPSM_TRACE_FUSE_FIRST_HIT, recs[0] only (a HOST pointer: read during the call) */
} EpsmRecordOut;

/* ---------------------------------------------------------------------------
 * epsm_trace_paths -- sample_rays + sample_path(Primal, log_path=True) for paths
 *   [path_offset, path_offset + N) of the wavefront  width*height*spp  (ordered pixel-major,
 *   then sample: common.py:320-330).
 *   seed, spp, max_depth, rr_depth   as in ADIntegrator (common.py:28-43, 424-480)
 *   K_log                            bounces to log (<= 5, epsm.py:648)
 *   ray_o/d/dx/dy (N,3), film_pos (N,2), radiance (N,3), valid (N) u8: outputs (any may be NULL
 *                                    except ray_*); radiance = L of epsm.py:658, valid = depth != 0
 *   recs                             K_log records to fill (all fields written for every path)
 *   flags                            0 or any of EPSM_TRACE_SPARSE_LOG, EPSM_TRACE_PACKED_LOG, EPSM_TRACE_GRADIENT_ONLY (+ _CAUSTIC)
 * ------------------------------------------------------------------------- */
int epsm_trace_paths(const EpsmScene *scene, const EpsmSensor *sensor,
                     uint32_t seed, int spp, int max_depth, int rr_depth,
                     int64_t path_offset, int64_t N, int K_log,
                     float *ray_o, float *ray_d, float *ray_dx, float *ray_dy,
                     float *film_pos, float *radiance, uint8_t *valid,
                     const EpsmRecordOut *recs, uint32_t flags, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_trace_paths_wavefront -- the same function (same arguments, same per-path results) run as a
 *   wavefront of stages with compaction between the bounces: per bounce one closest-hit kernel, one
 *   shading kernel (the loop body of epsm.py:551-735) and one shadow-ray kernel over QUEUES of the
 *   paths that are still alive, then one pass that writes radiance / valid and the inactive-zero
 *   records of the bounces a path never reached.  Pays on scenes with many triangles, where the
 *   one-launch form is bound by divergence (dead lanes, mixed closest-hit / shadow traversals) and by
 *   the occupancy its register count allows; costs 172 B/path/bounce of state traffic, so small scenes
 *   are faster in one launch.
 *   workspace        device memory, 16-byte aligned, >= epsm_trace_workspace_bytes(N); contents are
 *                    scratch (no state is kept between calls)
 * ------------------------------------------------------------------------- */
size_t epsm_trace_workspace_bytes(int64_t N);
int epsm_trace_paths_wavefront(const EpsmScene *scene, const EpsmSensor *sensor,
                               uint32_t seed, int spp, int max_depth, int rr_depth,
                               int64_t path_offset, int64_t N, int K_log,
                               float *ray_o, float *ray_d, float *ray_dx, float *ray_dy,
                               float *film_pos, float *radiance, uint8_t *valid,
                               const EpsmRecordOut *recs, uint32_t flags, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_trace_paths_color -- epsm_trace_paths (no vertex log) that also returns, per path, the derivative of its
 *   radiance w.r.t. the COLOUR parameters attached to the scene (EpsmBsdf.color_slot: diffuse reflectance;
 *   EpsmEmitter.color_slot: emitted radiance / intensity) -- the colour adjoint of the reference's hybrid phase
 *   (3-channel grad_in: epsm.py:230-234 -> prb-style backward, src/python/python/ad/integrators/prb.py) for parameters
 *   the radiance is multiplicative in.  Sampling is detached as in PRB: a term T of the estimator that passed n_j
 *   vertices of BSDF j satisfies dT/d rho_j,c = n_j T_c / rho_j,c, and dT/dE_e,c = T_c / E_e,c for the emitter it ends on.
 *     color_sum   (N, n_color, 3) f32, written: sum over the path's terms of n_j T_c (BSDF slots) / T_c (emitter
 *                 slots); the caller divides by the parameter value and contracts with the adjoint radiance
 *     n_color     number of slots, <= 4
 *   One-launch form only.  Visibility / geometry derivatives (prb_reparam's warp field) are NOT part of it.
 * ------------------------------------------------------------------------- */
int epsm_trace_paths_color(const EpsmScene *scene, const EpsmSensor *sensor,
                           uint32_t seed, int spp, int max_depth, int rr_depth,
                           int64_t path_offset, int64_t N,
                           float *film_pos, float *radiance, uint8_t *valid,
                           float *color_sum, int n_color, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_trace_paths_reparam -- the second pass of RBIntegrator.render_backward for `prb_reparam`
 *   (src/python/python/ad/integrators/common.py:944-955, prb_reparam.py:277-607, ad/reparam.py:10-333): paths
 *   [path_offset, path_offset + N) are replayed under the primal pass's seed and the gradient of
 *   sum(image * grad_in) w.r.t. the VERTEX POSITIONS (and vertex normals) of the meshes flagged EPSM_MESH_POS_ATTACHED
 *   (EPSM_MESH_NRM_ATTACHED) is ACCUMULATED into grad_pos / grad_nrm -- through shading, and through visibility by the
 *   warp field of Bangaru et al. (auxiliary rays, harmonic weights, divergence).
 *     radiance      (N,3) L of every path from the primal pass (epsm_trace_paths with the same seed / spp / depth)
 *     adj_radiance  (N,3) d loss / d L               } the adjoint of splat + weight division, which the caller owns
 *     adj_film      (N,3) d loss / d film position (x, y in pixels) and d loss / d det of the primary ray's
 *                         reparameterisation (common.py:405-418, 888-903)
 *     reparam_max_depth, reparam_rays (<= 64), kappa, exponent   prb_reparam.py:226-250
 *     flags         EPSM_REPARAM_ANTITHETIC: auxiliary rays 2m and 2m + 1 of a warp share one sample, the even one mirrored
 *                   about the ray (`reparam_antithetic`, prb_reparam.py:243-246, reparam.py:82-84, 189-196)
 *     grad_pos, grad_nrm   (V,3) f32 device buffers, float atomics; grad_nrm may be NULL
 *     workspace            device memory, 16-byte aligned, >= epsm_trace_reparam_workspace_bytes(N); scratch
 *   Two launches: (1) a lane replays its path, differentiates each vertex (dual numbers) and leaves one 64-byte REQUEST
 *   per reparameterize_ray call -- ray, adjoint of its direction and divergence, where its origin is glued -- at most
 *   13 per path; (2) one lane per AUXILIARY RAY: the 16 / 32 / 64 lanes of a request trace its rays side by side, reduce
 *   the weights over the group and scatter the warp field's adjoint.
 * ------------------------------------------------------------------------- */
#define EPSM_REPARAM_ANTITHETIC 1u
size_t epsm_trace_reparam_workspace_bytes(int64_t N);
int epsm_trace_paths_reparam(const EpsmScene *scene, const EpsmSensor *sensor,
                             uint32_t seed, int spp, int max_depth, int rr_depth,
                             int64_t path_offset, int64_t N,
                             const float *radiance, const float *adj_radiance, const float *adj_film,
                             int reparam_max_depth, int reparam_rays, float kappa, float exponent, uint32_t flags,
                             float *grad_pos, float *grad_nrm, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_trace_paths_reparam_forward -- forward mode of the same pass: what `prb_reparam`'s render_forward
 *   (src/python/python/ad/integrators/common.py:118-197, prb_reparam.py:243-589 under ADMode.Forward) computes for the
 *   geometry, as the exact TRANSPOSE of epsm_trace_paths_reparam: the same paths, the same auxiliary rays and the same
 *   detached quantities.  For tangents of the vertex positions (and vertex normals) of the meshes flagged
 *   EPSM_MESH_POS_ATTACHED (EPSM_MESH_NRM_ATTACHED) -- the rows of other meshes are not read -- it WRITES, per path:
 *     d_radiance    (N,3) d L
 *     d_film        (N,3) d film position (x, y in pixels) and d det of the primary ray's reparameterisation
 *   so that sum(adj_radiance * d_radiance + adj_film * d_film) = sum(grad_pos * tan_pos + grad_nrm * tan_nrm) for any
 *   adjoints the backward pass is given.  radiance, reparam_max_depth .. flags: as for epsm_trace_paths_reparam;
 *   tan_pos, tan_nrm (V,3) f32 device buffers, tan_nrm may be NULL; workspace >= epsm_trace_reparam_forward_workspace_bytes(N).
 *   Three launches: (1) a lane replays its path and writes its warp requests (ray, glued origin, emitter distance);
 *   (2) one lane per auxiliary ray, as in the backward pass, gathers the motion of its hit and of the origin, and each
 *   request's group reduces them to the tangent of its direction and of its divergence; (3) a lane replays its path again,
 *   reads those back and evaluates each vertex once per colour channel in dual numbers.  No atomics.
 * ------------------------------------------------------------------------- */
size_t epsm_trace_reparam_forward_workspace_bytes(int64_t N);
int epsm_trace_paths_reparam_forward(const EpsmScene *scene, const EpsmSensor *sensor,
                                     uint32_t seed, int spp, int max_depth, int rr_depth,
                                     int64_t path_offset, int64_t N,
                                     const float *radiance, const float *tan_pos, const float *tan_nrm,
                                     int reparam_max_depth, int reparam_rays, float kappa, float exponent, uint32_t flags,
                                     float *d_radiance, float *d_film, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_trace_paths_texture_backward -- the TEXEL adjoint of `prb` (prb.py, sampling, Russian roulette and MIS detached):
 *   paths [path_offset, path_offset + N) are replayed under the primal seed as epsm_trace_paths_color traced them, and
 *   d loss / d texel is ACCUMULATED (float atomics, after a merge over the lanes of a wave that share a footprint) for
 *     - the `bitmap` reflectance of a diffuse BSDF (EpsmBsdf.texture = t): grad_tex[t], (height_t, width_t, 3) f32 shaped like
 *       EpsmScene.textures[t].  A diffuse vertex k looked up at uv_k adds adj . L_after_k / rho_k x w to each texel of its
 *       footprint (4 bilinear, 1 nearest; wrap as the lookup), L_after_k = radiance - L collected up to and including the
 *       emission at k; a channel with rho_k = 0 adds nothing (prb.py's inv_bsdf_val_det);
 *     - the per-vertex reflectance of a diffuse BSDF (EpsmScene.textures[t].channels == EPSM_TEXTURE_VERTEX_RGB): grad_tex[t],
 *       (count_t, 3) f32 shaped like the table.  The same term goes to the three rows of the hit's vertices with the
 *       barycentrics (b0, b1, b2) as weights; a hit with a vertex outside the table adds nothing;
 *     - the envmap (EpsmScene.env.kind == EPSM_ENV_ENVMAP): grad_env, (height, width, 3) f32 -- the bitmap's shape: column
 *       `width` of EpsmEnvironment.texels folds into column 0.  A ray that leaves the scene adds adj . beta mis x w, an emitter
 *       sample on the map adj . beta bsdf mis / pdf x w when it is not occluded; the sampling tables are detached.
 *     radiance      (N,3) L of every path from the primal pass (epsm_trace_paths_color with the same seed / spp / depths)
 *     adj_radiance  (N,3) d loss / d L (the adjoint of splat + weight division, which the caller owns)
 *     grad_tex      NULL or an array of n_textures HOST pointers; entry t NULL = texture t not attached.  At most
 *                   EPSM_MAX_TEXTURE_GRADS entries non-NULL (EPSM_EINVAL): they go into the kernel's arguments, no allocation
 *     grad_env      NULL or the envmap's buffer
 *   One launch.  No host synchronisation.
 * epsm_trace_paths_texture_forward -- its exact transpose: the same replay GATHERS the tangents tan_tex / tan_env (same
 *   layouts, read only where attached) and WRITES d_radiance (N,3), so that sum(adj_radiance * d_radiance) =
 *   sum(grad_tex . tan_tex) + sum(grad_env . tan_env) for any adjoint.  No atomics.
 * ------------------------------------------------------------------------- */
#define EPSM_MAX_TEXTURE_GRADS 8
int epsm_trace_paths_texture_backward(const EpsmScene *scene, const EpsmSensor *sensor,
                                      uint32_t seed, int spp, int max_depth, int rr_depth,
                                      int64_t path_offset, int64_t N,
                                      const float *radiance, const float *adj_radiance,
                                      float *const *grad_tex, float *grad_env, void *stream);
int epsm_trace_paths_texture_forward(const EpsmScene *scene, const EpsmSensor *sensor,
                                     uint32_t seed, int spp, int max_depth, int rr_depth,
                                     int64_t path_offset, int64_t N,
                                     const float *radiance, const float *const *tan_tex, const float *tan_env,
                                     float *d_radiance, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_trace_paths_alpha_texture_backward -- the ROUGHNESS-MAP adjoint of `prb`: the rule of epsm_trace_paths_bsdf_backward
 *   (below) for a `roughconductor` whose alpha is a 1-channel `bitmap` (EpsmBsdf.texture = t, EpsmScene.textures[t].channels
 *   = 1), scattered like epsm_trace_paths_texture_backward.  Paths [path_offset, path_offset + N) are replayed under the primal
 *   seed as epsm_trace_paths_color traced them; at an active bounce on such a BSDF, alpha = the map's value at the vertex's uv,
 *     - the sampled direction gives L_ind  d f / d alpha / (weight pdf) per channel (a channel with weight pdf = 0: nothing),
 *     - the emitter sample gives Lr_dir  d ln f / d alpha (nothing when occluded),
 *   and adj . (their sum) x w is ACCUMULATED into each texel of the lookup's footprint (4 bilinear, 1 nearest; wrap as the
 *   lookup): float atomics, after a merge over the lanes of a wave that share a footprint.  Sampling, Russian roulette and the
 *   MIS weights are detached.
 *     radiance      (N,3) L of every path from the primal pass (epsm_trace_paths_color with the same seed / spp / depths)
 *     adj_radiance  (N,3) d loss / d L
 *     grad_tex      NULL or an array of n_textures HOST pointers; entry t NULL = texture t not attached, otherwise (height_t,
 *                   width_t) f32, added to.  An entry for a texture that is not 1-channel is never touched.  At most
 *                   EPSM_MAX_TEXTURE_GRADS entries non-NULL (EPSM_EINVAL).  With no entry the call does nothing
 *   One launch.  No host synchronisation.  Float atomics: the bits depend on the order of the adds.
 * epsm_trace_paths_alpha_texture_forward -- its exact transpose: the same replay GATHERS the tangents tan_tex (same layout,
 *   read only where attached) and WRITES d_radiance (N,3), so that sum(adj_radiance * d_radiance) = sum(grad_tex . tan_tex).
 *   No atomics.
 * ------------------------------------------------------------------------- */
int epsm_trace_paths_alpha_texture_backward(const EpsmScene *scene, const EpsmSensor *sensor,
                                            uint32_t seed, int spp, int max_depth, int rr_depth,
                                            int64_t path_offset, int64_t N,
                                            const float *radiance, const float *adj_radiance,
                                            float *const *grad_tex, void *stream);
int epsm_trace_paths_alpha_texture_forward(const EpsmScene *scene, const EpsmSensor *sensor,
                                           uint32_t seed, int spp, int max_depth, int rr_depth,
                                           int64_t path_offset, int64_t N,
                                           const float *radiance, const float *const *tan_tex,
                                           float *d_radiance, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_trace_paths_bsdf_backward -- the ROUGHNESS adjoint of `prb` (prb.py:145-158, 209-226; sampling, Russian roulette and the
 *   MIS weights detached): paths [path_offset, path_offset + N) are replayed under the primal seed as epsm_trace_paths_color
 *   traced them, and d loss / d alpha is ADDED to grad_alpha[EpsmBsdf.alpha_slot] for every `roughconductor` BSDF with
 *   0 <= alpha_slot < B.  At an active bounce on such a BSDF
 *     - the sampled direction adds adj . L_ind  d f / d alpha / (weight pdf) per channel, L_ind = what the path collects behind
 *       the bounce, f the value of eval_pdf for the sampled direction, weight and pdf those of the sample (a channel with
 *       weight pdf = 0 adds nothing);
 *     - the emitter sample adds adj . Lr_dir  d ln f / d alpha (nothing when occluded); its MIS weight is detached like the
 *       weight of the next vertex's emission, so that the two move together.
 *     radiance      (N,3) L of every path from the primal pass (epsm_trace_paths_color with the same seed / spp / depths)
 *     adj_radiance  (N,3) d loss / d L
 *     grad_alpha    (B) f32, added to; B <= EPSM_MAX_ALPHA_GRADS (EPSM_EINVAL otherwise: nothing is dropped silently)
 *     workspace     device memory, 16-byte aligned, >= epsm_trace_bsdf_workspace_bytes(N); scratch
 *   No float atomics: each workgroup of 128 paths reduces its sums to one row of the workspace, a second launch adds the rows
 *   in float64 in a fixed order -- two calls with the same arguments give the same bits.  No host synchronisation.
 * epsm_trace_paths_bsdf_forward -- its exact transpose: the same replay WRITES d_radiance (N,3) = sum over the path's terms of
 *   their coefficient x tangent_alpha[slot], so that sum(adj_radiance * d_radiance) = sum(grad_alpha * tangent_alpha).  One launch.
 * ------------------------------------------------------------------------- */
#define EPSM_MAX_ALPHA_GRADS 8
size_t epsm_trace_bsdf_workspace_bytes(int64_t N);
int epsm_trace_paths_bsdf_backward(const EpsmScene *scene, const EpsmSensor *sensor,
                                   uint32_t seed, int spp, int max_depth, int rr_depth,
                                   int64_t path_offset, int64_t N,
                                   const float *radiance, const float *adj_radiance, float *grad_alpha, int B,
                                   void *workspace, size_t workspace_bytes, void *stream);
int epsm_trace_paths_bsdf_forward(const EpsmScene *scene, const EpsmSensor *sensor,
                                  uint32_t seed, int spp, int max_depth, int rr_depth,
                                  int64_t path_offset, int64_t N,
                                  const float *radiance, const float *tangent_alpha, int B,
                                  float *d_radiance, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_trace_paths_material_backward -- the CONDUCTOR MATERIAL adjoint of `prb` (prb.py:145-158, 209-226; sampling, Russian
 *   roulette and the MIS weights detached): paths [path_offset, path_offset + N) are replayed under the primal seed as
 *   epsm_trace_paths_color traced them, and d loss / d [eta, k, specular_reflectance], per colour channel, is ADDED to
 *   grad_material[EpsmBsdf.material - 1] for every `conductor` / `roughconductor` BSDF with 1 <= material <= M.  The sample's
 *   weight is F(cos; eta, k) x specular_reflectance x w (conductor.cpp:235-270, roughconductor.cpp:225-300; F: fresnel.h:92-117)
 *   with w, the pdf and the direction free of the three, so nothing is lost to the detached sampling.  At an active bounce on
 *   such a BSDF, per channel c,
 *     - the sampled direction adds adj_c L_ind,c x [d F_c / d eta_c / F_c, d F_c / d k_c / F_c, 1 / R_c], L_ind = what the path
 *       collects behind the bounce, cos = wi . normalize(wi + wo) (wi.z for the delta lobe);
 *     - the emitter sample (roughconductor.cpp:302-400; a delta lobe evaluates to 0) adds the same with Lr_dir in place of
 *       L_ind at the half vector of the emitter's direction (nothing when occluded).
 *   A term whose denominator is 0 or which is not finite adds nothing; d F is 0 where F is cut to a constant (the
 *   `eta = 0, k = 1` mirror).
 *     radiance      (N,3) L of every path from the primal pass (epsm_trace_paths_color with the same seed / spp / depths)
 *     adj_radiance  (N,3) d loss / d L
 *     grad_material (M,3,3) f32 = [eta, k, specular_reflectance] x rgb per slot, added to; M <= EPSM_MAX_MATERIAL_GRADS
 *                   (EPSM_EINVAL otherwise: nothing is dropped silently)
 *     workspace     device memory, 16-byte aligned, >= epsm_trace_material_workspace_bytes(N); scratch
 *   No float atomics: each workgroup of 128 paths reduces its sums to one row of 9 EPSM_MAX_MATERIAL_GRADS floats of the
 *   workspace, a second launch adds the rows in float64 in a fixed order -- two calls with the same arguments give the same
 *   bits.  No host synchronisation.
 * epsm_trace_paths_material_forward -- its exact transpose: the same replay WRITES d_radiance (N,3), per channel the sum over
 *   the path's terms of their coefficients x tangent_material[slot], so that sum(adj_radiance * d_radiance) =
 *   sum(grad_material * tangent_material).  One launch.
 * ------------------------------------------------------------------------- */
#define EPSM_MAX_MATERIAL_GRADS 4
size_t epsm_trace_material_workspace_bytes(int64_t N);
int epsm_trace_paths_material_backward(const EpsmScene *scene, const EpsmSensor *sensor,
                                       uint32_t seed, int spp, int max_depth, int rr_depth,
                                       int64_t path_offset, int64_t N,
                                       const float *radiance, const float *adj_radiance, float *grad_material, int M,
                                       void *workspace, size_t workspace_bytes, void *stream);
int epsm_trace_paths_material_forward(const EpsmScene *scene, const EpsmSensor *sensor,
                                      uint32_t seed, int spp, int max_depth, int rr_depth,
                                      int64_t path_offset, int64_t N,
                                      const float *radiance, const float *tangent_material, int M,
                                      float *d_radiance, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_trace_paths_envpose_backward -- the ENVMAP POSE adjoint of `prb` (sampling, Russian roulette, the MIS weights and the
 *   world directions detached): paths [path_offset, path_offset + N) are replayed under the primal seed as
 *   epsm_trace_paths_color traced them, and d loss / d [omega, ln(scale)] of THE environment (EpsmScene.env, kind
 *   EPSM_ENV_ENVMAP; EPSM_EINVAL for any other kind) is ADDED to grad_pose (4):
 *     omega    parametrises to_world <- Rot(omega) to_world: world axes, right-handed, at omega = 0 (the sensor rotation's
 *              convention);
 *     scale    is the envmap's `scale` property (EpsmEnvironment.texels hold bitmap x scale); the number is d / d ln(scale).
 *   A replayed path reads the map in the items the texel adjoint forms (epsm_trace_paths_texture_backward): a ray that leaves
 *   the scene, coef = beta mis along its direction d, and an emitter sample on the map that is not occluded, coef =
 *   beta bsdf(wo) mis_em / pdf along the sample's direction; its radiance contains sum_items coef_c L_c(d).  Per item
 *     d / d omega     = sum_c adj_c coef_c (g_c x d), g_c = d L_c / d d of the bilinear lat-long lookup (the torque of the
 *                       world-direction gradient: the local direction is to_local Rot(-omega) d);
 *     d / d ln(scale) = sum_c adj_c coef_c L_c(d).
 *   The map sits at infinity, so turning it moves no visibility boundary in direction space: the detachment loses nothing in
 *   expectation.  A term that is not finite adds nothing.
 *     radiance      (N,3) L of every path from the primal pass (epsm_trace_paths_color with the same seed / spp / depths)
 *     adj_radiance  (N,3) d loss / d L
 *     grad_pose     (EPSM_ENV_POSE_GRADS) f32 = [omega.x, omega.y, omega.z, ln(scale)], added to
 *     workspace     device memory, 16-byte aligned, >= epsm_trace_envpose_workspace_bytes(N); scratch
 *   No float atomics: each workgroup of 128 paths reduces its sums to one row of 4 floats of the workspace, a second launch
 *   adds the rows in float64 in a fixed order -- two calls with the same arguments give the same bits.  No host
 *   synchronisation.
 * epsm_trace_paths_envpose_forward -- its exact transpose: the same replay WRITES d_radiance (N,3), per channel the sum over
 *   the path's items of their four derivatives x tangent_pose (4), so that sum(adj_radiance * d_radiance) =
 *   sum(grad_pose * tangent_pose).  One launch.
 * ------------------------------------------------------------------------- */
#define EPSM_ENV_POSE_GRADS 4   /* omega.x, omega.y, omega.z, ln(scale) */
size_t epsm_trace_envpose_workspace_bytes(int64_t N);
int epsm_trace_paths_envpose_backward(const EpsmScene *scene, const EpsmSensor *sensor,
                                      uint32_t seed, int spp, int max_depth, int rr_depth,
                                      int64_t path_offset, int64_t N,
                                      const float *radiance, const float *adj_radiance, float *grad_pose,
                                      void *workspace, size_t workspace_bytes, void *stream);
int epsm_trace_paths_envpose_forward(const EpsmScene *scene, const EpsmSensor *sensor,
                                     uint32_t seed, int spp, int max_depth, int rr_depth,
                                     int64_t path_offset, int64_t N,
                                     const float *radiance, const float *tangent_pose,
                                     float *d_radiance, void *stream);

/* epsm_film_splat -- ImageBlock::put + weight division (film.develop): accumulates
 * radiance with the reconstruction filter into accum (height,width,4) [r,g,b,w] (atomics);
 * epsm_film_develop divides into image (height,width,3). */
int epsm_film_splat(int64_t N, const float *film_pos, const float *radiance, int width, int height,
                    int rfilter, float *accum, void *stream);
int epsm_film_develop(int width, int height, const float *accum, float *image, void *stream);

/* epsm_film_adjoint_reparam -- the adjoint of splat + weight division between the two passes of prb_reparam's render_backward
 * (common.py:880-920: image[p] = sum_i w_ip L_i det_i / sum_i w_ip det_i with the gaussian reconstruction filter, radius 2):
 * per sample i of the primal pass, from its film position (N,2), its radiance (N,3), the gradient image grad_img
 * (height,width,grad_channels >= 3; the first three channels are read) and the primal film accum (height,width,4) [r,g,b,w]:
 *   dL  (N,3)  d loss / d radiance_i
 *   adj (N,3)  d loss / d film_pos_i.x, d loss / d film_pos_i.y, d loss / d det_i   (at det = 1)
 * which epsm_trace_paths_reparam takes as adj_radiance / adj_film.  One kernel, no allocation. */
int epsm_film_adjoint_reparam(int64_t N, const float *film_pos, const float *radiance, const float *grad_img, int grad_channels,
                              const float *accum, int width, int height, float *dL, float *adj, void *stream);

/* epsm_film_splat_tangent -- forward mode of splat + weight division, the transpose of epsm_film_adjoint_reparam (common.py:880-920):
 * per sample i (film position (N,2), radiance (N,3)) and its tangents d_radiance (N,3) and d_film (N,3) = [d pos.x, d pos.y,
 * d det], ACCUMULATES into d_accum (height,width,4), with the filter and footprint of epsm_film_splat,
 *   d_accum[p].rgb += (grad f(p - pos_i) . d pos_i + f d det_i) L_i + f d L_i,   d_accum[p].w += grad f . d pos_i + f d det_i
 * The tangent of the developed image is (d_accum.rgb - image * d_accum.w) / accum.w with the primal film.  d_film may be
 * NULL (colour tangents: the samples stay where they are); with the box filter it must be. */
int epsm_film_splat_tangent(int64_t N, const float *film_pos, const float *radiance, const float *d_radiance, const float *d_film,
                            int width, int height, int rfilter, float *d_accum, void *stream);

/* epsm_probe -- evaluates ONE of the tracer's per-path functions on n rows of plain numbers, on the device, with the very
 * code the tracer runs (csrc/epsm_probe_core.h).  It exists so that the known answers the reference's own unit tests hold
 * for these functions can be checked against the product (tests/golden/reference_vectors.py):
 *   EPSM_PROBE_TEA                in v0, v1 (u32 bits)                          out v0', v1' (bits)     include/mitsuba/core/random.h:77-104  (src/core/tests/test_random.py:9-27)
 *   EPSM_PROBE_PCG32              in initstate lo, hi, initseq lo, hi (bits)    out 6 draws (bits), then 6 x next_1d()   drjit PCG32::seed / next (src/samplers/tests/test_independent.py:16-28)
 *   EPSM_PROBE_SAMPLER            in seed, wavefront index (bits)               out 12 x next_1d() of that path's stream    src/render/sampler.cpp:115-134
 *   EPSM_PROBE_MICROFACET         in m (3), wi (3); cfg = EpsmBsdf (distr, alpha, sample_visible)    out D(m), pdf(wi, m), smith_g1(m, wi)    include/mitsuba/render/microfacet.h (src/render/tests/test_microfacet.py)
 *   EPSM_PROBE_MICROFACET_SAMPLE  in u1, u2; cfg = EpsmBsdf                     out m (3), pdf, d m / d alpha (3)
 *   EPSM_PROBE_FRESNEL            in cos_theta_i, eta                           out F, cos_theta_t, eta_it, eta_ti          include/mitsuba/render/fresnel.h:34-72 (src/render/tests/test_fresnel.py)
 *   EPSM_PROBE_FRESNEL_CONDUCTOR  in cos_theta_i, eta, k                        out F                                        fresnel.h:92-117
 *   EPSM_PROBE_RFILTER            in x                                          out gaussian reconstruction filter at x      src/rfilters/gaussian.cpp (src/rfilters/tests/test_rfilter.py:14-19)
 *   EPSM_PROBE_PRIMARY_RAY        in film position (pixels); cfg = EpsmSensor   out o, d, d_x, d_y (3 each)                  src/sensors/perspective.cpp:238-279 (src/sensors/tests/test_perspective.py:89-135)
 *   EPSM_PROBE_BSDF_SAMPLE        in wi (3), sample1, sample2 (2); cfg = EpsmBsdf out wo (3), weight (3), pdf, eta, sampled_type (bits), valid   src/bsdfs/{diffuse,conductor,roughconductor,dielectric,twosided}.cpp sample() (src/bsdfs/tests/test_dielectric.py:31-158)
 *   EPSM_PROBE_BSDF_EVAL          in wi (3), wo (3); cfg = EpsmBsdf             out value incl. cosine (3), pdf              eval_pdf() (src/bsdfs/tests/test_diffuse.py:13-35, test_twosided.py:29-45)
 *   EPSM_PROBE_MICROFACET_DALPHA  in m (3), v (3); cfg = EpsmBsdf                out d ln D(m) / d alpha, d ln smith_g1(v, m) / d alpha, D(m), smith_g1(v, m)   the closed forms of the roughness adjoint (epsm_trace_paths_bsdf_backward)
 *   EPSM_PROBE_BSDF_DALPHA        in wi (3), wo (3); cfg = EpsmBsdf             out d value / d alpha (3), d ln value / d alpha   roughconductor; 0 for the others
 *   EPSM_PROBE_FRESNEL_CONDUCTOR_GRAD  in cos_theta_i, eta, k                   out F, d F / d eta, d F / d k                the closed forms of the material adjoint (epsm_trace_paths_material_backward; fresnel.h:92-117)
 *   EPSM_PROBE_REPARAM_BSDF       in wi (3), wo (3), seeded (0: wi, else wo); cfg = EpsmBsdf   out rp::bsdf_eval_t<float> (3), the value of rp::bsdf_eval_t<Dual> (3), d value_c / d seeded_k (3 x 3, row c)   the reparameterised passes' own BSDF values (csrc/epsm_trace_reparam.h), which restate eval_pdf()
 *   EPSM_PROBE_REPARAM_FRESNEL    in cos_theta_i, eta, k                        out rp::fresnel_conductor_t<Dual>: F, d F / d cos_theta_i
 * in: (n, EPSM_PROBE_IN) floats, out: (n, EPSM_PROBE_OUT) floats, device pointers; cfg: HOST pointer to the struct named
 * above (NULL otherwise).  Not on any hot path. */
enum { EPSM_PROBE_TEA = 0, EPSM_PROBE_PCG32 = 1, EPSM_PROBE_SAMPLER = 2, EPSM_PROBE_MICROFACET = 3, EPSM_PROBE_MICROFACET_SAMPLE = 4,
       EPSM_PROBE_FRESNEL = 5, EPSM_PROBE_FRESNEL_CONDUCTOR = 6, EPSM_PROBE_RFILTER = 7, EPSM_PROBE_PRIMARY_RAY = 8, EPSM_PROBE_BSDF_SAMPLE = 9,
       EPSM_PROBE_BSDF_EVAL = 10, EPSM_PROBE_MICROFACET_DALPHA = 11, EPSM_PROBE_BSDF_DALPHA = 12,
       EPSM_PROBE_FRESNEL_CONDUCTOR_GRAD = 13, EPSM_PROBE_REPARAM_BSDF = 14, EPSM_PROBE_REPARAM_FRESNEL = 15, EPSM_PROBE_COUNT = 16 };
#define EPSM_PROBE_IN 8
#define EPSM_PROBE_OUT 16
int epsm_probe(int what, int64_t n, const float *in, float *out, const void *cfg, void *stream);

/* epsm_probe_rays -- the ray-query counterpart of epsm_probe: the tracer's own BVH traversal (csrc/epsm_trace_core.h intersect,
 * csrc/epsm_trace_packet.h packet_intersect) on n rays the CALLER gives, with the stack forms the tracer's kernels use.  It exists so
 * that closest-hit and any-hit answers can be checked ray by ray on rays no sensor produces (tests/test_gpu_ray_query.py).
 *   form  EPSM_RAYS_LANE / _LANE_ANY            intersect<false> / intersect<true>, one ray per lane of a 128-lane workgroup on the
 *                                               one-launch kernels' stack: 32 entries per lane in LDS, the rest in a private array
 *         EPSM_RAYS_WAVEFRONT / _WAVEFRONT_ANY  the same on the wavefront kernels' stack: 16 entries per lane in LDS, the rest in
 *                                               `workspace`, entry k of ray i at word (k - 16) n + i
 *         EPSM_RAYS_PACKET                      packet_intersect: rows 64 w .. 64 w + 63 are the lanes of one wave; a lane carries a
 *                                               ray when its row exists and its mask is set; every lane of the wave calls it
 *   scene      only bvh, n_nodes, prim_index and tri_verts are read (n_nodes = 0: every ray misses, nothing is read)
 *   rays       (n,8) f32, device: o (3), d (3), maxt, mask (0 = the row carries no ray: it reports a miss)
 *   out        (n,4) u32, device: triangle id or 0xffffffff, then t, u, v as bits (maxt, 0, 0 for a miss)
 *   workspace  device, >= epsm_probe_rays_workspace_bytes(form, n); scratch.  May be NULL where that is 0
 * EPSM_EINVAL, before any launch: an unknown form, n < 0, a NULL scene / rays / out with n > 0, n_nodes > 0 with a NULL table, a
 * workspace that is NULL or too small.  n = 0 returns EPSM_OK.  Not on any hot path. */
enum { EPSM_RAYS_LANE = 0, EPSM_RAYS_LANE_ANY = 1, EPSM_RAYS_WAVEFRONT = 2, EPSM_RAYS_WAVEFRONT_ANY = 3, EPSM_RAYS_PACKET = 4,
       EPSM_RAYS_FORM_COUNT = 5 };
#define EPSM_RAYS_IN 8
#define EPSM_RAYS_OUT 4
size_t epsm_probe_rays_workspace_bytes(int form, int64_t n);
int epsm_probe_rays(const EpsmScene *scene, int form, int64_t n, const float *rays, uint32_t *out,
                    void *workspace, size_t workspace_bytes, void *stream);

/* epsm_probe_reparam_warps -- STAGE 2 of the reparameterised passes alone (csrc/epsm_trace_reparam.hip: the production kernels
 * epsm_reparam_warp_kernel<G> / epsm_reparam_fwd_warp_kernel<G> through the launcher the passes use), on warp requests the CALLER
 * wrote.  Test infrastructure like epsm_probe_rays: it exists so that what a group of lanes makes of one request -- the drawn
 * auxiliary rays, the harmonic weights, Z, dZ, the adjoint or the tangent -- can be checked request by request against a float64
 * restatement (tests/_warp_oracle.py, tests/test_gpu_warp_stage.py).  Not on any hot path.
 *   workspace  device, 16-byte aligned, >= epsm_trace_reparam_workspace_bytes(N), FILLED BY THE CALLER in the layout stage 1 leaves:
 *              13 x N requests of 16 words, n-major (request n of path i at word 16 (n N + i)):
 *                o (3), gdiv, d (3), em_inv_dist, gdir (3), fb1, ftri (u32; 0xffffffff: the origin is glued to nothing), fb2, 2 pad
 *              rounded up to 256 bytes, then N int32 counts.  Of path i the requests n < min(count[i], n_max) are live, n_max =
 *              min(1 + 2 min(max_depth, 6), 13); nothing else is read or written.  ftri of a live request must be a triangle
 *              of the scene or 0xffffffff: it is not checked.
 *   seed, path_offset   the warp of request n of path i draws as WarpId{0xffffffff ^ seed, path_offset + i, n}
 *   forward == 0  backward: every live request's gdir / gdiv are d loss / d direction, d loss / d divergence; the adjoint is
 *                 ACCUMULATED into grad_pos (V,3) (rows of EPSM_MESH_POS_ATTACHED meshes).  tan_pos is not read.
 *   forward != 0  tan_pos (V,3) is read; every live request's gdir / gdiv are overwritten with d', div'.  grad_pos is not read.
 * EPSM_EINVAL, before any launch: a NULL scene, N < 0, max_depth < 1, path_offset < 0 or path_offset + N > 2^32, a NULL scene array,
 * a NULL grad_pos (backward) / tan_pos (forward), a workspace that is NULL, misaligned or too small, reparam_rays outside 1..64,
 * kappa or exponent <= 0, an unknown flag, a scene without triangles.  N = 0 returns EPSM_OK and touches nothing. */
int epsm_probe_reparam_warps(const EpsmScene *scene, uint32_t seed, int64_t path_offset, int64_t N, int max_depth,
                             int reparam_rays, float kappa, float exponent, uint32_t flags, int forward,
                             float *grad_pos /* backward */, const float *tan_pos /* forward */,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_bvh_build -- the four-wide BVH of T triangles on the device (csrc/epsm_trace_bvh.hip).  Replaces the native scene
 *   construction of the reference (src/render/scene.cpp:66-74, scene_native.inl:10-36: the acceleration structure built
 *   from the shapes) with the rules of the host builder (scene.py build_bvh): a Morton presort of the centroids, binned SAH
 *   (16 bins per axis) while d + 1 + ceil(log2 n) <= 32 and the middle of the Morton-ordered range otherwise, leaves of <= 6
 *   triangles, the four-wide collapse that keeps the tree inside 16 wide levels, and the boxes of epsm_bvh_refit.
 *     positions (V,3) f32, tri (T,3) u32 (every entry < V)         device
 *     nodes       >= epsm_bvh_max_nodes(T) EpsmBvhNode               device, written in breadth-first order (node 0 the root)
 *     prim_index  (T) u32, tri_verts (T,9) f32                       device, the leaf order and the triangles in it
 *     n_nodes, n_levels, level_begin (17 entries)                    HOST: wide level l is nodes [level_begin[l], level_begin[l + 1]),
 *                                                                    level_begin[n_levels] = n_nodes, n_levels <= 16
 *     workspace   device, 16-byte aligned, >= epsm_bvh_workspace_bytes(T): about 177 bytes per triangle; scratch
 *   The build SYNCHRONISES with the host (it reads back the size of every level, about 50 times per build) and returns when
 *   the tree is complete: it cannot be captured in a graph.  Deterministic: two builds of the same input are bit-identical.
 *   EPSM_EINVAL for T < 1, T >= 2^28 (a leaf reference holds first << 3 in 31 bits), V < 1, a NULL pointer or a workspace
 *   that is too small or misaligned -- checked before anything touches the device.
 * ------------------------------------------------------------------------- */
int64_t epsm_bvh_max_nodes(int64_t T);
size_t epsm_bvh_workspace_bytes(int64_t T);
int epsm_bvh_build(const float *positions, int64_t V, const uint32_t *tri, int64_t T,
                   EpsmBvhNode *nodes, uint32_t *prim_index, float *tri_verts,
                   int32_t *n_nodes, int32_t *level_begin, int32_t *n_levels,
                   void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * epsm_bvh_refit -- fresh boxes for moved vertices, same topology (the refit of DeviceBvh, scene.py, which replaces the
 *   reference's Scene::parameters_changed rebuild after a vertex update, src/render/scene.cpp:304-327, scene_native.inl:36-55).  Any breadth-first
 *   tree of this node format -- the host builder's included -- given its level table (HOST pointer, n_levels + 1 entries,
 *   1 <= n_levels <= 16): tri_verts is re-gathered in place in prim_index order, then one launch per wide level, deepest
 *   first, writes every slot's box: absent +-inf; a leaf the min / max of its triangles padded to lo - 1e-6 (1 + |lo|),
 *   hi + 1e-6 (1 + |hi|), rounded step by step (bit-identical to the torch refit); an inner slot the union of its child's
 *   four boxes.  Asynchronous on `stream`; no allocation.
 * ------------------------------------------------------------------------- */
int epsm_bvh_refit(const float *positions, int64_t V, const uint32_t *tri, const uint32_t *prim_index, int64_t T,
                   EpsmBvhNode *nodes, int32_t n_nodes, const int32_t *level_begin, int32_t n_levels,
                   float *tri_verts, void *stream);

/* ---------------------------------------------------------------------------
 * Scene tables on the device (csrc/epsm_trace_scene.hip): what Scene._upload computes with numpy, behind the C ABI, so that a
 * host with no Python builds a traceable scene and moves an emitting mesh without leaving the device.  All four run on `stream`
 * with no host synchronisation and no allocation (scratch comes from the caller, sized by the *_bytes queries; topology and
 * workspace 16-byte aligned), use no float atomics and sum in a fixed order: two calls on the same input give identical bits.
 * EPSM_EINVAL (with epsm_last_error()) for a NULL pointer, a negative count, a too-small workspace or a mesh range outside T /
 * V / cdf_len -- checked on the HOST copies of the tables before anything touches the device.
 *
 * epsm_scene_topology -- the vertex -> (triangle, corner) adjacency of T triangles in CSR form, by a device counting sort
 *   (stable LSD radix sort of the 3 T corner entries by vertex): each vertex's corners in triangle order.  `topology` (device,
 *   >= epsm_scene_topology_bytes(V, T)) is what epsm_vertex_normals reads; rebuild it when the triangles change, not when the
 *   vertices move.  tri (T,3) u32, every entry < V.  1 <= T < 2^28, 1 <= V < 2^31.
 * ------------------------------------------------------------------------- */
size_t epsm_scene_topology_bytes(int64_t V, int64_t T);
size_t epsm_scene_topology_workspace_bytes(int64_t T);
int epsm_scene_topology(const uint32_t *tri, int64_t V, int64_t T, void *topology, size_t topology_bytes,
                        void *workspace, size_t workspace_bytes, void *stream);

/* epsm_vertex_normals -- angle-weighted vertex normals (scene.vertex_normals, Mesh::recompute_vertex_normals): per corner the
 *   normalised face normal times the corner angle acos(clamp(cos, -1, 1)), summed per vertex in triangle order (fp64), then
 *   normalised; a zero sum gives (0, 0, 1).  Written only for the vertex rows [vertex_begin[m], vertex_begin[m + 1]) of the meshes
 *   flagged EPSM_MESH_VERTEX_NORMALS; every other row of `normals` is left as it is.  meshes (n_meshes) and vertex_begin
 *   (n_meshes + 1, non-decreasing, inside 0 .. V) are HOST arrays; a sub-range of a scene's meshes is a valid table.
 *   positions (V,3) f32, tri (T,3) u32, topology (epsm_scene_topology of the same tri), normals (V,3) f32: device. */
int epsm_vertex_normals(const float *positions, int64_t V, const uint32_t *tri, int64_t T, const void *topology,
                        const EpsmMesh *meshes, const int64_t *vertex_begin, int32_t n_meshes, float *normals, void *stream);

/* epsm_vertex_normals_backward / _forward -- the derivative of epsm_vertex_normals with respect to the positions, for the same
 *   table convention (only the vertex rows of the meshes flagged EPSM_MESH_VERTEX_NORMALS are read as normals and written as
 *   positions; every other row of g_pos / d_nrm is left bit for bit).  With N_v the unnormalised sum and n_v = N_v / |N_v|:
 *     backward   g_pos[w] += sum_v (d n_v / d p_w)^T g_nrm[v].  Two launches per run of flagged meshes: a_v = (I - n_v n_v^T)
 *                g_nrm[v] / |N_v| into `workspace` (>= epsm_vertex_normals_backward_bytes(V), 16-byte aligned), then one thread
 *                per vertex w gathers d / d p_w of sum_c a_{i_c} . (theta_c f_t) over its triangles in triangle order;
 *     forward    d_nrm[v] += (I - n_v n_v^T) / |N_v| sum over the corners at v of (d theta f + theta d f): one gather, the exact
 *                transpose, no workspace.
 *   fp64 sums in a fixed order, rounded to float32 once and added: no atomics, two calls give identical bits.  Where the primal
 *   is cut to a constant the derivative is 0: a face normal or a vertex sum of length 0 (or below the 1e-30 floor of its
 *   division), a cosine on or outside [-1, 1], a corner with an edge of length 0, a triangle naming an index >= V.  A position
 *   outside the run of consecutive flagged meshes a vertex belongs to is a constant to that vertex (a mesh's triangles name its own
 *   vertices).  V == 0, T == 0 or an empty table: EPSM_OK, nothing is done.  Arrays as for epsm_vertex_normals; g_nrm, g_pos,
 *   d_pos, d_nrm (V,3) f32: device. */
size_t epsm_vertex_normals_backward_bytes(int64_t V);
int epsm_vertex_normals_backward(const float *positions, int64_t V, const uint32_t *tri, int64_t T, const void *topology,
                                 const EpsmMesh *meshes, const int64_t *vertex_begin, int32_t n_meshes, const float *g_nrm,
                                 float *g_pos, void *workspace, size_t workspace_bytes, void *stream);
int epsm_vertex_normals_forward(const float *positions, int64_t V, const uint32_t *tri, int64_t T, const void *topology,
                                const EpsmMesh *meshes, const int64_t *vertex_begin, int32_t n_meshes, const float *d_pos,
                                float *d_nrm, void *stream);

/* epsm_emitter_tables -- for every mesh of the table, as Scene._upload does: the triangle areas 0.5 |(p1 - p0) x (p2 - p0)| from
 *   the float32 positions, their normalised running sum written to emitter_cdf[cdf_begin .. cdf_begin + tri_count) and their sum
 *   written IN PLACE to meshes_device[m].area (no other field is touched).  fp64 throughout, rounded to float32 once; the last
 *   CDF entry of a mesh of non-zero area is exactly 1.  Chunks of 1024 triangles per workgroup: a mesh of any size spreads over
 *   the whole device.  meshes: HOST copy of meshes_device (same ranges; the kernels read the device table and clip its ranges
 *   to T and cdf_len); a sub-range of a scene's table (pointer and count) updates those meshes only.  The triangle ranges of
 *   the non-empty meshes must not overlap, nor must their CDF ranges (EPSM_EINVAL). */
size_t epsm_emitter_tables_bytes(int64_t T, int32_t n_meshes);
int epsm_emitter_tables(const float *positions, int64_t V, const uint32_t *tri, int64_t T, const EpsmMesh *meshes,
                        EpsmMesh *meshes_device, int32_t n_meshes, float *emitter_cdf, int64_t cdf_len,
                        void *workspace, size_t workspace_bytes, void *stream);

/* epsm_environment_tables -- the EpsmEnvironment arrays of an (height, width, 3) lat-long map `bitmap` (scale applied), the rule
 *   of scene.environment_tables: texels (height, width + 1, 3) with column `width` a copy of column 0; cell weights (mean over a
 *   cell's four corners of luminance x sin theta, fp64); row_cdf (height - 1) and col_cdf (height - 1, width) normalised running
 *   sums with the last entries exactly 1, uniform (linspace) for a zero row or a zero total; cell_pdf (height - 1, width) =
 *   weight / total x width (height - 1), zero for a zero total.  width, height >= 2; all arrays device. */
size_t epsm_environment_tables_bytes(int32_t width, int32_t height);
int epsm_environment_tables(const float *bitmap, int32_t width, int32_t height, float *texels, float *row_cdf, float *col_cdf,
                            float *cell_pdf, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Rigid motions of vertex ranges (csrc/epsm_trace_rigid.hip): what the reference's experiments optimise -- `trafo @
 * initial_positions` of an object, the sensor's pose -- as a reduction of the per-vertex gradient rows the passes produce, and its
 * transpose.  A slot s is a vertex range [ranges[2 s], ranges[2 s + 1]) (clipped to 0 .. V by the kernels; ranges may overlap or be
 * empty) and a pivot pivots[3 s ..]; its twist is a translation dt and a rotation dw about the pivot, world axes.  Both entries
 * run on `stream` with no host synchronisation and no allocation.  ranges (n_slots, 2) i64, pivots (n_slots, 3) f32, positions /
 * normals / g_* / d_* (V, 3) f32: device.  EPSM_EINVAL (with epsm_last_error()) for a NULL pointer, V outside 0 .. 2^31 - 1,
 * n_slots outside 0 .. 65535, n_slots ceil(V / 1024) above 2^23 (the reduce's first launch is a grid of that many workgroups) or a
 * workspace that is too small or misaligned -- checked before anything touches the device.
 *
 * epsm_rigid_reduce -- out (n_slots, 6) += [F, T] per slot: force F = sum_v g_pos[v], torque T = sum_v (x_v - c) x g_pos[v] +
 *   n_v x g_nrm[v] (a rotation turns the stored vertex normals too; g_nrm NULL: no normal term, normals is not read).  float64
 *   sums, no atomics, a fixed order: a first launch writes one row of six doubles per (slot, chunk of 1024 vertices), a second adds
 *   a slot's rows and ADDS the result to out in float32.  Two calls on the same input add the same bits.
 *   workspace: device, 16-byte aligned, >= epsm_rigid_workspace_bytes(V, n_slots) = 48 n_slots ceil(V / 1024) bytes.
 * epsm_rigid_expand -- the transpose: d_pos[v] += dt + dw x (x_v - c), d_nrm[v] += dw x n_v for every slot that contains v, in
 *   slot order; twists (n_slots, 6) f32 = [dt, dw].  d_nrm NULL: positions only.  Vertices in no slot are not written.
 * ------------------------------------------------------------------------- */
size_t epsm_rigid_workspace_bytes(int64_t V, int32_t n_slots);
int epsm_rigid_reduce(const float *positions, const float *normals, const float *g_pos, const float *g_nrm, int64_t V,
                      const int64_t *ranges, const float *pivots, int32_t n_slots, float *out, void *workspace,
                      size_t workspace_bytes, void *stream);
int epsm_rigid_expand(const float *positions, const float *normals, int64_t V, const int64_t *ranges, const float *pivots,
                      const float *twists, int32_t n_slots, float *d_pos, float *d_nrm, void *stream);

/* ---------------------------------------------------------------------------
 * Large-steps vertex updates (csrc/epsm_trace_smooth.hip): the matrix I + lambda L of a mesh on the device, L its unique-edge
 * combinatorial Laplacian, and conjugate gradients on it -- the re-parameterisation u = (I + lambda L) x of Nicolet, Jakob and
 * Jacobson (2021), under which the gradient of u is (I + lambda L)^-1 g_x.  All entries run on `stream` with no host
 * synchronisation and no allocation, use no float atomics and sum in float64 in a fixed order: two calls on the same input give
 * identical bits.  EPSM_EINVAL (with epsm_last_error()) for a NULL pointer, a negative count, a non-finite or negative lambda,
 * max_iters < 1 (or above 65536), a rel_tol outside (0, 1), an unknown form, b == x, or a table / workspace that is too small or
 * not 16-byte aligned -- checked before anything touches the device.  V == 0: EPSM_OK, nothing is done.
 *
 * epsm_mesh_laplacian -- the neighbour table of L from the topology of the same tri (epsm_scene_topology): L_vw = -1 for every
 *   undirected edge {v, w}, v != w, that some triangle has -- once, however many triangles share it (boundary and non-manifold
 *   edges, duplicated triangles) -- and L_vv = the number of distinct neighbours.  `laplacian` (device, 16-byte aligned,
 *   >= epsm_mesh_laplacian_bytes(V, T)) is a CSR table over the topology's own row offsets, two candidate slots per corner: one
 *   thread per vertex keeps the first occurrence of every neighbour at the front of its row, in corner order, fills the rest of
 *   the row with 0xFFFFFFFF (a candidate that repeats an earlier one, equals v or is >= V) and stores the row's degree; that
 *   walk is quadratic in a vertex's valence.  The table's first 32-bit word is the maximum degree, for the host to read once
 *   after the build.  Rebuild it when the triangles change, not when the vertices move.  A vertex no triangle names has degree
 *   0.  tri (T,3) u32.  1 <= T < 2^28, 1 <= V < 2^31.
 * epsm_laplacian_apply -- y = (I + lambda L) x for (V,3) f32 rows: y_v = x_v + lambda (deg_v x_v - sum_w x_w), each row summed
 *   in float64 in table order and rounded to float32 once.  V must be the V the table was built with (the kernels compare it
 *   with the table's own and do nothing otherwise; the solve then writes its info as 0 iterations, not converged, residual -1).
 *   x and y must not overlap.
 * epsm_laplacian_solve -- conjugate gradients on (I + lambda L) x = b, the three columns sharing the gather, each with its own
 *   alpha, beta and convergence state.  x is read as the initial guess and overwritten with the result; b is not written.
 *   Vectors are float32; every dot product is a float64 sum in a fixed order (a lane's rows, the wave by shuffles, the waves in
 *   order, then the chunks of 1024 vertices in order); the CG scalars are float64 in device memory.  A column stops when
 *   |r| / |b| <= rel_tol (r the recurrence's residual); a column with b == 0 gets x == 0 exactly; p.q == 0 makes the column's
 *   step 0.  Convergence is a device word: the launches queued after it is set return at once.  No grid-wide barrier, no
 *   cooperative launch, nothing waits on a flag: where a launch's last workgroup to arrive adds up the chunk rows, it is
 *   found by an integer arrival counter and the order of the sum does not depend on which one it is.
 *   info (device, 3 entries, one per column): the iterations used, whether the column met rel_tol, and the final |r| / |b|
 *   (0 for a zero column).  Not converged after max_iters is no error: EPSM_OK, info says so.  A warm start from the result
 *   of an earlier solve at the same rel_tol may take a few iterations more: the residual recomputed from the float32 x differs
 *   from the recurrence's by up to about kappa 2^-23 |b|, kappa = 1 + 2 lambda max_degree.
 *   form: EPSM_SMOOTH_GRID      any V; one launch per vertex chunk row, two launches per iteration (the gather recomputes
 *                               its neighbours' new search direction r + beta p from the previous one) and two before the first;
 *         EPSM_SMOOTH_ONE_GROUP the whole solve in one launch of one workgroup of 1024 lanes, __syncthreads its only barrier
 *                               (five per iteration: two in each of the two dot products, one after the new direction),
 *                               the search direction in LDS, a lane's rows of r and A p (of x too up to 4 rows per lane) in
 *                               registers.  V <= EPSM_SMOOTH_ONE_GROUP_MAX_V, EPSM_EINVAL above: 12 bytes of LDS per vertex
 *                               next to 768 bytes of reduction rows, (163840 - 768) / 12 = 13589, cut to whole rows of 1024;
 *         EPSM_SMOOTH_AUTO      ONE_GROUP up to the measured crossover (MEASUREMENTS 33), GRID above.
 *   workspace: device, 16-byte aligned, >= epsm_laplacian_solve_bytes(V), whatever the form.
 * ------------------------------------------------------------------------- */
#define EPSM_SMOOTH_AUTO 0
#define EPSM_SMOOTH_GRID 1
#define EPSM_SMOOTH_ONE_GROUP 2
#define EPSM_SMOOTH_ONE_GROUP_MAX_V 13312

typedef struct EpsmSmoothInfo {
    int32_t iterations;     /* CG iterations the column used */
    int32_t converged;      /* 1: |r| / |b| <= rel_tol (or b == 0) */
    double residual;        /* the final |r| / |b| */
} EpsmSmoothInfo;

size_t epsm_mesh_laplacian_bytes(int64_t V, int64_t T);
int epsm_mesh_laplacian(const uint32_t *tri, int64_t V, int64_t T, const void *topology, void *laplacian,
                        size_t laplacian_bytes, void *stream);
int epsm_laplacian_apply(const void *laplacian, int64_t V, double lambda, const float *x, float *y, void *stream);
size_t epsm_laplacian_solve_bytes(int64_t V);
int epsm_laplacian_solve(const void *laplacian, int64_t V, double lambda, const float *b, float *x, int32_t max_iters,
                         double rel_tol, int32_t form, EpsmSmoothInfo *info, void *workspace, size_t workspace_bytes,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif
