"""The reference's integrator surface for the EPSM gradient path.

Mirrors ``EPSMIntegrator`` / ``ManifoldIntegrator`` / ``ManifoldCausticIntegrator``
(src/python/python/ad/integrators/epsm.py:12-306, 744-948, 951-1202) and the plugin
registration the drivers use (``mi.register_integrator`` epsm.py:948,1202;
``mi.load_dict({'type': 'manifold', 'max_depth': d})`` EPSM/optim.py:97-100).

The reference's ``render_backward`` (epsm.py:84-306) is
    trace + log paths  ->  first-vertex tangent  ->  calc_grad  ->  re-trace in
    Backward mode so Dr.Jit scatters into the parameter gradients.
Here the path tracer is whatever object implements ``trace_paths`` (a native
wavefront tracer, or seeded synthetic records for the benchmark); it logs the
vertex INDICES next to the vertex records, so the second trace is replaced by one
scatter kernel.  Everything between the trace and the parameter gradients runs in
three HIP launches (tangent, gradient, scatter) on the current stream.
"""
from __future__ import annotations

from contextlib import contextmanager, nullcontext
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import torch

from . import _lib
from . import dist as _dist
from . import profiler as _prof
from . import replays as _replays
from .film import (_WEIGHT_ONE, develop_tangent, film_adjoint, film_adjoint_reparam, film_adjoint_reparam_torch,  # noqa: F401
                   film_splat_tangent, film_splat_tangent_torch, film_weight_counts)
from .manifold_grad import OUTLIER_CLIP, calc_grad as _calc_grad, manifold_grad_packed
from .params import ParamGrads
from .records import PackedLog, PackedRecords, PackedScatter
from .tangent_scatter import (backward_pass, backward_pass_packed, first_vertex_tangent, manifold_grad_scatter,
                              scatter)


def sample_tea_32(v0: int, v1: int, rounds: int = 4):
    """drjit's ``sample_tea_32`` on two 32-bit integers (the Tiny Encryption Algorithm, 4 rounds by default) -- what the
    sampler seeds its streams with (src/render/sampler.cpp:115-134) and what ``mi.render`` derives the differential
    seed from (src/python/python/util.py:505-508)."""
    v0 &= 0xFFFFFFFF; v1 &= 0xFFFFFFFF
    s = 0
    for _ in range(rounds):
        s = (s + 0x9E3779B9) & 0xFFFFFFFF
        v0 = (v0 + ((((v1 << 4) + 0xA341316C) ^ (v1 + s) ^ ((v1 >> 5) + 0xC8013EA4)) & 0xFFFFFFFF)) & 0xFFFFFFFF
        v1 = (v1 + ((((v0 << 4) + 0xAD90777D) ^ (v0 + s) ^ ((v0 >> 5) + 0x7E95761E)) & 0xFFFFFFFF)) & 0xFFFFFFFF
    return v0, v1


def render_seeds(seed: int, seed_grad: int = 0):
    """(seed, seed_grad) of one ``mi.render`` call, src/python/python/util.py:505-513: the differential pass gets its OWN
    seed -- ``sample_tea_32(seed, 1)[0]`` unless the caller names one -- because ``grad_in`` is a function of the primal
    image: replaying the very samples whose noise it carries correlates the two factors of the estimator and biases the
    gradient (E[grad] picks up a variance-gradient term).  An explicit ``seed_grad == seed`` is refused with the
    reference's message."""
    if seed_grad == 0:
        seed_grad = sample_tea_32(seed, 1)[0]
    elif seed_grad == seed:
        raise Exception('The primal and differential seed should be different '
                        'to ensure unbiased gradient computation!')
    return seed, seed_grad


@dataclass
class PathTrace:
    """What one logging trace of the backward sensor yields (epsm.py:166-181, 547, 648-654)
    plus the parameter addressing of every logged vertex."""
    res: int                      # film side of the backward sensor
    spp: int
    ray_o: torch.Tensor           # (N,3) primary rays, N = res*res*spp ordered (pixel, sample)
    ray_d: torch.Tensor
    ray_dx: torch.Tensor
    ray_dy: torch.Tensor
    path_info: List[dict]         # [{"cam"}, vertex 1, ..., vertex K]
    scatter_info: List[dict]      # K entries (EpsmScatterRecord fields)
    path_offset: int = 0          # first path of this shard within the full wavefront
    n_paths_total: Optional[int] = None
    log: Optional[PackedLog] = None   # the native log (then path_info / scatter_info may be None)
    ior_grads: bool = False           # the tracer had an IOR slot (Scene.attach_ior): aux[1] of a refraction is d eta / d int_ior


def _max_depth_property(props: dict):
    """``max_depth`` of an integrator's properties (common.py:31-37); -1 = infinite (the reference stores 0xffffffff)."""
    max_depth = props.get("max_depth", 6)
    if max_depth < 0 and max_depth != -1:
        raise Exception("\"max_depth\" must be set to -1 (infinite) or a value >= 0")
    return max_depth


def _replay_depth(max_depth) -> int:
    """``max_depth`` as the tracer's logging and replaying passes take it: their path loop stops after 6 bounces whatever the
    integrator says (epsm.py:549) and -1 means "no limit" (common.py:31-37)."""
    return 6 if max_depth < 0 else min(int(max_depth), 6)


class EPSMIntegrator:
    """Base class; ``variant`` selects the calc_grad flavour."""
    variant: str = ""

    def __init__(self, props: Optional[dict] = None):
        props = dict(props or {})
        self.max_depth = _max_depth_property(props)
        self.rr_depth = props.get("rr_depth", 5)        # common.py:39-41
        if self.rr_depth <= 0:
            raise Exception("\"rr_depth\" must be set to a value greater than zero!")
        # hard-coded in the reference (epsm.py:142,145,549,648,932-944); explicit options here
        self.backward_sensor = props.get("backward_sensor", 2)
        self.backward_spp = props.get("backward_spp", 8)
        self.fuse_tangent = bool(props.get("fuse_tangent", True))   # with `fused`: epsm_backward_pass (one launch per tile)
        self.max_log_depth = min(props.get("max_log_depth", 5), 5)
        self.outlier_clip = props.get("outlier_clip", OUTLIER_CLIP)
        # True: calc_grad and the scatter run as ONE kernel (no dense per-path gradient lists);
        # False: the reference's two-stage shape (calc_grad lists, then scatter)
        self.fused = props.get("fused", True)
        # True: render_backward asks the tracer for the native packed log (one 128-byte record per path vertex) and runs
        # epsm_backward_pass_packed on it; False: the reference's per-field tensors all the way
        self.packed_log = bool(props.get("packed_log", True))
        # True: the backward trace retires a path as soon as nothing behind its last logged vertex can reach calc_grad
        # (EPSM_TRACE_GRADIENT_ONLY, include/epsm_trace.h): identical gradients, the image of that pass -- which the 5-channel
        # branch never uses (epsm.py:729-732) -- is not formed
        self.gradient_only = bool(props.get("gradient_only", True))
        # True: with the native log and the gradient-only trace, the stage that shades a path's FIRST hit also does what the backward
        # pass would do for a path without a chain (EPSM_TRACE_FUSE_FIRST_HIT, include/epsm_trace.h: first-vertex rows, d / d ray.o);
        # such paths -- most of a real wavefront -- are neither logged nor read again.  Same sums.
        self.fuse_first_hit = bool(props.get("fuse_first_hit", True))

    def to_string(self):
        md = 0xFFFFFFFF if self.max_depth < 0 else self.max_depth
        return f"{type(self).__name__}[max_depth = {md}, rr_depth = {self.rr_depth}]"

    __repr__ = to_string

    # -- calc_grad: drop-in -------------------------------------------------
    def calc_grad(self, path_info, dlduv, dldp, Lt=None):
        """epsm.py:745 / 952 -- same arguments and return structure."""
        return _calc_grad(self.variant, path_info, dlduv, dldp, Lt, clip=self.outlier_clip)

    # -- primal -------------------------------------------------------------
    def render(self, scene, sensor=0, seed=0, spp=0, develop=True, evaluate=True):
        """epsm.py:13-82: primal image with two zero channels appended, (H,W,5); the
        5-channel shape is what makes the driver take the EPSM branch (EPSM/optim.py:130)."""
        if not develop:
            raise Exception("develop=True must be specified when invoking AD integrators")
        if not hasattr(scene, "render_primal"):
            raise NotImplementedError("scene object has no render_primal(sensor, seed, spp, max_depth)")
        with _prof.phase("epsm.render.primal"):
            img = scene.render_primal(sensor=sensor, seed=seed, spp=spp, max_depth=self.primal_depth())
        pad = torch.zeros(img.shape[0], img.shape[1], 2, device=img.device, dtype=img.dtype)
        self.primal_image = torch.cat([img[..., :3], pad], dim=-1)
        return self.primal_image

    def primal_depth(self) -> int:
        """The primal pass has no 6-bounce cap (recorded loop, epsm.py:308-501); -1 = as deep as the tracer goes."""
        return 1 << 20 if self.max_depth < 0 else int(self.max_depth)

    # -- backward -----------------------------------------------------------
    def render_backward(self, scene, params: ParamGrads, grad_in: torch.Tensor,
                        sensor=0, seed: int = 0, spp: int = 0) -> None:
        """epsm.py:84-306.  ``sensor`` and ``spp`` are ignored exactly as the reference
        ignores them (epsm.py:142,145): the backward pass uses ``backward_sensor`` and
        ``backward_spp``.  Gradients are ACCUMULATED into ``params`` (as dr.backward does).

        An index of refraction attached with ``Scene.attach_ior`` gets its gradient HERE, in the 5-channel branch, and only here:
        the refraction direction depends on the IOR, which the detached sampling of the colour adjoint cannot see,
        so the 3-channel branch, ``prb`` and ``prb_reparam`` leave its slot of ``params.alpha`` at zero."""
        if grad_in.shape[-1] == 3:
            # epsm.py:230-234: a 3-channel gradient image is the colour adjoint deltaL = grad_in of the PRB replay, on
            # the sensor and sample count the caller names (the 5-channel branch alone ignores them, epsm.py:142-145).
            # The manifold integrators move geometry through channels 3, 4 only (epsm.py:729-732 leaves the colour
            # adjoint's propagation into geometry commented out): what a 3-channel image can reach are the colour
            # parameters attached to the scene.
            return self._prb().render_backward(scene, params, grad_in, sensor=sensor, seed=seed, spp=spp)
        # The one place that is handed something other than a `Scene` -- `SyntheticScene`, bench.py's records: any object with
        # `trace_paths`.  What such an object may leave out is read here, by name with a default, and nowhere else.
        tracer = getattr(scene, "iter_traces", None) or scene.trace_paths      # a generator: one tile resident at a time
        packed_log = getattr(scene, "supports_packed_log", False)
        gradient_only = getattr(scene, "supports_gradient_only", False)
        first_hit = getattr(scene, "supports_first_hit_fusion", False)
        rigid_slots = getattr(scene, "rigid_slots", ())
        if getattr(scene, "alpha_map_slots", lambda: ())():
            # the logged half vector depends on alpha, so the map's gradient is not zero here -- and the record carries no uv to
            # scatter it by
            raise NotImplementedError("the 5-channel manifold branch has no gradient for a roughness map (a '<bsdf>.alpha.data' slot "
                                      "is attached): the vertex log carries no texture coordinates to scatter it by; `prb` "
                                      "differentiates it (a 3-channel gradient image)")
        if getattr(scene, "sensor_rotation", False):
            # this branch transports d / d ray.o alone (epsm.py:260-261): the sensor's rotation has no term in it
            raise NotImplementedError("the 5-channel manifold branch differentiates the sensor's position only (epsm.py:260-261); the "
                                      "gradient of its rotation is `prb_reparam`'s (attach_sensor(rotation=True))")
        # An attached index of refraction (Scene.attach_ior): the backward kernel takes the scalar row of a refraction vertex for
        # d / d eta_k x d eta / d int_ior (EPSM_OPT_IOR_GRADS).  The option is process-wide: set on EVERY call, 1 or 0,
        # from the scene in hand, and back at 0 when the call ends (_ior_option); only the launches with in-kernel tangents have
        # that instantiation.
        ior = bool(getattr(scene, "ior_slots", ()))
        if ior and not (self.fused and self.fuse_tangent):
            raise NotImplementedError("an index of refraction is attached (attach_ior): its gradient is formed by the fused backward "
                                      "pass alone (fused=True, fuse_tangent=True); the unfused stages and the entry point that "
                                      "takes precomputed tangents cannot fill the slot")
        rank, world = _dist.world()
        with _ior_option(ior), _call_contribution(scene, params, _rigid_slot_count(rigid_slots, params)) as target:
            kw = {}
            if self.fused and self.fuse_tangent and self.packed_log and packed_log:
                kw["packed_log"] = True        # the tracer writes the backward kernel's native layout (EpsmPackedLog)
            if self.gradient_only and gradient_only:
                kw["gradient_only"] = self.variant
                if self.fuse_first_hit and kw.get("packed_log") and first_hit:
                    kw["first_hit"] = (grad_in if grad_in.is_contiguous() else grad_in.contiguous(), target, self.outlier_clip, True)
            traces = tracer(sensor=self.backward_sensor, seed=seed, spp=self.backward_spp,
                            max_depth=self.tracer_depth(), max_log_depth=self.max_log_depth, rank=rank, world_size=world,
                            sparse_log=True,   # the log is consumed here and nowhere else: skip the zeros of dead bounces
                            **kw)
            if isinstance(traces, PathTrace):
                traces = [traces]
            traces = iter(traces)
            while True:                                # this rank's pixel/sample tiles
                with _prof.phase("epsm.render_backward.trace"):          # (a generator: the tile is traced when asked for)
                    trace = next(traces, None)
                if trace is None:
                    break
                with _prof.phase("epsm.render_backward.backward_pass"):
                    self.backward_from_trace(trace, target, grad_in)
                del trace

    # -- forward ------------------------------------------------------------
    def render_forward(self, scene, params: ParamGrads, sensor=0, seed: int = 0, spp: int = 0) -> torch.Tensor:
        """common.py:118-197: d image / d theta . delta theta, (H,W,3), for the tangent ``params`` (laid out like the gradients
        of ``render_backward``).  The transpose of the 3-channel branch of ``render_backward``: the ``prb`` forward pass at this
        integrator's depths -- the attached colour parameters; geometry tangents contribute nothing, as that branch leaves the
        geometry alone.  The 5-channel branch transports a requested pixel motion (epsm.py:236-272) and is no adjoint of a
        rendered quantity: it has no forward form."""
        return self._prb().render_forward(scene, params, sensor=sensor, seed=seed, spp=spp)

    def _prb(self) -> "PRBIntegrator":
        """The colour phase at this integrator's depths: what the 3-channel branch and ``render_forward`` delegate to."""
        return PRBIntegrator({"max_depth": self.max_depth, "rr_depth": self.rr_depth})

    def tracer_depth(self) -> int:
        """``max_depth`` as the backward trace takes it (``_replay_depth``)."""
        return _replay_depth(self.max_depth)

    def backward_from_trace(self, trace: PathTrace, params: ParamGrads, grad_in: torch.Tensor,
                            packed=None, out=None, mark: Optional[Callable[[str], None]] = None,
                            fused: Optional[bool] = None):
        """Tangent -> gradient -> scatter for one tile.  ``packed`` = (PackedRecords, PackedScatter)
        built once for records that stay resident; ``out`` = reusable output tensors; ``mark(name)`` is
        called after each stage (bench.py records HIP events there).

        A trace of a scene with an IOR slot (``trace.ior_grads``, set by ``Scene``) carries d eta / d int_ior in ``aux[1]`` of its
        refractions: it must be read under EPSM_OPT_IOR_GRADS, or the roughness rule would add ``gm.x * aux[1]`` -- garbage -- to
        the IOR slot.  So the option is taken from the trace here, for the launch, and the routes without the ``IOR``
        instantiations (unfused stages, precomputed tangents) refuse such a trace."""
        mark = mark or (lambda name: None)
        fused_now = self.fused if fused is None else fused
        if trace.ior_grads and not (isinstance(packed, PackedLog) or trace.log is not None or (fused_now and self.fuse_tangent)):
            raise NotImplementedError("the trace carries an index-of-refraction slot (attach_ior): only the fused backward pass with "
                                      "in-kernel tangents can fill it")
        with _ior_option(trace.ior_grads):
            return self._backward_from_trace(trace, params, grad_in, packed, out, mark, fused)

    def _backward_from_trace(self, trace, params, grad_in, packed, out, mark, fused):
        if isinstance(packed, PackedLog) or trace.log is not None:
            # the native log (one 128-byte record per path vertex): one launch, nothing else
            log = packed if isinstance(packed, PackedLog) else trace.log
            mark("tangent")
            # (a log traced under EPSM_TRACE_FUSE_FIRST_HIT: d / d ray.o and the paths without a chain are in the buffers already)
            backward_pass_packed(self.variant, log, grad_in, trace.spp, trace.res, params.pos, params.nrm,
                                 params.alpha if params.B else None, None if log.first_hit_done else params.cam_origin,
                                 clip=self.outlier_clip, path_offset=trace.path_offset)
            mark("grad"); mark("scatter")
            return None
        dev = trace.ray_d.device
        rec, sc = packed if packed is not None else (PackedRecords(trace.path_info, device=dev),
                                                     PackedScatter(trace.scatter_info, device=dev))
        fused = self.fused if fused is None else fused
        if fused and self.fuse_tangent:
            # one launch for the whole tile: tangents live in registers, gradients go into the parameter buffers
            mark("tangent")
            backward_pass(self.variant, rec, sc, trace.ray_o, trace.ray_d, trace.ray_dx, trace.ray_dy, grad_in,
                          trace.spp, trace.res, params.pos, params.nrm, params.alpha if params.B else None,
                          params.cam_origin, clip=self.outlier_clip, path_offset=trace.path_offset)
            mark("grad"); mark("scatter")
            return None
        first = trace.path_info[1]
        dlduv, dldp, grad_o = first_vertex_tangent(
            trace.ray_o, trace.ray_d, trace.ray_dx, trace.ray_dy, grad_in, trace.spp, trace.res,
            first["points"][0], first["points"][1], first["points"][2], first["active"],
            dlduv_width=2, want_origin_grad=True, path_offset=trace.path_offset)
        mark("tangent")
        if fused:
            # gradients go from registers into the parameter buffers
            manifold_grad_scatter(self.variant, rec, sc, dlduv, dldp, params.pos, params.nrm,
                                  params.alpha if params.B else None, clip=self.outlier_clip)
            params.cam_origin += grad_o
            mark("grad")
            mark("scatter")
            return None
        out = manifold_grad_packed(self.variant, rec, dlduv, dldp, clip=self.outlier_clip, dlduv_cols=2, out=out)
        mark("grad")
        scatter(self.variant, rec, sc, *out, params.pos, params.nrm, params.alpha if params.B else None)
        params.cam_origin += grad_o
        mark("scatter")
        return out


class ManifoldIntegrator(EPSMIntegrator):
    variant = "manifold"


@contextmanager
def _ior_option(on: bool):
    """EPSM_OPT_IOR_GRADS = ``on`` for the launches of a block, and 0 -- its default -- behind it, whatever it was and however
    the block ends: the option is process-wide, belongs to the integrators, and must not outlive the call (a later launch with
    precomputed tangents would be refused, a later default launch would run the slower ``IOR`` instantiations)."""
    lib = _lib.lib()
    _lib.check(lib.epsm_set_option(_lib.OPT_IOR_GRADS, int(bool(on))), "epsm_set_option")
    try:
        yield
    finally:
        lib.epsm_set_option(_lib.OPT_IOR_GRADS, 0)


class ManifoldCausticIntegrator(EPSMIntegrator):
    variant = "manifold_caustic"


def _pass_frame(scene, sensor: int, spp: int, kind: str):
    """What a pass over a sensor's wavefront starts from, resolved once for a ``(scene, sensor, spp)`` triple: the sensor's index
    and the sensor, the sample count, the world size, the zero film (H,W,4) [r,g,b,w] the primal estimates are splatted into, and
    this rank's tiles of the ``kind`` plan (``Scene.tile_plan``)."""
    si = min(sensor, len(scene.sensors) - 1)
    s = scene.sensors[si]
    spp = spp or s.spp
    rank, world = _dist.world()
    accum = torch.zeros((s.height, s.width, 4), device=scene.device, dtype=torch.float32)
    return si, s, spp, world, accum, scene.tile_plan(s.wavefront_size(spp), kind, rank, world)


def _refuse_box_filter(sensor) -> None:
    if sensor.rfilter == 0:
        raise Exception("ADIntegrator detected the potential for image-space motion due to differentiable shape or camera "
                        "pose parameters. This is, however, incompatible with the box reconstruction filter that is "
                        "currently used. Please specify a smooth reconstruction filter in your scene description (e.g. "
                        "'gaussian', which is actually the default)")          # common.py:379-388


def _develop_forward(scene, sensor: int, films) -> torch.Tensor:
    """Sums the image tangents of the (primal film, tangent film) pairs of a forward pass (None: a pass that had nothing
    attached); with several ranks ONE all-reduce of all of them first."""
    s = scene.sensors[min(sensor, len(scene.sensors) - 1)]
    out = torch.zeros((s.height, s.width, 3), device=scene.device, dtype=torch.float32)
    films = [pair for pair in films if pair is not None]
    if not films:
        return out
    _, world = _dist.world()
    if world > 1:
        flat = torch.stack([t for pair in films for t in pair])
        _dist.allreduce_param_grads(flat)
        films = [(flat[2 * k], flat[2 * k + 1]) for k in range(len(films))]
    for accum, d_accum in films:
        out += develop_tangent(accum, d_accum)
    return out


def _rigid_slot_count(rigid_slots, params: ParamGrads) -> int:
    """The number of rigid slots (``Scene.rigid_slots``, from ``Scene.attach_rigid``); ``params.rigid`` must hold them."""
    n = len(rigid_slots)
    if n and params.R < n:
        raise ValueError("rigid slots are attached: the gradient buffer must come from Scene.param_grads() after attach_rigid")
    return n


def _rigid_backward(scene, params: ParamGrads, contrib: ParamGrads, n: int) -> None:
    """``params.rigid`` += [force, torque] of the ``n`` rigid slots over ONE call's contribution to the vertex rows, after its sum
    over the ranks (``epsm_rigid_reduce``: float64, a fixed order -- every rank adds the same bits)."""
    if n:
        with _prof.phase("epsm.render_backward.rigid_reduce"):
            scene.rigid_reduce(contrib.pos, contrib.nrm, params.rigid[:n], *scene.rigid_tables())


def _normals_chain_backward(scene, params: ParamGrads, contrib: ParamGrads) -> None:
    """``params.pos`` += ONE call's ``nrm`` rows, after their sum over the ranks, carried through the recomputed vertex normals of
    the meshes attached with ``recomputed_normals`` (``epsm_vertex_normals_backward``: float64, a fixed order -- every rank adds
    the same bits).  It goes into ``params`` and not into ``contrib``: the rigid slots and the sensor's pass reduce ``contrib``
    with their own n x g_nrm term, which is this chain's torque already (sum_w x_w x (J^T g)_w = sum_v n_v x g_v)."""
    with _prof.phase("epsm.render_backward.normals_chain"):
        scene.normals_backward(contrib.nrm, params.pos)


@contextmanager
def _call_contribution(scene, params: ParamGrads, n_rigid: int, add: Optional[Callable[[ParamGrads], None]] = None):
    """The buffer ONE ``render_backward`` writes its geometry gradients into.  dr.backward ACCUMULATES into the gradients that
    are already there, and with more than one rank only THIS call's contribution may be summed over the ranks: what ``params``
    held on entry is already a sum over the ranks (or the caller's own data) and must not be multiplied by the world size.  The
    rigid slots reduce this call's contribution too, the sensor's pass (``add``) sums every vertex row of it, and a mesh attached
    with ``recomputed_normals`` has this call's ``nrm`` rows carried back to ``pos``.  So: ``params`` itself with one rank, no
    rigid slot, no such mesh and no ``add``; else ``params.scratch()``, and on exit, in this order, ONE all-reduce of the whole
    buffer when there are several ranks, the normals' chain of this call's rows into ``params.pos``, ``params.flat += `` the
    buffer (or ``add(contribution)`` in its place), the rigid slots' reduction."""
    world = _dist.world()[1]
    chained = getattr(scene, "has_recomputed_normals", lambda: False)()       # (bench.py's SyntheticScene has no meshes to flag)
    if world == 1 and not n_rigid and add is None and not chained:
        yield params
        return
    target = params.scratch()
    yield target
    if world > 1:
        with _prof.phase("epsm.render_backward.allreduce"):
            _dist.allreduce_param_grads(target.flat)
    if chained:
        _normals_chain_backward(scene, params, target)
    if add is None:
        params.flat += target.flat
    else:
        add(target)
    _rigid_backward(scene, params, target, n_rigid)


def _pose_attached(scene, params: ParamGrads, what: str):
    """(sensor attached?, its rotation too?, number of rigid slots) of a `prb_reparam` call.  Refuses what the every-shape-moves
    argument of the sensor's pass cannot carry, and a ``params`` (``what``: "gradient buffer" / "tangent") laid out before the
    rotation or the slots were attached -- before any pass runs: a refused call leaves nothing behind."""
    cam = rot = False
    if scene.has_alpha_map() and (scene.sensor_attached or scene.has_attached_geometry() or scene.rigid_slots):
        # the point a ray sees slides over the map: d f / d alpha x d alpha / d uv x d uv / d theta needs alpha as a dual number
        # in bsdf_eval_t -- without it the geometry's gradient would silently lack a term
        raise NotImplementedError("prb_reparam: the scene has a roughness map (a roughconductor whose alpha is a bitmap) and geometry "
                                  "or the sensor is attached -- the term through the map's uv derivative is not differentiated "
                                  "here; with nothing geometric attached prb_reparam differentiates the map itself")
    if scene.sensor_attached:
        if any(e["type"] == 1 for e in scene.emitter_desc):
            raise NotImplementedError("prb_reparam: a `point` emitter's position would have to move with the shapes for the "
                                      "sensor's gradient; scenes with point emitters keep the sensor fixed")
        cam, rot = True, scene.sensor_rotation
        if rot and any(e["type"] == 3 for e in scene.emitter_desc):
            raise NotImplementedError("prb_reparam: an `envmap` would have to turn with the shapes for the gradient of the sensor's "
                                      "rotation; scenes with an envmap take attach_sensor(rotation=False)")
        if rot and params.cam_rotation is None:
            raise ValueError(f"the sensor's rotation is attached: the {what} must come from Scene.param_grads() after "
                             "attach_sensor(rotation=True)")
    return cam, rot, _rigid_slot_count(scene.rigid_slots, params)


class _EveryMeshAttached:
    """For the duration of the sensor's pass: the positions of every mesh attached and, for the rotation, the normals of the
    meshes that have vertex normals (a rotation turns them too).  ``was``: (mesh, positions attached, normals attached) before."""

    def __init__(self, scene, normals: bool):
        self.scene, self.normals = scene, normals
        self.was = [(m, bool(m.pos_attached), bool(m.nrm_attached)) for m in scene.meshes]

    def __enter__(self):
        for m, _, n in self.was:
            m.pos_attached = True
            if self.normals:
                m.nrm_attached = bool(n or m.has_normals)
        self.scene._refresh_attach_flags(sync_host=False)
        return self

    def __exit__(self, *exc):
        for m, p, n in self.was:
            m.pos_attached, m.nrm_attached = p, n
        self.scene._refresh_attach_flags(sync_host=False)
        return False


class PRBIntegrator:
    """Second phase of the reference's ``*_hybrid`` scheme (EPSM/optim.py:87-94, 113-119 switch to ``prb_reparam`` after
    ``thres`` iterations): a 3-channel image and the COLOUR adjoint -- ``render_backward`` takes ``grad_in (H,W,3)``
    (the branch of epsm.py:230-234) and accumulates d sum(image * grad_in) / d theta for the colour parameters attached
    to the scene (``Scene.attach_color``: diffuse reflectances, ``Scene.attach_radiance``: emitters) into
    ``params.color``.  Path replay with detached sampling as in prb.py: one pass of ``epsm_trace_paths_color`` under the
    primal pass's seed returns, per path, the radiance and its derivative sums; the film's adjoint turns ``grad_in``
    into the adjoint radiance of every sample.  This class is ``prb`` (prb.py): colour parameters only, ``reparam`` is
    False and geometry receives nothing.  What ``prb_reparam`` adds on top -- the warp field that makes visibility
    differentiable, i.e. gradients of vertex positions and normals through shading, silhouettes and shadow boundaries
    (ad/reparam.py) -- is the subclass ``PRBReparamIntegrator`` below (csrc/epsm_trace_reparam.h)."""
    reparam = False

    def __init__(self, props: Optional[dict] = None):
        props = dict(props or {})
        self.max_depth = _max_depth_property(props)
        self.rr_depth = props.get("rr_depth", 5)        # (not validated here: the C entries refuse rr_depth < 1)

    def _depth(self) -> int:
        """Depth of BOTH passes: ``epsm_trace_paths_color`` replays at most 6 bounces, and the image the adjoint is paired
        with must come from the same estimator (render() went to the full max_depth, the replay to 6)."""
        return _replay_depth(self.max_depth)

    def to_string(self):
        return f"PRBIntegrator[max_depth = {self.max_depth}, rr_depth = {self.rr_depth}, reparam = False]"

    __repr__ = to_string

    def render(self, scene, sensor=0, seed=0, spp=0, develop=True, evaluate=True):
        if not develop:
            raise Exception("develop=True must be specified when invoking AD integrators")
        self.primal_image = scene.render_primal(sensor=sensor, seed=seed, spp=spp, max_depth=self._depth())[..., :3]
        return self.primal_image

    def render_backward(self, scene, params: ParamGrads, grad_in: torch.Tensor, sensor=0, seed: int = 0, spp: int = 0) -> None:
        """Accumulates into ``params.color`` (one all-reduce of this call's contribution when there are several ranks)."""
        self._color_backward(scene, params, grad_in, sensor, seed, spp)

    def render_forward(self, scene, params: ParamGrads, sensor=0, seed: int = 0, spp: int = 0) -> torch.Tensor:
        """common.py:118-197: the image's tangent d image / d theta . delta theta (H,W,3) for the tangent ``params`` (its
        ``color`` rows: the attached colour parameters), under the estimator and the random numbers of ``render`` /
        ``render_backward`` with the same seed and spp -- the exact transpose of ``render_backward``."""
        return _develop_forward(scene, sensor, [self._color_forward(scene, params, sensor, seed, spp)])

    def _color_attached(self, scene, params: ParamGrads, what: str):
        """(anything for the colour pass?, the attached replays in the order of ``replays.REPLAYS``); ``params`` (``what``:
        "gradient buffer" / "tangent") must be laid out for their sections -- refused before any pass runs.  Neither a colour nor
        a replay attached is nothing this phase differentiates: skipped -- and refused by `prb` when geometry is attached
        instead."""
        active = _replays.attached(scene)
        for section in _replays.sections(active):
            section.check(scene, params, what)
        if not scene.color_slots and not active and not self.reparam and scene.has_attached_geometry():
            raise NotImplementedError(
                "prb: geometry is attached but no colour parameter is -- `prb` differentiates colours only (prb.py); the "
                "gradients of vertex positions through visibility are what `prb_reparam` (its warp field: "
                "csrc/epsm_trace_reparam.h) or the manifold integrators compute")
        return bool(scene.color_slots or active), active

    def _color_forward(self, scene, params: ParamGrads, sensor=0, seed: int = 0, spp: int = 0):
        """The transpose of ``_color_backward``: per path dL = sum_c sums[:, c] * dcolor[c] / value[c], splatted with the
        primal pass's film weights, plus d radiance of every attached replay (``Scene.replay_forward``) for its section's tangent:
        the texels of the attached textures, ``params.alpha`` of the attached roughconductors, ``params.conductor`` of the attached
        conductors, the envmap's pose ``params.env_rotation`` / ``env_scale``.  Returns this rank's (primal film,
        tangent film), or None when none of them is attached.  (The tangent film is developed with the film's own float-atomic
        weights, while the backward pass of a call with a reducing replay divides by their fixed-point sums: ~1e-7 apart,
        far inside the transpose identity's bound.)"""
        any_attached, active = self._color_attached(scene, params, "tangent")
        if not any_attached:
            return None
        si, s, spp, _, accum, tiles = _pass_frame(scene, sensor, spp, "color")
        d_accum = torch.zeros_like(accum)
        values = scene.color_values()                                   # (C,3)
        t = params.color.to(scene.device, torch.float32)[: values.shape[0]] / values.clamp_min(1e-12)
        tangents = {section: section.tangent(scene, params) for section in _replays.sections(active)}
        for lo, hi in tiles:
            film_pos, radiance, sums = scene.trace_color(si, seed, spp, self._depth(), lo, hi)
            scene.film_splat(accum, s, film_pos, radiance)
            dL = (sums * t[None]).sum(dim=1)                            # (n,3)
            for r in active:
                dL = dL + scene.replay_forward(r, si, seed, spp, self._depth(), lo, hi, radiance.contiguous(), tangents[r.section])
            film_splat_tangent(d_accum, film_pos, radiance, dL, None, s.rfilter)
        return accum, d_accum

    def _color_backward(self, scene, params: ParamGrads, grad_in: torch.Tensor, sensor=0, seed: int = 0, spp: int = 0) -> None:
        any_attached, active = self._color_attached(scene, params, "gradient buffer")
        if not any_attached:
            return
        exact = any(r.reduces for r in active)                          # the call must repeat bit for bit: fixed-point film weights
        si, s, spp, world, accum, tiles = _pass_frame(scene, sensor, spp, "color")
        kept, counts = [], None
        for lo, hi in tiles:
            film_pos, radiance, sums = scene.trace_color(si, seed, spp, self._depth(), lo, hi)
            scene.film_splat(accum, s, film_pos, radiance)
            kept.append((film_pos, sums, radiance.contiguous() if active else None))
            if exact:
                if counts is None:
                    counts = torch.zeros((s.height, s.width), device=scene.device, dtype=torch.int64)
                film_weight_counts(counts, film_pos, s.rfilter)
        if world > 1:
            _dist.allreduce_param_grads(accum)
            if exact:
                _dist.allreduce_param_grads(counts)
        # (with a reducing replay attached the call repeats bit for bit: the weights the film adjoint divides by are the exact sums)
        weight_img = accum[..., 3] if not exact else (counts.double() / _WEIGHT_ONE).float()
        g = grad_in.to(scene.device, torch.float32)[: s.height, : s.width, :3]
        values = scene.color_values()                                   # (C,3)
        contrib = torch.zeros_like(values)
        # per section (the two texel replays share one): the tensor this call all-reduces, the buffer the replays accumulate into
        bufs = {section: section.zeros(scene, params) for section in _replays.sections(active)}
        for (lo, hi), (film_pos, sums, radiance) in zip(tiles, kept):
            dL = film_adjoint(film_pos, g, weight_img, s.rfilter)       # (n,3)
            contrib += (sums * dL[:, None, :]).sum(dim=0)
            for r in active:                                            # each a replay of the same paths
                scene.replay_backward(r, si, seed, spp, self._depth(), lo, hi, radiance, dL.contiguous(), bufs[r.section][1])
        contrib = contrib / values.clamp_min(1e-12)
        if world > 1:
            _dist.allreduce_param_grads(contrib)
        params.color += contrib
        for section, (flat, buf) in bufs.items():
            if world > 1:
                _dist.allreduce_param_grads(flat)                       # this call's contribution to the section, once
            section.deposit(scene, params, buf)


class PRBReparamIntegrator(PRBIntegrator):
    """``prb_reparam`` (src/python/python/ad/integrators/prb_reparam.py): path replay with detached sampling PLUS the
    reparameterisation of Bangaru et al. that makes visibility differentiable -- ``render_backward`` accumulates
    d sum(image * grad_in) / d vertex positions (and vertex normals) of the attached meshes into ``params.pos`` /
    ``params.nrm`` through silhouettes, shadow boundaries and shading, and the colour adjoint of ``PRBIntegrator`` into
    ``params.color``.  Properties as in prb_reparam.py:226-250: ``reparam_max_depth`` (default: max_depth),
    ``reparam_rays`` (16; at most 64 here), ``reparam_kappa`` (1e5), ``reparam_exp`` (3.0), ``reparam_antithetic`` (False:
    auxiliary rays in mirrored pairs, reparam.py:82-84, 189-196).  The pass replays the estimator of ``Scene.render_primal`` under the
    same seed (csrc/epsm_trace_reparam.h); a box reconstruction filter is refused as in common.py:379-388."""
    reparam = True

    def __init__(self, props: Optional[dict] = None):
        super().__init__(props)
        props = dict(props or {})
        self.reparam_max_depth = props.get("reparam_max_depth", self._depth())
        self.reparam_rays = int(props.get("reparam_rays", 16))
        self.reparam_kappa = float(props.get("reparam_kappa", 1e5))
        self.reparam_exp = float(props.get("reparam_exp", 3.0))
        self.reparam_antithetic = bool(props.get("reparam_antithetic", False))
        if not 1 <= self.reparam_rays <= 64:
            raise ValueError("prb_reparam: 1 <= reparam_rays <= 64")

    def to_string(self):
        return (f"PRBReparamIntegrator[max_depth = {self.max_depth}, rr_depth = {self.rr_depth}, reparam_max_depth = "
                f"{self.reparam_max_depth}, reparam_rays = {self.reparam_rays}]")

    __repr__ = to_string

    def render_backward(self, scene, params: ParamGrads, grad_in: torch.Tensor, sensor=0, seed: int = 0, spp: int = 0) -> None:
        cam, rot, n_rigid = _pose_attached(scene, params, "gradient buffer")
        self._color_backward(scene, params, grad_in, sensor, seed, spp)
        if not cam:
            if scene.has_attached_geometry():
                with _call_contribution(scene, params, n_rigid) as target:
                    self._geometry_backward(scene, target, grad_in, sensor, seed, spp)
            return
        # Moving the sensor by t moves every shape (and every emitter that is one) by -t as the sensor sees it; environment
        # emitters do not care.  So d loss / d sensor position = - sum over ALL vertices of d loss / d vertex position: the
        # same reparameterised pass with every mesh attached, summed (the primary rays' warp field carries the silhouettes).
        # Its rotation likewise: the sensor turning by omega about its position o is every shape turning by -omega about o, so
        # d loss / d omega = - the torque about o of all vertex rows, normals included; a `constant` environment does not care.
        # Both are ONE slot of epsm_rigid_reduce over every vertex with pivot o.
        every = _EveryMeshAttached(scene, normals=rot)

        def add_sensor_pass(full: ParamGrads) -> None:
            o = scene.sensors[min(sensor, len(scene.sensors) - 1)].to_world[:3, 3]
            twist = torch.zeros((1, 6), device=full.flat.device, dtype=torch.float32)
            ranges, pivots = scene.rigid_tables(extra=[(0, params.V, o)])
            scene.rigid_reduce(full.pos, full.nrm if rot else None, twist, ranges[n_rigid:], pivots[n_rigid:])
            params.cam_origin -= twist[0, :3]
            if rot:
                params.cam_rotation -= twist[0, 3:]
            for m, p, n in every.was:                          # the meshes the caller attached keep their own rows
                lo, hi = params.mesh_slices[m.name]
                if p:
                    params.pos[lo:hi] += full.pos[lo:hi]
                if n:
                    params.nrm[lo:hi] += full.nrm[lo:hi]
        with _call_contribution(scene, params, n_rigid, add=add_sensor_pass) as full:
            with every:
                self._geometry_backward(scene, full, grad_in, sensor, seed, spp)

    def render_forward(self, scene, params: ParamGrads, sensor=0, seed: int = 0, spp: int = 0) -> torch.Tensor:
        """The transpose of ``render_backward``: the colour part of ``PRBIntegrator.render_forward`` plus the reparameterised
        forward pass (``Scene.trace_reparam_forward``) for the tangents of the attached meshes' vertex positions / normals and,
        with ``Scene.attach_sensor``, of the sensor's position (``params.cam_origin``)."""
        cam, rot, n_rigid = _pose_attached(scene, params, "tangent")
        films = [self._color_forward(scene, params, sensor, seed, spp)]
        if not scene.has_attached_geometry() and not cam:
            return _develop_forward(scene, sensor, films)
        dev = scene.device
        twists = [params.rigid[:n_rigid].to(dev, torch.float32)] if n_rigid else []
        extra = []
        if cam:
            # the sensor moving by t and turning by omega about its position o = every shape moving by -t and turning by -omega
            # about o: one more slot over every vertex, the attached meshes' own rows on top, every mesh attached for the call
            w = params.cam_rotation.to(dev, torch.float32) if rot else torch.zeros(3, device=dev, dtype=torch.float32)
            twists.append(-torch.cat([params.cam_origin.to(dev, torch.float32), w])[None, :])
            extra.append((0, params.V, scene.sensors[min(sensor, len(scene.sensors) - 1)].to_world[:3, 3]))
        # the tangents of the rows the caller attached (the others are not read -- unless the sensor's pass attaches them: zero there)
        own = (lambda t: t.to(dev, torch.float32).clone()) if twists else (lambda t: t.to(dev, torch.float32).contiguous())
        tan_pos = torch.zeros((params.V, 3), device=dev, dtype=torch.float32) if cam else own(params.pos)
        tan_nrm = torch.zeros((params.V, 3), device=dev, dtype=torch.float32) if rot else own(params.nrm)
        for m in scene.meshes:
            lo, hi = params.mesh_slices[m.name]
            if cam and m.pos_attached:
                tan_pos[lo:hi] += params.pos[lo:hi].to(dev, torch.float32)
            if rot and m.nrm_attached:
                tan_nrm[lo:hi] += params.nrm[lo:hi].to(dev, torch.float32)
        if scene.has_recomputed_normals():
            # the transpose of _normals_chain_backward: the caller's own position tangents of those meshes move their normals (the
            # twists' motion of a normal is rigid_expand's dw x n, below)
            own_pos = params.pos.to(dev, torch.float32).contiguous()
            if tan_nrm.data_ptr() == params.nrm.data_ptr():
                tan_nrm = tan_nrm.clone()
            with _prof.phase("epsm.render_forward.normals_chain"):
                scene.normals_forward(own_pos, tan_nrm)
        if twists:
            ranges, pivots = scene.rigid_tables(extra=extra)
            scene.rigid_expand(torch.cat(twists).contiguous(), tan_pos, tan_nrm, ranges, pivots)
        with _EveryMeshAttached(scene, normals=rot) if cam else nullcontext():
            films.append(self._geometry_forward(scene, tan_pos, tan_nrm, sensor, seed, spp))
        return _develop_forward(scene, sensor, films)

    def _geometry_forward(self, scene, tan_pos: torch.Tensor, tan_nrm: torch.Tensor, sensor=0, seed: int = 0, spp: int = 0):
        """The transpose of ``_geometry_backward``: this rank's (primal film, tangent film) of the reparameterised pass."""
        si, s, spp, _, accum, tiles = _pass_frame(scene, sensor, spp, "reparam")
        _refuse_box_filter(s)
        d_accum = torch.zeros_like(accum)
        for lo, hi in tiles:
            with _prof.phase("epsm.prb_reparam.primal_pass"):
                tr = scene._trace(si, seed, spp, self._depth(), 0, lo, hi)
                scene.film_splat(accum, s, tr.film_pos, tr.radiance)
            radiance = tr.radiance.contiguous()
            with _prof.phase("epsm.prb_reparam.reparam_forward"):
                d_rad, d_film = scene.trace_reparam_forward(si, seed, spp, self._depth(), lo, hi, radiance, tan_pos, tan_nrm,
                                                            int(self.reparam_max_depth), self.reparam_rays, self.reparam_kappa,
                                                            self.reparam_exp, antithetic=self.reparam_antithetic)
            with _prof.phase("epsm.prb_reparam.film_tangent"):
                film_splat_tangent(d_accum, tr.film_pos, radiance, d_rad, d_film, s.rfilter)
        return accum, d_accum

    def _geometry_backward(self, scene, out: ParamGrads, grad_in: torch.Tensor, sensor=0, seed: int = 0, spp: int = 0) -> None:
        """Adds this rank's vertex gradients of the reparameterised pass to ``out.pos`` / ``out.nrm``: the caller's buffer of one
        call's contribution (``_call_contribution`` sums it over the ranks)."""
        si, s, spp, world, accum, tiles = _pass_frame(scene, sensor, spp, "reparam")
        _refuse_box_filter(s)
        # pass 1 (common.py:872-882): the primal estimate of every sample and the film they make
        kept = []
        for lo, hi in tiles:
            with _prof.phase("epsm.prb_reparam.primal_pass"):
                tr = scene._trace(si, seed, spp, self._depth(), 0, lo, hi)
                scene.film_splat(accum, s, tr.film_pos, tr.radiance)
            kept.append((tr.film_pos, tr.radiance.contiguous()))
        if world > 1:
            _dist.allreduce_param_grads(accum)
        # pass 2 (common.py:944-955): adjoint radiance, adjoint film position / determinant, the reparameterised replay
        g = grad_in.to(scene.device, torch.float32)[: s.height, : s.width, :3]
        for lo, hi in tiles:
            film_pos, radiance = kept.pop(0)
            with _prof.phase("epsm.prb_reparam.film_adjoint"):
                dL, adj = film_adjoint_reparam(film_pos, radiance, g, accum)
            with _prof.phase("epsm.prb_reparam.reparam_pass"):
                scene.trace_reparam(si, seed, spp, self._depth(), lo, hi, radiance, dL, adj, out.pos, out.nrm,
                                    int(self.reparam_max_depth), self.reparam_rays, self.reparam_kappa, self.reparam_exp,
                                    antithetic=self.reparam_antithetic)


# -- plugin registry (mi.register_integrator / mi.load_dict) -------------------
_REGISTRY: Dict[str, Callable[[dict], EPSMIntegrator]] = {}


def register_integrator(name: str, constructor: Callable[[dict], EPSMIntegrator]) -> None:
    _REGISTRY[name] = constructor


def load_dict(d: dict) -> EPSMIntegrator:
    d = dict(d)
    kind = d.pop("type")
    if kind not in _REGISTRY:
        raise RuntimeError(f"Plugin \"{kind}\" not found")   # PluginManager error text, plugin.cpp:24-38
    return _REGISTRY[kind](d)


register_integrator("manifold", lambda props: ManifoldIntegrator(props))                  # epsm.py:948
register_integrator("manifold_caustic", lambda props: ManifoldCausticIntegrator(props))   # epsm.py:1202
register_integrator("prb", lambda props: PRBIntegrator(props))
register_integrator("prb_reparam", lambda props: PRBReparamIntegrator(props))    # EPSM/optim.py:89-92 asks for this name
