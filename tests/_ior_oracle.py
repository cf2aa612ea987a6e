"""Float64 torch restatement of the linear systems of the reference's two calc_grad flavours (epsm.py:745-946 `manifold`,
952-1200 `manifold_caustic`) with ONE more parameter column per vertex: eta_k, the relative index of refraction the half-vector
constraint C_k = [normalize(T(n_k)(wi + eta_k wo))]_xy - m_k is evaluated with.  Test infrastructure: the yardstick for the eta
column of epsm_cp_core.h (tests/test_ior_restatement.py), valid only as far as its normal and hf columns reproduce the reference's
own float64 results on the goldens -- which that file checks first.

What is restated, per depth id and per version of the last constraint (towards the emitter sample / towards vertex id + 1):
  rows     the Jacobian of constraint k w.r.t. the barycentrics of vertices k - 1, k, k + 1 (through the positions and, for vertex k,
           through its interpolated normal as well) and w.r.t. the parameters n_k (the interpolated normal, held apart), m_k, eta_k --
           by autograd, one backward sweep per component;
  system   cur = the rows of vertices 1..id against the barycentrics of vertices 1..id; a parameter's gradient is
           -dlduv[:2 id] cur^-1 (d rows / d parameter), summed over depths and versions;
  masks    the reference's: every vertex so far a mesh hit, fewer than two diffuse ones, the end vertex active (and its emitter sample
           usable / its BSDF diffuse), no diffuse vertex so far (`manifold`); identity systems where the term is void; nan_to_num per
           term; components beyond +-clip zeroed on the SUM of a vertex's terms;
  caustic  dlduv counts on paths whose first vertex is diffuse; at every depth the two rows of the last diffuse vertex are REPLACED by
           the pseudo-constraint wo2 = [T(n_id) normalize(x_id+1 - x_id)]_xy of the current vertex, parameters included (eta and m have
           no part in it); the emitter-sample version contributes nothing to n, m or eta there and is left out.
Only the n, m and eta columns are formed: positions, emitter samples and end points are the oracle's business (oracle/)."""
import torch

DIFFUSE = 0x2 | 0x4


def _unit(v):
    return v / torch.linalg.norm(v, dim=-1, keepdim=True)


def _bary(tri, uv):
    return tri[0] * uv[:, 0:1] + tri[1] * uv[:, 1:2] + tri[2] * (1.0 - uv[:, 0:1] - uv[:, 1:2])


def _to_local(n, w):
    """[t . w, bt . w, nn . w] in the frame t = (0, -nn_z, nn_y) / |.|, bt = nn x t of nn = n / |n|"""
    nn = _unit(n)
    t = _unit(torch.stack([torch.zeros_like(nn[:, 0]), -nn[:, 2], nn[:, 1]], dim=-1))
    bt = torch.linalg.cross(nn, t, dim=-1)
    return torch.stack([(t * w).sum(-1), (bt * w).sum(-1), (nn * w).sum(-1)], dim=-1)


def _rows(rec, cam, k, towards_light, want_pseudo):
    """Constraint k (1-based) of every path: -> dict of Jacobian rows, each (N, 2, width); None where there is no such vertex."""
    N = cam.shape[0]
    leaf = lambda t: t.detach().clone().requires_grad_(True)
    uv = {j: leaf(torch.stack(rec[j]["uv"], dim=-1)) for j in (k - 1, k, k + 1) if 1 <= j < len(rec) and not (towards_light and j == k + 1)}
    eta, m = leaf(rec[k]["eta"]), leaf(rec[k]["hf"])
    x = _bary(rec[k]["points"], uv[k])
    xp = cam if k == 1 else _bary(rec[k - 1]["points"], uv[k - 1])
    xn = rec[k]["light"] if towards_light else _bary(rec[k + 1]["points"], uv[k + 1])
    n = _bary(rec[k]["normals"], uv[k])                       # a parameter of its own AND a function of the barycentrics
    wi, wo = _unit(xp - x), _unit(xn - x)
    wo_l = _to_local(n, wo)
    c = _unit(_to_local(n, wi) + wo_l * eta[:, None])
    if not towards_light:
        c = c - m
    names = [("prev", uv.get(k - 1)), ("own", uv[k]), ("next", uv.get(k + 1)), ("n", n), ("m", m), ("eta", eta)]
    names = [(a, t) for a, t in names if t is not None]

    def jac(f):
        out = {a: [] for a, _ in names}
        for i in range(2):
            g = torch.autograd.grad(f[:, i].sum(), [t for _, t in names], retain_graph=True, allow_unused=True)
            for (a, t), gi in zip(names, g):
                out[a].append(torch.zeros_like(t) if gi is None else gi)
        return {a: torch.stack([r.reshape(N, -1) for r in v], dim=1) for a, v in out.items()}
    res = {"c": jac(c)}
    if want_pseudo:
        res["w"] = jac(wo_l)
    return res


def _solve_term(cur, dlduv, cols, void):
    """-dlduv cur^-1 cols per path; `void`: the system is replaced by the identity (the term is dropped afterwards)"""
    n = cur.shape[1]
    cur = torch.where(void[:, None, None], torch.eye(n, dtype=cur.dtype).expand_as(cur), cur)
    inv, info = torch.linalg.inv_ex(cur)
    inv = torch.where((info != 0)[:, None, None], torch.full_like(inv, float("nan")), inv)
    return -torch.bmm(dlduv[:, None, :n], torch.bmm(inv, cols))[:, 0]


def calc_grad_with_eta(variant, path_info, dlduv, dldp=None, clip=0.1):
    """-> (gn, gm, geta): lists over the vertices 1..K of (N,3), (N,3), (N,) float64 -- d loss / d n_k, d m_k, d eta_k"""
    rec = [None] + [{"uv": [u.double() for u in r["uv"]], "points": [p.double() for p in r["points"][:3]],
                     "normals": [p.double() for p in r["normals"]], "eta": r["eta"].double(), "hf": r["hf"].double(),
                     "light": r["light"].double(), "active": r["active"] != 0, "active_em": r["active_em"] != 0,
                     "ismesh": r["ismesh"] > 0, "diffuse": (r["bsdf"].long() & DIFFUSE) != 0} for r in path_info[1:]]
    cam = path_info[0]["cam"].double()
    N, K = cam.shape[0], len(rec) - 1
    caustic = variant == "manifold_caustic"
    R, C = 2 * (K + 1), 2 * (K + 1) + 4
    d = torch.zeros((N, R), dtype=torch.float64)
    flat = dlduv.double().reshape(N, -1)
    d[:, :min(R, flat.shape[1])] = flat[:, :R]
    if caustic:
        d = torch.where(rec[1]["diffuse"][:, None], d, torch.zeros_like(d))
    A = torch.zeros((N, R, C), dtype=torch.float64)                      # rows: constraints; columns 2 j, 2 j + 1: vertex j
    P = {(kind, k): torch.zeros((N, R, w), dtype=torch.float64) for k in range(1, K + 1) for kind, w in (("n", 3), ("m", 3), ("eta", 1))}
    total = {key: torch.zeros((N, w.shape[2]), dtype=torch.float64) for key, w in P.items()}
    valid = torch.ones(N, dtype=torch.bool)
    ndiffuse = torch.zeros(N, dtype=torch.int64)
    last_diffuse = torch.zeros(N, dtype=torch.int64)

    def put_rows(k, J, with_m):
        for i in range(2):
            r = 2 * k - 2 + i
            if "prev" in J:
                A[:, r, 2 * k - 2:2 * k] = J["prev"][:, i]
            A[:, r, 2 * k:2 * k + 2] = J["own"][:, i]
            if "next" in J:
                A[:, r, 2 * k + 2:2 * k + 4] = J["next"][:, i]
            P[("n", k)][:, r] = J["n"][:, i]
            P[("eta", k)][:, r] = J["eta"][:, i]
            P[("m", k)][:, r] = J["m"][:, i] if with_m else 0.0

    def add_terms(k, void, live):
        cur = A[:, :2 * k, 2:2 * k + 2]
        for key, cols in P.items():
            t = torch.nan_to_num(_solve_term(cur, d, cols[:, :2 * k], void))
            total[key] += torch.where(live[:, None], t, torch.zeros_like(t))

    for k in range(1, K + 1):
        v = rec[k]
        valid = valid & v["ismesh"]
        ndiffuse = ndiffuse + v["diffuse"].long()
        valid = valid & (ndiffuse < 2)
        last_diffuse = torch.where(v["diffuse"], torch.full_like(last_diffuse, k), last_diffuse)
        if not caustic:
            put_rows(k, _rows(rec, cam, k, True, False)["c"], False)
            ok = valid & v["active"] & v["active_em"]
            add_terms(k, ~ok, ok & (ndiffuse == 0))
        if k == K:
            break
        J = _rows(rec, cam, k, False, caustic)
        put_rows(k, J["c"], True)
        nxt = rec[k + 1]
        if caustic:
            W = J["w"]
            for j in range(1, k + 1):
                sel = last_diffuse == j
                for i in range(2):
                    r = 2 * j - 2 + i
                    A[sel, r] = 0.0
                    A[sel, r, 2 * k:2 * k + 2] = W["own"][sel, i]
                    A[sel, r, 2 * k + 2:2 * k + 4] = W["next"][sel, i]
                    for key, cols in P.items():
                        cols[sel, r] = W["n"][sel, i] if key == ("n", k) else 0.0
        ok = valid & nxt["active"]
        live = ok & nxt["diffuse"]
        add_terms(k, ~ok, live if caustic else live & (ndiffuse == 0))

    def clamp(t):
        return t if not (clip and clip > 0) else torch.where((t > clip) | (t < -clip), torch.zeros_like(t), t)
    gn = [clamp(total[("n", k)]) for k in range(1, K + 1)]
    gm = [clamp(total[("m", k)]) for k in range(1, K + 1)]
    geta = [clamp(total[("eta", k)])[:, 0] for k in range(1, K + 1)]
    return gn, gm, geta
