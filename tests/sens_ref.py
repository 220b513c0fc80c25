"""Reference solution sensitivities from the dense oracle (test infrastructure only).

Computed live from oracle/qp.py, independently of the device's W / T_x route: the condensed QP
of one instance is solved (ipm + polish, KKT-certified), its on-bound rows A are read off the
solution, and the derivative of the solution with respect to x0 (and to each yref component)
is the solution of the equality-constrained KKT system

    [[H, A'], [A, 0]] [dU; dnu] = [-dg; db_A]

g, lo and hi are affine in x0 and g is affine in yref, so their derivatives are exact
differences of two CondensedQP constructions (x0 + e_i, yref + e_q). Then
dx_k = Phi_k + Gam_k dU for x0 and Gam_k dU for yref.

`case(name)` builds the inputs of the named test cases (the generator is part of the cases'
definition: default_rng(7), offsets, then per instance the draws in the listed order).
"""
import functools

import numpy as np

from oracle import models, qp
from oracle.trajectory import gen_circle_traj

ACTIVE_MULT = 1e-9     # a row is active when its multiplier exceeds this
ON_BOUND = 1e-7        # a row is on its bound when its slack is below this


def table_for(model, N):
    if model == "quad13":
        return models.quad13_reference(500, N)
    return gen_circle_traj(500, N, 6, 2)


def _draws(model, rng, scale):
    """The perturbation of one instance's start state, in the order the cases define."""
    if model == "force":
        p, v = scale
        return np.concatenate([rng.uniform(-p, p, 2), rng.uniform(-v, v, 2)])
    if model == "jerk":
        p, v, a = scale
        return np.concatenate([rng.uniform(-p, p, 2), rng.uniform(-v, v, 2), rng.uniform(-a, a, 2)])
    d = np.zeros(13)
    d[0:3] = rng.normal(0, 0.2, 3)
    d[3:6] = rng.normal(0, 0.5, 3)
    d[7:10] = rng.normal(0, 0.1, 3)
    d[10:13] = rng.normal(0, 0.5, 3)
    return d


# name: (model, N, B, draw scales)
CASES = {
    "force_N20": ("force", 20, 48, (0.2, 0.6)),
    "jerk_N40": ("jerk", 40, 24, (0.1, 0.3, 1.0)),
    "quad13_N20": ("quad13", 20, 32, None),
    "force_N3": ("force", 3, 5, (0.1, 0.3)),
    "force_N6": ("force", 6, 16, (0.1, 0.3)),
}


def window(spec, table, off):
    """yref [N, ny] (rows off .. off+N-1) and yref_e [ny_e] (row off+N) of one instance."""
    N = spec.N
    return table[off:off + N, :spec.ny].copy(), table[off + N, :spec.nx].copy()


def inputs(model, N, B, scale):
    """(spec, offsets [B], x0 [B, nx], yref [B, N, ny], yref_e [B, nx])."""
    spec = models.MODELS[model](N)
    table = table_for(model, N)
    rng = np.random.default_rng(7)
    off = rng.integers(0, 500, B)
    x0 = np.zeros((B, spec.nx))
    for b in range(B):
        x0[b] = table[off[b], :spec.nx] + _draws(model, rng, scale)
    Y = np.array([window(spec, table, o)[0] for o in off])
    Ye = np.array([window(spec, table, o)[1] for o in off])
    return spec, off, x0, Y, Ye


def stacked_yref(Y, Ye):
    """The engine's stage-stacked layout [B, N*ny + ny_e]."""
    return np.concatenate([Y.reshape(Y.shape[0], -1), Ye], axis=1)


def sens_ref(spec, x0, yref, yref_e, with_yref=False):
    """Oracle solution and its Jacobians for one instance. Keys:
    certified; U [N, nu], X [N+1, nx]; n_on (on-bound rows), weak (on bound, multiplier <= 1e-9),
    cond (A H^-1 A' over the on-bound rows; 1 for none), rank_deficient, min_mult, min_slack;
    Jx [N+1, nx, nx] = dx_k/dx0, Ju [N, nu, nx] = du_k/dx0; with_yref: Yx [N+1, nx, nY],
    Yu [N, nu, nY] with nY = N*ny + ny_e in the stage-stacked order."""
    N, nx, nu = spec.N, spec.nx, spec.nu
    x0 = np.asarray(x0, float)
    Q = qp.CondensedQP(spec, x0, yref, yref_e)
    U, ll, lu, tl, tu, _ = Q.ipm()
    Up, ml, mu_, ok = Q.polish(U, ll, lu, tl, tu)
    kkt = Q.kkt_residuals(Up, ml, mu_)
    scale = 1.0 + np.abs(Q.g).max() + np.abs(Q.H).max()
    certified = bool(ok and kkt["stationarity"] < 1e-9 * scale and kkt["primal"] < 1e-9 and kkt["dual"] < 1e-9)
    out = {"certified": certified, "U": Up.reshape(N, nu), "X": Q.states(Up)}
    if not certified:
        return out
    CU = Q.C @ Up
    slack = np.minimum(CU - Q.lo, Q.hi - CU)
    on = slack < ON_BOUND
    mult = ml + mu_
    active = mult > ACTIVE_MULT
    A = Q.C[on]
    n, na = Q.H.shape[0], A.shape[0]
    out["n_on"] = int(na)
    out["weak"] = int((on & ~active).sum())
    out["min_mult"] = float(mult[on].min()) if na else np.inf
    out["min_slack"] = float(slack[~on].min()) if (~on).any() else np.inf
    if na:
        S = A @ np.linalg.solve(Q.H, A.T)
        out["cond"] = float(np.linalg.cond(S))
        out["rank_deficient"] = bool(np.linalg.matrix_rank(A) < na)
    else:
        out["cond"], out["rank_deficient"] = 1.0, False
    K = np.zeros((n + na, n + na))
    K[:n, :n] = Q.H
    K[:n, n:] = A.T
    K[n:, :n] = A

    def solve(dg, db):
        rhs = np.concatenate([-dg, db], axis=0)
        if out["rank_deficient"]:
            return np.linalg.lstsq(K, rhs, rcond=None)[0][:n]
        return np.linalg.solve(K, rhs)[:n]

    # x0: exact differences of two constructions (g, lo, hi affine in x0)
    dg = np.zeros((n, nx))
    db = np.zeros((na, nx))
    for i in range(nx):
        e = np.zeros(nx)
        e[i] = 1.0
        Qi = qp.CondensedQP(spec, x0 + e, yref, yref_e)
        dg[:, i] = Qi.g - Q.g
        db[:, i] = (Qi.lo - Q.lo)[on]
    dU = solve(dg, db)
    out["Jx"] = np.array([Q.Phi[k] + Q.Gam[k] @ dU for k in range(N + 1)])
    out["Ju"] = dU.reshape(N, nu, nx)
    if with_yref:
        ny = spec.ny
        nY = N * ny + spec.nx
        dgy = np.zeros((n, nY))
        for q in range(nY):
            Y2, Ye2 = np.array(yref, float), np.array(yref_e, float)
            if q < N * ny:
                Y2[q // ny, q % ny] += 1.0
            else:
                Ye2[q - N * ny] += 1.0
            dgy[:, q] = qp.CondensedQP(spec, x0, Y2, Ye2).g - Q.g
        dUy = solve(dgy, np.zeros((na, nY)))
        out["Yx"] = np.array([Q.Gam[k] @ dUy for k in range(N + 1)])
        out["Yu"] = dUy.reshape(N, nu, nY)
    return out


@functools.lru_cache(maxsize=None)
def case(name, with_yref=False):
    """Inputs and per-instance references of a named case, computed once per process:
    {spec, off, x0, Y, Ye, yref (stacked), ref: [sens_ref dict per instance]}. Read-only."""
    model, N, B, scale = CASES[name]
    spec, off, x0, Y, Ye = inputs(model, N, B, scale)
    ref = [sens_ref(spec, x0[b], Y[b], Ye[b], with_yref) for b in range(B)]
    return {"model": model, "N": N, "B": B, "spec": spec, "off": off, "x0": x0, "Y": Y, "Ye": Ye,
            "yref": stacked_yref(Y, Ye), "ref": ref}


def size_classes(ref):
    """Counts of the certified instances' on-bound set sizes: (empty, 1-16, 17-32, 33-64, > 64)."""
    n = np.array([r["n_on"] for r in ref if r["certified"]])
    return (int((n == 0).sum()), int(((n >= 1) & (n <= 16)).sum()), int(((n >= 17) & (n <= 32)).sum()),
            int(((n >= 33) & (n <= 64)).sum()), int((n > 64).sum()))


def rel_err(J, Jref):
    """The tests' metric: max|J - J_ref| / max(1, max|J_ref|)."""
    return float(np.abs(J - Jref).max() / max(1.0, np.abs(Jref).max()))
