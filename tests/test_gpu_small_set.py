"""The active-set step of small sets (nmpc_cl_fast.hip solve_set_one: a set of one bound, one fetch of
W[e_0, :] for the set solve and the combination, compiled into the three- and four-slot shapes)
against the oracle, on workloads whose sets sit on both sides of the limit, and against the general path
(NMPC_CLF_SMALLSET=0) bit for bit. The quad13 loop runs the new step (109 steps of one bound); the force solves and
the jerk loop hold the general path to its results on the shapes that keep it.

  * the fp64 general solve (sf_kernel + fin64_kernel) on the force shape's first-step QPs, N = 20 and N = 3:
    final set sizes 1..5 and above, counted from the oracle's solution (a bound active within 1e-7 (1 + |b|));
  * the closed loops of quad13 N = 20 B = 2048 (cl_lock_kernel, whose phase 2 runs the rare steps) and jerk
    N = 40 B = 1024 (cl_fast_kernel), seed 42, 3 warm-up steps + 20: the oracle's mode-1 loop stepped one step
    at a time, its path log and active flags giving the final set size of every active-set-path step.

Bars: x, u and states 1e-6 relative (the project's fp64 bar), status, qp_iter and failure counts exact.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL64 = 1e-6
SOLVE_CASES = [20, 3]
LOOP_CASES = [("quad13", 20, 2048, "cl_lock_kernel"), ("jerk", 40, 1024, "cl_fast_kernel")]
WARMUP, STEPS = 3, 20


def _rel(a, b):
    return np.abs(a - b).max(-1) / np.maximum(1.0, np.abs(b).max(-1))


def _set_sizes(spec, X, U):
    """active bounds per QP of the solutions X [B, N+1, nx], U [B, N, nu]: within 1e-7 (1 + |b|) of a bound"""
    from oracle import cref
    q = cref.stage_qp_data(spec)
    B, N = X.shape[0], spec.N

    def on(z, lb, ub):
        fl = np.isfinite(lb) & (np.abs(lb) < 1e20)
        fu = np.isfinite(ub) & (np.abs(ub) < 1e20)
        lo = fl & (np.abs(z - np.where(fl, lb, 0.0)) <= 1e-7 * (1.0 + np.abs(np.where(fl, lb, 0.0))))
        hi = fu & (np.abs(z - np.where(fu, ub, 0.0)) <= 1e-7 * (1.0 + np.abs(np.where(fu, ub, 0.0))))
        return (lo | hi).reshape(B, -1).sum(1)

    Z = np.concatenate([X[:, :N], U], axis=2)                     # [B, N, nx + nu]
    n = on(Z[:, 0], q["lb0"], q["ub0"])
    if N > 1:
        n = n + on(Z[:, 1:], q["lb"], q["ub"])
    return n + on(X[:, N], q["lbe"], q["ube"])


@pytest.fixture(scope="module")
def solve_refs():
    """per horizon: the force first-step QPs (seed 42, 256 instances) and the C restatement's fast solve"""
    from drone_attitude_control_amd.batched import first_step_qps
    from drone_attitude_control_amd.models import OCPS
    from drone_attitude_control_amd.sharding import rank_workload
    from oracle import cref, models
    out = {}
    for N in SOLVE_CASES:
        table, off, x, _ = rank_workload("force", N, 256, 1, 0, 42)
        x0, Y = first_step_qps("force", N, table, off, x)
        R = cref.RiccatiIpmRef.for_options(models.MODELS["force"](N), OCPS["force"](N).solver_options)
        X, U, st, it, _ = R.solve_fast(x0, Y, wsmax=cref.WSMAX["force"])
        out[N] = dict(x0=x0, Y=Y, X=X, U=U, st=st, it=it, sizes=_set_sizes(models.MODELS["force"](N), X, U))
    return out


def _gpu_solve(N, x0, Y):
    from drone_attitude_control_amd import AcadosOcpSolver
    from drone_attitude_control_amd.models import OCPS
    s = AcadosOcpSolver(OCPS["force"](N), batch=x0.shape[0])
    s.set_batch("x0", x0)
    s.set_batch("yref", Y)
    s.solve()
    assert s.launch_info()["solve_kernel"] == "sf_kernel"
    return s.get_batch("x"), s.get_batch("u"), s.get_batch_int("status"), s.get_batch_int("qp_iter")


@pytest.fixture(scope="module")
def loop_refs():
    """per closed-loop case: the oracle's mode-1 loop, single steps after the warm-up; sizes: the final set size
    of every step on the active-set path (path log 1)"""
    import bench
    from drone_attitude_control_amd.batched import workload
    from oracle import cref, models
    out = {}
    for model, N, B, _ in LOOP_CASES:
        table, off, x = workload(model, N, B, 42)
        tc, tr, pm, ps = bench.ipm_tolerances(model, N)
        ref = cref.ClosedLoopRef(models.MODELS[model](N), model, table, off, x, mode=1, seed=42,
                                 tol_comp=tc, tol_res=tr, polish_mu=pm, polish_steps=ps)
        ref.run(WARMUP)
        sizes, full = [], 0
        for _k in range(STEPS):
            _, _, _, path = ref.run(1, logs=True)
            sizes.append((ref.act != 0).sum(1)[path[:, 0] == 1])
            full += int((path[:, 0] == 2).sum())
        out[model] = dict(state=ref.state.copy(), acc=ref.acc.copy(), sizes=np.concatenate(sizes), full=full)
    return out


def _gpu_loop(model, N, B, kernel):
    from drone_attitude_control_amd.batched import ClosedLoop
    cl = ClosedLoop(model, B, N=N, seed=42)
    assert cl.solver.launch_info()["closed_loop_kernel"] == kernel
    cl.run(WARMUP)
    cl.run(STEPS)
    return cl.state(), cl.instance_stats()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("N", SOLVE_CASES)
def test_general_solve_across_the_limit(N, solve_refs):
    """fin64_kernel's rounds on sets below, at and above the small-set limit against the C restatement."""
    r = solve_refs[N]
    hist = np.bincount(np.minimum(r["sizes"], 6), minlength=7)
    print(f"force N={N}: final set sizes 0..5, >5: {hist.tolist()}; status != 0: {int((r['st'] != 0).sum())}")
    if N == 20:
        assert all(hist[k] >= 10 for k in (1, 2, 3, 4, 5)) and hist[6] >= 10, hist
    else:
        assert hist[4] >= 100 and hist[5] >= 10, hist
    X, U, st, it = _gpu_solve(N, r["x0"], r["Y"])
    B = X.shape[0]
    ex = _rel(X.reshape(B, -1), r["X"].reshape(B, -1))
    eu = _rel(U.reshape(B, -1), r["U"].reshape(B, -1))
    print(f"force N={N}: max rel err x {ex.max():.3e} u {eu.max():.3e}")
    assert ex.max() < TOL64 and eu.max() < TOL64, (ex.max(), eu.max())
    assert np.array_equal(st, r["st"])
    assert np.array_equal(it, r["it"])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("model,N,B,kernel", LOOP_CASES)
def test_closed_loops_with_small_sets(model, N, B, kernel, loop_refs):
    """The rare steps of the two lean kernels, almost all of them sets of one or two bounds, against the oracle's
    mode-1 loop."""
    r = loop_refs[model]
    hist = np.bincount(np.minimum(r["sizes"], 5), minlength=6)
    print(f"{model}: active-set-path steps by final set size 0..4, >4: {hist.tolist()}; full solves {r['full']}; "
          f"failures {int(r['acc'][:, 2].sum())}")
    if model == "quad13":
        assert hist[1] >= 50 and hist[2] >= 1, hist
    else:
        assert hist[1] >= 20 and hist[2] >= 3 and hist[3] + hist[4] >= 1, hist
    S, A = _gpu_loop(model, N, B, kernel)
    err = _rel(S, r["state"])
    print(f"{model}: max rel state err {err.max():.3e}")
    assert err.max() < TOL64, (err.max(), int(err.argmax()))
    assert np.array_equal(A[:, 2], r["acc"][:, 2])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", ["solve20", "solve3", "quad13", "jerk"])
def test_small_set_step_equals_general_path(case, solve_refs, monkeypatch):
    """NMPC_CLF_SMALLSET=0 (every set through solve_set_gj + w_combo_slots) and the default: the single-bound step
    reads the same words of W and repeats the elimination's pivot operation for operation, so everything is bit
    for bit equal."""
    out = []
    for arm in ("0", None):
        if arm is None:
            monkeypatch.delenv("NMPC_CLF_SMALLSET", raising=False)
        else:
            monkeypatch.setenv("NMPC_CLF_SMALLSET", arm)
        if case.startswith("solve"):
            r = solve_refs[int(case[5:])]
            out.append(_gpu_solve(int(case[5:]), r["x0"], r["Y"]))
        else:
            out.append(_gpu_loop(*[c for c in LOOP_CASES if c[0] == case][0]))
    for a, b in zip(*out):
        assert np.array_equal(a, b), (case, np.abs(a.astype(np.float64) - b.astype(np.float64)).max())
