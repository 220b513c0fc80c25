"""GPU tests of the solution sensitivities (nmpc_sens_forward / nmpc_sens_adjoint, nmpc_sens.hip).

Reference: tests/sens_ref.py, the KKT-system derivatives on the dense oracle's on-bound rows, independent of
the device's W / T_x route. Error metric per instance: max|J - J_ref| / max(1, max|J_ref|); bar: the project's
fp64 parity bar 1e-6 (tests/test_gpu_solver.py TOL64). Every test first asserts, from the oracle alone, what it
relies on: no weakly active bound, cond(A H^-1 A') < 1e8, the set-size classes populated. Every certified
instance is compared; an instance the oracle does not certify is compared only through its status: a failed
engine solve must give NMPC_SENS_NO_SOLUTION and NaN outputs.
Measured on an MI355X: forward 1.2e-12 (force N=20), 2.0e-14 (jerk), 5.1e-15 (quad13), 3.6e-14 (force N=3);
adjoint 6.0e-13; adjoint against the forward assembly 3.7e-13; the closed loop's last step 3.4e-14.
"""
import ctypes
import functools

import numpy as np
import pytest

import sens_ref as sr
from drone_attitude_control_amd import AcadosOcpSolver, _lib
from drone_attitude_control_amd.batched import ClosedLoop
from drone_attitude_control_amd.models import OCPS
from oracle import models

pytestmark = pytest.mark.gpu

TOL = 1e-6
# case: (instances the oracle certifies, set-size classes (empty, 1-16, 17-32, 33-64) that must be populated)
EXPECT = {
    "force_N20": (46, (1, 2, 3)),
    "jerk_N40": (24, (0, 1, 2)),
    "quad13_N20": (21, (0, 1, 2)),
    "force_N3": (5, (1,)),
    "force_N6": (16, (1,)),
}


def oracle_conditions(name, with_yref=False):
    """The case with its references, after asserting the oracle-side conditions the comparison relies on."""
    c = sr.case(name, with_yref)
    cert = [r for r in c["ref"] if r["certified"]]
    ncert, classes = EXPECT[name]
    assert len(cert) == ncert, (name, len(cert))
    assert all(r["weak"] == 0 for r in cert)
    assert max(r["cond"] for r in cert) < 1e8
    sizes = sr.size_classes(c["ref"])
    assert all(sizes[k] >= 1 for k in classes), (name, sizes)
    assert sizes[4] == 0
    return c


@functools.lru_cache(maxsize=None)
def solved(name):
    """A solver holding the case's solution (shared, read-only: the sensitivity calls never change it)."""
    c = sr.case(name)
    s = AcadosOcpSolver(OCPS[c["model"]](c["N"]), batch=c["B"])
    s.set_batch("x0", c["x0"])
    s.set_batch("yref", c["yref"])
    s.solve()
    return s


def fwd_raw(s, stage, want_u=True):
    """nmpc_sens_forward through ctypes: (return code, sens_x, sens_u)."""
    sx = np.zeros((s.batch, s.nx, s.nx))
    su = np.zeros((s.batch, s.nu, s.nx)) if want_u else None
    rc = s.lib.nmpc_sens_forward(s._h, stage, _lib.dptr(sx), sx.size, _lib.dptr(su), su.size if want_u else 0)
    return rc, sx, su


def uncertified_ok(st_solve, st_sens, outs):
    """An instance the oracle does not certify: a failed engine solve must be flagged and NaN; else not compared."""
    if st_solve != 0:
        assert st_sens == _lib.NMPC_SENS_NO_SOLUTION
        for o in outs:
            assert o is None or np.isnan(o).all()


@pytest.mark.parametrize("name", ["force_N20", "jerk_N40", "quad13_N20", "force_N3"])
def test_forward_parity(name):
    """sens_batch(k) for k in {0, 1, N-1, N} after solve() against sens_ref, status 0 on every compared instance;
    sens_u is refused at k = N."""
    c = oracle_conditions(name)
    s, N = solved(name), c["N"]
    st_solve = s.get_batch_int("status")
    worst = 0.0
    for k in sorted({0, 1, N - 1, N}):
        sx, su, st = s.sens_batch(k)
        assert (su is None) == (k == N)
        for b, r in enumerate(c["ref"]):
            if not r["certified"]:
                uncertified_ok(st_solve[b], st[b], (sx[b], su[b] if su is not None else None))
                continue
            assert st_solve[b] == 0 and st[b] == _lib.NMPC_SENS_OK, (k, b, st_solve[b], st[b])
            errs = [sr.rel_err(sx[b], r["Jx"][k])] + ([sr.rel_err(su[b], r["Ju"][k])] if k < N else [])
            worst = max(worst, *errs)
            assert max(errs) < TOL, (k, b, r["n_on"], errs)
    print(f"{name}: forward max error {worst:.2e}")
    rc, _, _ = fwd_raw(s, N, want_u=True)
    assert rc == _lib.NMPC_EINVAL


def test_facade_eval_solution_sensitivity():
    """eval_solution_sensitivity(0, "initial_state", instance=i) is row i of the batch call; a stage list returns
    lists; any other with_respect_to raises NotImplementedError."""
    c = oracle_conditions("force_N3")
    s, N = solved("force_N3"), c["N"]
    sx, su, _ = s.sens_batch(0)
    for i in range(c["B"]):
        out = s.eval_solution_sensitivity(0, "initial_state", instance=i)
        assert np.array_equal(out["sens_x"], sx[i]) and np.array_equal(out["sens_u"], su[i])
        assert sr.rel_err(out["sens_u"], c["ref"][i]["Ju"][0]) < TOL
    out = s.eval_solution_sensitivity([0, 1, N], "initial_state", instance=2)
    assert isinstance(out["sens_x"], list) and isinstance(out["sens_u"], list) and len(out["sens_x"]) == 3
    for j, k in enumerate((0, 1, N)):
        assert sr.rel_err(out["sens_x"][j], c["ref"][2]["Jx"][k]) < TOL
    assert out["sens_u"][2].shape == (0, s.nx)     # no u at the terminal stage
    only_x = s.eval_solution_sensitivity(1, "initial_state", return_sens_u=False)
    assert set(only_x) == {"sens_x"}
    with pytest.raises(NotImplementedError):
        s.eval_solution_sensitivity(0, "params_global")


def test_adjoint_parity():
    """force N=6 B=16: grad_x0 and grad_yref against J_ref' g with the full oracle Jacobians, for a cotangent on all
    of (x, u), then one that is nonzero only on u_0."""
    c = oracle_conditions("force_N6", True)
    s, B, N = solved("force_N6"), c["B"], c["N"]
    rng = np.random.default_rng(11)
    gx = rng.normal(size=(B, N + 1, s.nx))
    gu = rng.normal(size=(B, N, s.nu))
    gu0 = np.zeros_like(gu)
    gu0[:, 0] = gu[:, 0]
    worst = 0.0
    for cx, cu in ((gx, gu), (None, gu0)):
        g0, gy, st = s.adjoint_batch(cx, cu)
        for b, r in enumerate(c["ref"]):
            assert r["certified"] and st[b] == _lib.NMPC_SENS_OK
            ex = np.einsum("kri,kr->i", r["Ju"], cu[b])
            ey = np.einsum("krq,kr->q", r["Yu"], cu[b])
            if cx is not None:
                ex = ex + np.einsum("kri,kr->i", r["Jx"], cx[b])
                ey = ey + np.einsum("krq,kr->q", r["Yx"], cx[b])
            errs = (sr.rel_err(g0[b], ex), sr.rel_err(gy[b], ey))
            worst = max(worst, *errs)
            assert max(errs) < TOL, (b, errs)
    print(f"force_N6: adjoint max error {worst:.2e}")


def test_adjoint_equals_forward_assembly():
    """force N=20 B=48: grad_x0 equals sum_k J_k' g_k assembled from the forward calls over all stages."""
    c = oracle_conditions("force_N20")
    s, B, N = solved("force_N20"), c["B"], c["N"]
    rng = np.random.default_rng(11)
    gx = rng.normal(size=(B, N + 1, s.nx))
    gu = rng.normal(size=(B, N, s.nu))
    want = np.zeros((B, s.nx))
    for k in range(N + 1):
        sx, su, stf = s.sens_batch(k)
        want += np.einsum("bri,br->bi", sx, gx[:, k])
        if k < N:
            want += np.einsum("bri,br->bi", su, gu[:, k])
    g0, _, st = s.adjoint_batch(gx, gu)
    st_solve = s.get_batch_int("status")
    assert np.array_equal(st, stf)
    worst = 0.0
    for b, r in enumerate(c["ref"]):
        if not r["certified"]:
            uncertified_ok(st_solve[b], st[b], (g0[b],))
            continue
        assert st[b] == _lib.NMPC_SENS_OK
        e = sr.rel_err(g0[b], want[b])
        worst = max(worst, e)
        assert e < TOL, (b, e)
    print(f"force_N20: adjoint vs forward assembly max error {worst:.2e}")


def _hip():
    _lib.load()
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip


def _dev(hip, s, field, shape, dtype=np.float64):
    out = np.zeros(shape, dtype=dtype)
    assert hip.hipMemcpy(out.ctypes.data, s.device_ptr(field), out.nbytes, 2) == 0
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def test_stream_order_and_determinism():
    """solve_async(); sens_forward_async(0); synchronize() returns the bits of the synchronous sequence, a second
    call returns the same bits, and x / u / status / qp_iter are bitwise unchanged by the sensitivity calls."""
    c = sr.case("force_N20")
    B, N = c["B"], c["N"]
    s = AcadosOcpSolver(OCPS["force"](N), batch=B)
    s.set_batch("x0", c["x0"])
    s.set_batch("yref", c["yref"])
    s.solve()
    sx, su, st = s.sens_batch(0)
    sx2, su2, st2 = s.sens_batch(0)
    assert np.array_equal(_bits(sx), _bits(sx2)) and np.array_equal(_bits(su), _bits(su2)) and np.array_equal(st, st2)
    g0, gy, _ = s.adjoint_batch(None, np.ones((B, N, s.nu)))
    g0b, gyb, _ = s.adjoint_batch(None, np.ones((B, N, s.nu)))
    assert np.array_equal(_bits(g0), _bits(g0b)) and np.array_equal(_bits(gy), _bits(gyb))
    hip = _hip()
    shapes = {"x": ((B, N + 1, s.nx), np.float64), "u": ((B, N, s.nu), np.float64),
              "status": ((B,), np.int32), "qp_iter": ((B,), np.int32)}
    s.solve_async()
    s.synchronize()
    before = {f: _dev(hip, s, f, *sh) for f, sh in shapes.items()}
    s.solve_async()
    s.sens_forward_async(0)
    s.synchronize()
    ax, au = _dev(hip, s, "sens_x", sx.shape), _dev(hip, s, "sens_u", su.shape)
    ast = _dev(hip, s, "sens_status", (B,), np.int32)
    assert np.array_equal(_bits(ax), _bits(sx)) and np.array_equal(_bits(au), _bits(su)) and np.array_equal(ast, st)
    s.sens_adjoint_async()
    s.synchronize()
    after = {f: _dev(hip, s, f, *sh) for f, sh in shapes.items()}
    for f in shapes:
        assert np.array_equal(_bits(before[f]), _bits(after[f])), f


def test_closed_loop_last_step():
    """ClosedLoop("force", 16, N=20) on the default workload: with set_outputs(True), after run(3), the stage-0
    sensitivities match sens_ref at each instance's downloaded x_0 and the table window at rows offset + 2 ...;
    with outputs off the call returns NMPC_ESTATE."""
    N, B = 20, 16
    spec = models.force_model(N)
    cl = ClosedLoop("force", B, N=N)
    rc, _, _ = fwd_raw(cl.solver, 0)
    assert rc == _lib.NMPC_ESTATE
    cl.run(3)
    rc, _, _ = fwd_raw(cl.solver, 0)
    assert rc == _lib.NMPC_ESTATE
    cl = ClosedLoop("force", B, N=N)
    cl.set_outputs(True)
    cl.run(3)
    s = cl.solver
    sx, su, st = s.sens_batch(0)
    X, st_solve = s.get_batch("x"), s.get_batch_int("status")
    table, off = cl._keep["table"], cl._keep["offsets"]
    compared, worst = 0, 0.0
    for b in range(B):
        t = (int(off[b]) + 2) % cl.period
        Y, Ye = sr.window(spec, table, t)
        r = sr.sens_ref(spec, X[b, 0], Y, Ye)
        if not r["certified"]:
            uncertified_ok(st_solve[b], st[b], (sx[b], su[b]))
            continue
        assert r["weak"] == 0 and r["cond"] < 1e8
        assert st_solve[b] == 0 and st[b] == _lib.NMPC_SENS_OK
        errs = (sr.rel_err(sx[b], r["Jx"][0]), sr.rel_err(su[b], r["Ju"][0]))
        worst = max(worst, *errs)
        assert max(errs) < TOL, (b, errs)
        compared += 1
    assert compared == B, compared      # the default workload starts near the reference: every step certifies
    print(f"closed loop: stage-0 max error {worst:.2e}")


def test_refusals():
    """Before any solve NMPC_ESTATE; a stage outside [0, N] and wrong counts NMPC_EINVAL; an fp32 handle
    NMPC_EUNSUPPORTED, and it still solves afterwards."""
    c = sr.case("force_N3")
    B, N = c["B"], c["N"]
    s = AcadosOcpSolver(OCPS["force"](N), batch=B)
    lib, h = s.lib, s._h
    assert fwd_raw(s, 0)[0] == _lib.NMPC_ESTATE
    assert lib.nmpc_sens_forward_async(h, 0) == _lib.NMPC_ESTATE
    assert lib.nmpc_sens_adjoint_async(h) == _lib.NMPC_ESTATE
    g0 = np.zeros((B, s.nx))
    assert lib.nmpc_sens_adjoint(h, None, 0, None, 0, _lib.dptr(g0), g0.size, None, 0) == _lib.NMPC_ESTATE
    s.set_batch("x0", c["x0"])
    s.set_batch("yref", c["yref"])
    assert s.solve() == 0
    for stage in (-1, N + 1):
        assert fwd_raw(s, stage)[0] == _lib.NMPC_EINVAL
        assert lib.nmpc_sens_forward_async(h, stage) == _lib.NMPC_EINVAL
    sx = np.zeros((B, s.nx, s.nx))
    assert lib.nmpc_sens_forward(h, 0, _lib.dptr(sx), sx.size - 1, None, 0) == _lib.NMPC_EINVAL
    assert lib.nmpc_sens_forward(h, 0, None, 0, _lib.dptr(sx), sx.size) == _lib.NMPC_EINVAL
    assert lib.nmpc_sens_forward(h, 0, None, 3, None, 0) == _lib.NMPC_EINVAL
    assert lib.nmpc_sens_adjoint(h, _lib.dptr(sx), sx.size - 1, None, 0, _lib.dptr(g0), g0.size, None, 0) == _lib.NMPC_EINVAL
    assert lib.nmpc_sens_adjoint(h, None, 0, None, 0, _lib.dptr(g0), g0.size + 1, None, 0) == _lib.NMPC_EINVAL
    assert lib.nmpc_sens_forward(h, 0, _lib.dptr(sx), sx.size, None, 0) == 0      # either output may be NULL
    assert sr.rel_err(sx[0], c["ref"][0]["Jx"][0]) < TOL
    assert lib.nmpc_sens_adjoint(h, None, 0, None, 0, _lib.dptr(g0), g0.size, None, 0) == 0
    assert np.array_equal(g0, np.zeros_like(g0))                                   # NULL cotangents are zero
    bad = np.zeros(B + 1, dtype=np.int32)
    assert lib.nmpc_get_batch_int(h, b"sens_status", bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), bad.size) \
        == _lib.NMPC_EINVAL
    from drone_attitude_control_amd.batched import first_step_qps, workload
    x32, y32 = first_step_qps("force", 20, *workload("force", 20, 8))
    s32 = AcadosOcpSolver(OCPS["force"](20), batch=8, precision="fp32")
    s32.set_batch("x0", x32)
    s32.set_batch("yref", y32)
    assert s32.solve() == 0
    assert fwd_raw(s32, 0)[0] == _lib.NMPC_EUNSUPPORTED
    assert b"fp64" in s32.lib.nmpc_last_error(s32._h)
    assert s32.lib.nmpc_sens_adjoint_async(s32._h) == _lib.NMPC_EUNSUPPORTED
    with pytest.raises(Exception):
        s32.device_ptr("sens_x")
    assert s32.solve() == 0
    assert np.abs(s32.get_batch("x")[:, 0] - x32).max() < 1e-5
