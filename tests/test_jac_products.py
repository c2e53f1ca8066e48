"""twr_jac_mul / twr_jac_tmul on the device: y = J v and z = J^T w per problem against float64 scipy, on the oracle's Jacobian
values and on the device's own, the adjoint identity, central differences of the values path, bit-reproducibility across
calls and batch compositions, containment of NaN / Inf, and stream order under hipGraph capture.  The handles here are
JacBatch(..., make=("ops",)) of tests/jac_device.py: products alone, no solver handle."""
import numpy as np
import pytest

import towr_amd as ta

from .common import baseline_cases, random_case
from .jac_device import JacBatch, assert_replay_equals_eager, capture, dev, ragged, ragged_x, torch_ctx
from .jac_ref import csr

pytestmark = pytest.mark.gpu


def _check_problem(S, jv, v, w, y, z, what):
    A = csr(S, jv)
    absA = abs(A)
    ty, tz = absA @ np.abs(v), absA.T @ np.abs(w)
    assert np.all(np.abs(y - A @ v) <= 1e-12 * ty), (what, "J v", np.abs(y - A @ v).max())
    assert np.all(np.abs(z - A.T @ w) <= 1e-12 * tz), (what, "J^T w", np.abs(z - A.T @ w).max())
    lhs, rhs = w @ y, z @ v
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(w) @ ty), (what, "adjoint", lhs, rhs)


def _check_batch(B, jac_h, v_h, w_h, y, z, what):
    for p, s in enumerate(B.order):
        _check_problem(B.structs[s], jac_h[B.js(p)], v_h[B.xs(p)], w_h[B.gs(p)], y[B.gs(p)], z[B.xs(p)], "%s problem %d" % (what, p))


def test_exact_on_the_oracle_jacobian():
    """The five BASELINE cases in one handle, the oracle's Jacobian values written into the batch layout."""
    cases = [make() for _, make in sorted(baseline_cases().items())]
    B = JacBatch([c.S for c in cases], range(len(cases)), make=("ops",))
    rng = np.random.default_rng(11)
    jac_h = np.concatenate([c.P.eval(c.x_perturbed(i))[3] for i, c in enumerate(cases)])
    assert jac_h.size == B.jo[-1]
    v_h, w_h = rng.normal(size=B.X), rng.normal(size=B.G)
    y, z = B.products(dev(jac_h), dev(v_h), dev(w_h))
    _check_batch(B, jac_h, v_h, w_h, y, z, "oracle J")


def test_ragged_batch_on_the_device_jacobian():
    torch, _, st = torch_ctx()
    cases, order = ragged()
    structs = [c.S for c in cases]
    B = JacBatch(structs, order, make=("batch", "ops"))
    xo, go, jo = B.xo, B.go, B.jo
    assert np.array_equal(xo, B.batch.x_off) and np.array_equal(go, B.batch.g_off) and np.array_equal(jo, B.batch.jac_off)
    x = dev(ragged_x(cases, order))
    _, jac = B.eval(x)
    rng = np.random.default_rng(7)
    v_h, w_h = rng.normal(size=B.X), rng.normal(size=B.G)
    v, w = dev(v_h), dev(w_h)
    y, z = B.products(jac, v, w)
    jac_h = jac.cpu().numpy()
    _check_batch(B, jac_h, v_h, w_h, y, z, "device J")
    # two calls: the same bits
    y2, z2 = B.products(jac, v, w)
    assert np.array_equal(y, y2) and np.array_equal(z, z2)
    # a problem alone in a one-problem handle (its values copied: another alignment of the same entries) has the same bits
    for p in (0, 1, 2, 3, 17, 150, 299):
        one = JacBatch([structs[order[p]]], [0], make=("ops",))
        yo, zo = one.products(*(dev(a[o[p]:o[p + 1]].copy()) for a, o in ((jac_h, jo), (v_h, xo), (w_h, go))))
        assert np.array_equal(yo, y[go[p]:go[p + 1]]) and np.array_equal(zo, z[xo[p]:xo[p + 1]]), p
    # central differences of the values path along v (smooth problems: C3 and the wide one, flat terrain)
    h = 1e-6
    gp = torch.empty(B.G, dtype=torch.float64, device=x.device)
    gm = torch.empty_like(gp)
    B.batch.eval_device((x + h * v).data_ptr(), gp.data_ptr(), 0, ta.EVAL_VALUES, st)
    B.batch.eval_device((x - h * v).data_ptr(), gm.data_ptr(), 0, ta.EVAL_VALUES, st)
    torch.cuda.synchronize()
    fd = ((gp - gm) / (2 * h)).cpu().numpy()
    for p in (0, 3):
        a, b = go[p], go[p + 1]
        assert (np.abs(y[a:b] - fd[a:b]) / np.maximum(np.abs(fd[a:b]), 1.0)).max() < 1e-5, p


def test_structure_without_rows():
    torch, device, _ = torch_ctx()
    case = random_case(5111)
    assert case.S.m == 0 and case.S.nnz == 0
    B = JacBatch([case.S], [0, 0, 0], make=("ops",))
    one = torch.zeros(1, dtype=torch.float64, device=device)
    v = torch.ones(B.X, dtype=torch.float64, device=device)
    y, z = B.products(one, v, one)
    assert y.size == 0 and np.array_equal(z, np.zeros(B.X)) and not np.signbit(z).any()


def test_c3_full_batch_against_one_problem_batches():
    model = ta.model_preset("anymal", "flat")
    S = ta.Structure(model, ta.gait_combo(4, 1, 2.0))
    n = 8192
    B = JacBatch([S], [0] * n, make=("ops",))
    assert B.ops.bytes()["distinct_patterns"] == 1
    twin = ta.Structure(model, ta.gait_combo(4, 1, 2.0))
    assert ta.JacOps([S, twin], [0, 1], device=0).bytes()["distinct_patterns"] == 1
    rng = np.random.default_rng(2)
    jac = dev(rng.normal(size=B.J))
    v = dev(rng.normal(size=B.X))
    w = dev(rng.normal(size=B.G))
    y, z = B.products(jac, v, w)
    one = JacBatch([S], [0], make=("ops",))
    for p in (0, 4095, 8191):
        yo, zo = one.products(jac[B.js(p)].clone(), v[B.xs(p)].clone(), w[B.gs(p)].clone())
        assert np.array_equal(yo, y[B.gs(p)]) and np.array_equal(zo, z[B.xs(p)]), p


def test_nan_and_inf_are_contained():
    cases, order = ragged()
    B = JacBatch([c.S for c in cases], order[:40], make=("ops",))
    xo, go, jo = B.xo, B.go, B.jo
    rng = np.random.default_rng(9)
    jac_h, v_h, w_h = rng.normal(size=B.J), rng.normal(size=B.X), rng.normal(size=B.G)
    y0, z0 = B.products(dev(jac_h), dev(v_h), dev(w_h))
    bad = {5: ("jac", np.nan), 6: ("v", np.inf), 7: ("w", -np.inf), 20: ("jac", np.inf), 21: ("v", np.nan), 22: ("w", np.nan)}
    jb, vb, wb = jac_h.copy(), v_h.copy(), w_h.copy()
    for p, (where, val) in bad.items():
        arr, off = {"jac": (jb, jo), "v": (vb, xo), "w": (wb, go)}[where]
        arr[off[p]:off[p + 1]:3] = val
    y1, z1 = B.products(dev(jb), dev(vb), dev(wb))
    for p in range(B.P):
        if p in bad:
            continue
        assert np.array_equal(y0[go[p]:go[p + 1]], y1[go[p]:go[p + 1]]) and np.array_equal(z0[xo[p]:xo[p + 1]], z1[xo[p]:xo[p + 1]]), p
    assert not np.isfinite(z1[xo[5]:xo[6]]).all() and not np.isfinite(y1[go[6]:go[7]]).all()


def test_capture_eval_mul_tmul_as_one_graph():
    torch, device, _ = torch_ctx()
    cases, order = ragged()
    order = order[:24]
    B = JacBatch([c.S for c in cases], order, make=("batch", "ops"))
    rng = np.random.default_rng(4)
    x = dev(ragged_x(cases, order))
    v = dev(rng.normal(size=B.X))
    w = dev(rng.normal(size=B.G))
    jac = torch.zeros(B.J, dtype=torch.float64, device=device)
    y = torch.zeros(B.G, dtype=torch.float64, device=device)
    z = torch.zeros(B.X, dtype=torch.float64, device=device)

    def step(stream):   # a single chain: no parallel branches
        B.batch.eval_device(x.data_ptr(), 0, jac.data_ptr(), ta.EVAL_JACOBIAN, stream)
        B.ops.mul_device(jac.data_ptr(), v.data_ptr(), y.data_ptr(), stream)
        B.ops.tmul_device(jac.data_ptr(), w.data_ptr(), z.data_ptr(), stream)

    graph = capture(step)
    x1 = torch.from_numpy(ragged_x(cases, order, seed0=100))

    def reset():
        x.copy_(x1)
        y.zero_()
        z.zero_()

    assert_replay_equals_eager(step, graph, reset, (y, z))
    _check_batch(B, jac.cpu().numpy(), v.cpu().numpy(), w.cpu().numpy(), y.cpu().numpy(), z.cpu().numpy(), "graph")
