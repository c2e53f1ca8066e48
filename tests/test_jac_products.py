"""twr_jac_mul / twr_jac_tmul on the device: y = J v and z = J^T w per problem against float64 scipy, on the oracle's Jacobian
values and on the device's own, the adjoint identity, central differences of the values path, bit-reproducibility across
calls and batch compositions, containment of NaN / Inf, and stream order under hipGraph capture."""
import numpy as np
import pytest
import scipy.sparse as sp

import towr_amd as ta

from .common import Case, baseline_cases, k_params, random_case

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch, torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream


def _csr(S, vals):
    return sp.csr_matrix((vals, S.col_idx, S.row_ptr), shape=(S.m, S.n))


def _run(ops, jac, v, w, stream=None):
    """(y, z) of both products on device tensors; y / z start as NaN so that an unwritten output shows."""
    torch, dev, st = _torch()
    xo, go, _ = ops.layout()
    y = torch.full((max(1, int(go[-1])),), float("nan"), dtype=torch.float64, device=dev)
    z = torch.full((int(xo[-1]),), float("nan"), dtype=torch.float64, device=dev)
    ops.mul_device(jac.data_ptr(), v.data_ptr(), y.data_ptr(), st if stream is None else stream)
    ops.tmul_device(jac.data_ptr(), w.data_ptr(), z.data_ptr(), st if stream is None else stream)
    torch.cuda.synchronize()
    return y.cpu().numpy()[:int(go[-1])], z.cpu().numpy()


def _check_problem(S, jv, v, w, y, z, what):
    A = _csr(S, jv)
    absA = abs(A)
    ty, tz = absA @ np.abs(v), absA.T @ np.abs(w)
    assert np.all(np.abs(y - A @ v) <= 1e-12 * ty), (what, "J v", np.abs(y - A @ v).max())
    assert np.all(np.abs(z - A.T @ w) <= 1e-12 * tz), (what, "J^T w", np.abs(z - A.T @ w).max())
    lhs, rhs = w @ y, z @ v
    assert abs(lhs - rhs) <= 1e-12 * (np.abs(w) @ ty), (what, "adjoint", lhs, rhs)


def _check_batch(structs, order, jac_h, v_h, w_h, y, z, ops, what):
    xo, go, jo = ops.layout()
    for p, s in enumerate(order):
        S = structs[s]
        _check_problem(S, jac_h[jo[p]:jo[p + 1]], v_h[xo[p]:xo[p + 1]], w_h[go[p]:go[p + 1]], y[go[p]:go[p + 1]],
                       z[xo[p]:xo[p + 1]], "%s problem %d" % (what, p))


def test_exact_on_the_oracle_jacobian():
    """The five BASELINE cases in one handle, the oracle's Jacobian values written into the batch layout."""
    torch, dev, _ = _torch()
    cases = [make() for _, make in sorted(baseline_cases().items())]
    structs = [c.S for c in cases]
    ops = ta.JacOps(structs, list(range(len(cases))), device=0)
    xo, go, jo = ops.layout()
    rng = np.random.default_rng(11)
    jac_h = np.concatenate([c.P.eval(c.x_perturbed(i))[3] for i, c in enumerate(cases)])
    assert jac_h.size == jo[-1]
    v_h, w_h = rng.normal(size=int(xo[-1])), rng.normal(size=int(go[-1]))
    y, z = _run(ops, *(torch.from_numpy(a).to(dev) for a in (jac_h, v_h, w_h)))
    _check_batch(structs, range(len(cases)), jac_h, v_h, w_h, y, z, ops, "oracle J")


def _ragged():
    """About 300 problems of quadruped structures: random ones, optimised timings, a grid map, one too wide for the LDS copy
    of v in J v; struct 0 is C3."""
    cases = [Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200)),
             Case("anymal", "gap", ta.gait_combo(4, 0, 2.4, 0.9), constraint_sets=127),
             Case("anymal", "grid_map", ta.gait_combo(4, 1, 2.0),
                  grid=(np.random.default_rng(3).uniform(-0.05, 0.3, size=(40, 30)).astype(np.float32), 0.06, (0.8, -0.2))),
             Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), duration_base_poly=0.003)]
    assert cases[3].S.n > 6144
    seed = 0
    while len(cases) < 8:
        c = random_case(seed)
        if c.S.n_ee == 4:
            cases.append(c)
        seed += 1
    order = [0, 1, 2, 3] + list(np.random.default_rng(5).integers(0, len(cases), size=296))
    xs = [cases[s].x_perturbed(i) for i, s in enumerate(order)]
    return cases, order, xs


def _device_jacobian(batch, x):
    torch, dev, st = _torch()
    jac = torch.empty(int(batch.jac_off[-1]), dtype=torch.float64, device=dev)
    g = torch.empty(max(1, int(batch.g_off[-1])), dtype=torch.float64, device=dev)
    batch.eval_device(x.data_ptr(), g.data_ptr(), jac.data_ptr(), ta.EVAL_BOTH, st)
    torch.cuda.synchronize()
    return jac


def test_ragged_batch_on_the_device_jacobian():
    torch, dev, st = _torch()
    cases, order, xs = _ragged()
    structs = [c.S for c in cases]
    batch = ta.Batch(structs, order, device=0)
    ops = ta.JacOps(structs, order, device=0)
    xo, go, jo = ops.layout()
    assert np.array_equal(xo, batch.x_off) and np.array_equal(go, batch.g_off) and np.array_equal(jo, batch.jac_off)
    x = torch.from_numpy(np.concatenate(xs)).to(dev)
    jac = _device_jacobian(batch, x)
    rng = np.random.default_rng(7)
    v_h, w_h = rng.normal(size=int(xo[-1])), rng.normal(size=int(go[-1]))
    v, w = torch.from_numpy(v_h).to(dev), torch.from_numpy(w_h).to(dev)
    y, z = _run(ops, jac, v, w)
    jac_h = jac.cpu().numpy()
    _check_batch(structs, order, jac_h, v_h, w_h, y, z, ops, "device J")
    # two calls: the same bits
    y2, z2 = _run(ops, jac, v, w)
    assert np.array_equal(y, y2) and np.array_equal(z, z2)
    # a problem alone in a one-problem handle (its values copied: another alignment of the same entries) has the same bits
    for p in (0, 1, 2, 3, 17, 150, 299):
        s = order[p]
        one = ta.JacOps([structs[s]], [0], device=0)
        yo, zo = _run(one, *(torch.from_numpy(a[o[p]:o[p + 1]].copy()).to(dev)
                             for a, o in ((jac_h, jo), (v_h, xo), (w_h, go))))
        assert np.array_equal(yo, y[go[p]:go[p + 1]]) and np.array_equal(zo, z[xo[p]:xo[p + 1]]), p
    # central differences of the values path along v (smooth problems: C3 and the wide one, flat terrain)
    h = 1e-6
    gp = torch.empty(int(go[-1]), dtype=torch.float64, device=dev)
    gm = torch.empty_like(gp)
    batch.eval_device((x + h * v).data_ptr(), gp.data_ptr(), 0, ta.EVAL_VALUES, st)
    batch.eval_device((x - h * v).data_ptr(), gm.data_ptr(), 0, ta.EVAL_VALUES, st)
    torch.cuda.synchronize()
    fd = ((gp - gm) / (2 * h)).cpu().numpy()
    for p in (0, 3):
        a, b = go[p], go[p + 1]
        assert (np.abs(y[a:b] - fd[a:b]) / np.maximum(np.abs(fd[a:b]), 1.0)).max() < 1e-5, p


def test_structure_without_rows():
    torch, dev, _ = _torch()
    case = random_case(5111)
    assert case.S.m == 0 and case.S.nnz == 0
    ops = ta.JacOps([case.S], [0, 0, 0], device=0)
    xo, _, _ = ops.layout()
    one = torch.zeros(1, dtype=torch.float64, device=dev)
    v = torch.ones(int(xo[-1]), dtype=torch.float64, device=dev)
    y, z = _run(ops, one, v, one)
    assert y.size == 0 and np.array_equal(z, np.zeros(int(xo[-1]))) and not np.signbit(z).any()


def test_c3_full_batch_against_one_problem_batches():
    torch, dev, st = _torch()
    model = ta.model_preset("anymal", "flat")
    S = ta.Structure(model, ta.gait_combo(4, 1, 2.0))
    n = 8192
    ops = ta.JacOps([S], [0] * n, device=0)
    assert ops.bytes()["distinct_patterns"] == 1
    twin = ta.Structure(model, ta.gait_combo(4, 1, 2.0))
    assert ta.JacOps([S, twin], [0, 1], device=0).bytes()["distinct_patterns"] == 1
    xo, go, jo = ops.layout()
    rng = np.random.default_rng(2)
    jac = torch.from_numpy(rng.normal(size=int(jo[-1]))).to(dev)
    v = torch.from_numpy(rng.normal(size=int(xo[-1]))).to(dev)
    w = torch.from_numpy(rng.normal(size=int(go[-1]))).to(dev)
    y, z = _run(ops, jac, v, w)
    one = ta.JacOps([S], [0], device=0)
    for p in (0, 4095, 8191):
        yo, zo = _run(one, jac[jo[p]:jo[p + 1]].clone(), v[xo[p]:xo[p + 1]].clone(), w[go[p]:go[p + 1]].clone())
        assert np.array_equal(yo, y[go[p]:go[p + 1]]) and np.array_equal(zo, z[xo[p]:xo[p + 1]]), p


def test_nan_and_inf_are_contained():
    torch, dev, _ = _torch()
    cases, order, xs = _ragged()
    order, xs = order[:40], xs[:40]
    structs = [c.S for c in cases]
    ops = ta.JacOps(structs, order, device=0)
    xo, go, jo = ops.layout()
    rng = np.random.default_rng(9)
    jac_h, v_h, w_h = rng.normal(size=int(jo[-1])), rng.normal(size=int(xo[-1])), rng.normal(size=int(go[-1]))
    y0, z0 = _run(ops, *(torch.from_numpy(a).to(dev) for a in (jac_h, v_h, w_h)))
    bad = {5: ("jac", np.nan), 6: ("v", np.inf), 7: ("w", -np.inf), 20: ("jac", np.inf), 21: ("v", np.nan), 22: ("w", np.nan)}
    jb, vb, wb = jac_h.copy(), v_h.copy(), w_h.copy()
    for p, (where, val) in bad.items():
        arr, off = {"jac": (jb, jo), "v": (vb, xo), "w": (wb, go)}[where]
        arr[off[p]:off[p + 1]:3] = val
    y1, z1 = _run(ops, *(torch.from_numpy(a).to(dev) for a in (jb, vb, wb)))
    for p in range(len(order)):
        if p in bad:
            continue
        assert np.array_equal(y0[go[p]:go[p + 1]], y1[go[p]:go[p + 1]]) and np.array_equal(z0[xo[p]:xo[p + 1]], z1[xo[p]:xo[p + 1]]), p
    assert not np.isfinite(z1[xo[5]:xo[6]]).all() and not np.isfinite(y1[go[6]:go[7]]).all()


def test_capture_eval_mul_tmul_as_one_graph():
    torch, dev, _ = _torch()
    cases, order, xs = _ragged()
    order, xs = order[:24], xs[:24]
    structs = [c.S for c in cases]
    batch = ta.Batch(structs, order, device=0)
    ops = ta.JacOps(structs, order, device=0)
    xo, go, jo = ops.layout()
    rng = np.random.default_rng(4)
    x = torch.from_numpy(np.concatenate(xs)).to(dev)
    v = torch.from_numpy(rng.normal(size=int(xo[-1]))).to(dev)
    w = torch.from_numpy(rng.normal(size=int(go[-1]))).to(dev)
    jac = torch.zeros(int(jo[-1]), dtype=torch.float64, device=dev)
    y = torch.zeros(int(go[-1]), dtype=torch.float64, device=dev)
    z = torch.zeros(int(xo[-1]), dtype=torch.float64, device=dev)

    def step(stream):
        batch.eval_device(x.data_ptr(), 0, jac.data_ptr(), ta.EVAL_JACOBIAN, stream)
        ops.mul_device(jac.data_ptr(), v.data_ptr(), y.data_ptr(), stream)
        ops.tmul_device(jac.data_ptr(), w.data_ptr(), z.data_ptr(), stream)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture (module load)
        step(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(torch.cuda.current_stream().cuda_stream)
    x.copy_(torch.from_numpy(np.concatenate([cases[s].x_perturbed(100 + i) for i, s in enumerate(order)])))
    y.zero_()
    z.zero_()
    graph.replay()
    torch.cuda.synchronize()
    gy, gz = y.clone(), z.clone()
    y.zero_()
    z.zero_()
    step(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(gy, y) and torch.equal(gz, z)
    _check_batch(structs, order, jac.cpu().numpy(), v.cpu().numpy(), w.cpu().numpy(), y.cpu().numpy(), z.cpu().numpy(), ops, "graph")
