"""The device harness of the Jacobian solver tests (tests/test_jac_*.py): the ragged batch, the handles of one batch with the
calls under test on device tensors, and hipGraph capture.  Every output a helper allocates starts as NaN, so that an unwritten
output shows.  The reference side (numpy / scipy, the bounds) is tests/jac_ref.py."""
import functools

import numpy as np
import scipy.sparse as sp

import towr_amd as ta

from .common import Case, k_params, random_case
from .jac_ref import ITERS, REL_FLOOR, STEPS, TOL, csr, lm_case, same_bits

F = {k: i for i, k in enumerate(ta.JacLm.FIELDS)}


def torch_ctx():
    import torch

    return torch, torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream


def dev(a):
    torch, device, _ = torch_ctx()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def nan(n):
    torch, device, _ = torch_ctx()
    return torch.full((max(1, int(n)),), float("nan"), dtype=torch.float64, device=device)


# ---------------------------------------------------------------- batches

@functools.lru_cache(maxsize=None)
def ragged():
    """(cases, order) of about 300 problems of quadruped structures: random ones, optimised timings, a grid map, one too wide
    for the LDS copy of a vector in the x layout; struct 0 is C3, struct 1 the gap with every constraint set.  Built once per
    process: shared by the tests, never changed."""
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
    return tuple(cases), tuple(order)


def ragged_x(cases, order, point="x_perturbed", seed0=0):
    """The concatenated start vector of problems in `order`: problem i at point(seed0 + i)."""
    return np.concatenate([getattr(cases[s], point)(seed0 + i) for i, s in enumerate(order)])


class JacBatch:
    """Batch + JacOps + JacLsq of the same arguments and the calls under test on device tensors.  A handle is made on first
    use; `make` names those made at once, in that order."""

    def __init__(self, structs, order, make=("ops", "lsq")):
        self.structs, self.order = structs, list(order)
        for name in make:
            getattr(self, name)
        self.xo, self.go, self.jo = self.ops.layout()
        self.P = len(self.order)
        self.X, self.G, self.J = int(self.xo[-1]), int(self.go[-1]), int(self.jo[-1])

    @functools.cached_property
    def batch(self):
        return ta.Batch(self.structs, self.order, device=0)

    @functools.cached_property
    def ops(self):
        return ta.JacOps(self.structs, self.order, device=0)

    @functools.cached_property
    def lsq(self):
        return ta.JacLsq(self.ops)

    @functools.cached_property
    def _bounds(self):
        b = [self.structs[s].bounds() for s in self.order]
        return [np.concatenate([v[i] for v in b]) if self.G else np.zeros(0) for i in (0, 1)]

    @property
    def lo(self):
        """The structures' lower bounds in the g layout, on the host."""
        return self._bounds[0]

    @property
    def hi(self):
        return self._bounds[1]

    def xs(self, p):
        return slice(self.xo[p], self.xo[p + 1])

    def gs(self, p):
        return slice(self.go[p], self.go[p + 1])

    def js(self, p):
        return slice(self.jo[p], self.jo[p + 1])

    def A(self, p, jac_h):
        return csr(self.structs[self.order[p]], jac_h[self.js(p)])

    def eval(self, x, flags=ta.EVAL_BOTH):
        torch, _, st = torch_ctx()
        g, jac = nan(self.G), nan(self.J)
        self.batch.eval_device(x.data_ptr(), g.data_ptr(), jac.data_ptr(), flags, st)
        torch.cuda.synchronize()
        return g, jac

    def violation(self, g, w=None, merit=True):
        """(r, w_active, merit) of twr_jac_violation; merit False: d_merit is left out, and None is returned for it."""
        torch, _, st = torch_ctx()
        r, wa, m = nan(self.G), nan(self.G), nan(self.P) if merit else None
        self.lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w=0 if w is None else w.data_ptr(), d_w_active=wa.data_ptr(),
                                  d_merit=m.data_ptr() if merit else 0, stream=st)
        torch.cuda.synchronize()
        return r, wa, m

    def linearise(self, x, merit=True):
        """(jac, b = -viol, active-set weights) at x."""
        g, jac = self.eval(x)
        r, wa, _ = self.violation(g, merit=merit)
        return jac, -r, wa

    def colsq(self, jac, w, stream=None):
        torch, _, st = torch_ctx()
        out = nan(self.X)
        self.ops.col_sqnorms_device(jac.data_ptr(), out.data_ptr(), d_w=0 if w is None else w.data_ptr(), stream=stream or st)
        torch.cuda.synchronize()
        return out

    def scale(self, colsq, rel_floor=REL_FLOOR, colmax=None, stream=None):
        torch, _, st = torch_ctx()
        c = nan(self.X)
        self.lsq.col_scale_device(colsq.data_ptr(), c.data_ptr(), rel_floor, d_colsq_max=0 if colmax is None else colmax.data_ptr(),
                                  stream=stream or st)
        torch.cuda.synchronize()
        return c

    def col_scale(self, jac, w, rel_floor=REL_FLOOR):
        """(column norms, scale): the norms, then the scale of them."""
        q = self.colsq(jac, w)
        return q, self.scale(q, rel_floor)

    def products(self, jac, v, w, stream=None):
        """(y, z) of twr_jac_mul and twr_jac_tmul, on the host."""
        torch, _, st = torch_ctx()
        y, z = nan(self.G), nan(self.X)
        self.ops.mul_device(jac.data_ptr(), v.data_ptr(), y.data_ptr(), stream or st)
        self.ops.tmul_device(jac.data_ptr(), w.data_ptr(), z.data_ptr(), stream or st)
        torch.cuda.synchronize()
        return y.cpu().numpy()[:self.G], z.cpu().numpy()[:self.X]

    def normal(self, jac, v, w, with_y=True, stream=None):
        """(y or None, u) of one twr_jac_normal_mul, on the host."""
        torch, _, st = torch_ctx()
        y, u = nan(self.G), nan(self.X)
        self.ops.normal_mul_device(jac.data_ptr(), v.data_ptr(), u.data_ptr(), d_w=0 if w is None else w.data_ptr(),
                                   d_y=y.data_ptr() if with_y else 0, stream=stream or st)
        torch.cuda.synchronize()
        return (y.cpu().numpy()[:self.G] if with_y else None), u.cpu().numpy()[:self.X]

    def solve(self, jac, b, w, mu, c=None, kind="cgls", iters=ITERS, tol=TOL, stream=None):
        """(d, info[n_problems, 4]) of one solve, on the host (w None: unit weights).  kind: "cgls" twr_jac_lsq_solve (no c),
        "scaled" twr_jac_lsq_solve_scaled, "masked" twr_jac_lsq_solve_masked, "onepass" twr_jac_lsq_solve_onepass (c None:
        unscaled)."""
        torch, _, st = torch_ctx()
        d, info = nan(self.X), nan(4 * self.P)
        ins, outs = (jac.data_ptr(), b.data_ptr(), mu.data_ptr()), (d.data_ptr(), info.data_ptr(), iters, tol)
        kw = dict(d_w=0 if w is None else w.data_ptr(), stream=stream or st)
        if kind == "cgls":
            assert c is None
            self.lsq.solve_device(*ins, *outs, **kw)
        elif kind == "onepass":
            self.lsq.solve_onepass_device(*ins, *outs, d_scale=0 if c is None else c.data_ptr(), **kw)
        else:
            f = {"scaled": self.lsq.solve_scaled_device, "masked": self.lsq.solve_masked_device}[kind]
            f(*ins, c.data_ptr(), *outs, **kw)
        torch.cuda.synchronize()
        return d.cpu().numpy()[:self.X], info.cpu().numpy()[:4 * self.P].reshape(-1, 4)


def c3_batch(n, seed0=0, merit=True):
    """(case, batch, x, g, jac, b = -viol, active-set weights) of n C3 problems at x_perturbed(seed0 ..)."""
    c = Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200))
    B = JacBatch([c.S], [0] * n)
    x = dev(np.concatenate([c.x_perturbed(seed0 + i) for i in range(n)]))
    g, jac = B.eval(x)
    r, wa, _ = B.violation(g, merit=merit)
    return c, B, x, g, jac, -r, wa


class GramBatch(JacBatch):
    """JacBatch with the Gram tables reserved, the layout of N and every problem's pattern."""

    def __init__(self, structs, order):
        super().__init__(structs, order)
        self.ops.reserve_gram()
        self.no = self.ops.gram_layout()
        pats = [S.gram_pattern() for S in structs]
        self.pat = [pats[s] for s in self.order]

    def form(self, jac, w=None, stream=None):
        torch, _, st = torch_ctx()
        N = nan(self.no[-1])
        self.ops.gram_device(jac.data_ptr(), N.data_ptr(), d_w=0 if w is None else w.data_ptr(), stream=stream or st)
        torch.cuda.synchronize()
        return N

    def mul(self, N, v, stream=None):
        torch, _, st = torch_ctx()
        u = nan(self.X)
        self.ops.gram_mul_device(N.data_ptr(), v.data_ptr(), u.data_ptr(), stream=stream or st)
        torch.cuda.synchronize()
        return u.cpu().numpy()[:self.X]

    def tmul(self, jac, t):
        torch, _, st = torch_ctx()
        z = nan(self.X)
        self.ops.tmul_device(jac.data_ptr(), t.data_ptr(), z.data_ptr(), st)
        torch.cuda.synchronize()
        return z

    def solve(self, N, z, mu, c=None, iters=ITERS, tol=TOL, stream=None):
        """(d, info[n_problems, 4]) of one twr_jac_lsq_solve_gram, on the host."""
        torch, _, st = torch_ctx()
        d, info = nan(self.X), nan(4 * self.P)
        self.lsq.solve_gram_device(N.data_ptr(), z.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), iters, tol,
                                   d_scale=0 if c is None else c.data_ptr(), stream=stream or st)
        torch.cuda.synchronize()
        return d.cpu().numpy()[:self.X], info.cpu().numpy().reshape(-1, 4)

    def csr(self, p, N_h):
        rp, ci = self.pat[p]
        n = len(rp) - 1
        return sp.csr_matrix((N_h[self.no[p]:self.no[p] + len(ci)], ci, rp), shape=(n, n))


def lm_inputs(problems):
    """(structures, order, x0, lo, up) of a batch of (name, seed) problems of tests/jac_ref.py::lm_case."""
    names = []
    for name, _ in problems:
        if name not in names:
            names.append(name)
    order = [names.index(name) for name, _ in problems]
    x0 = np.concatenate([lm_case(name)[0].x_perturbed(seed) for name, seed in problems])
    lo = np.concatenate([lm_case(name)[1][0] for name, _ in problems])
    up = np.concatenate([lm_case(name)[1][1] for name, _ in problems])
    return [lm_case(n)[0].S for n in names], order, x0, lo, up


class LmBatch(JacBatch):
    """JacBatch + JacLm of a batch of (name, seed) problems, and the caller's buffers."""

    def __init__(self, problems, **params):
        self.problems = tuple(problems)
        structs, order, self.x0, self.lo_h, self.up_h = lm_inputs(problems)
        super().__init__(structs, order, make=("batch", "ops", "lsq"))
        self.lm = ta.JacLm(self.batch, self.lsq, **params)
        self.x, self.d_lo, self.d_up = nan(self.X), nan(self.X), nan(self.X)
        self.g, self.jac, self.rec = nan(self.G), nan(self.J), nan(ta.JacLm.REC * self.P)

    def start(self, x_h=None, lo_h=None, up_h=None, stream=None):
        torch, _, st = torch_ctx()
        self.x[:self.X].copy_(torch.from_numpy(np.ascontiguousarray(self.x0 if x_h is None else x_h)))
        self.d_lo[:self.X].copy_(torch.from_numpy(np.ascontiguousarray(self.lo_h if lo_h is None else lo_h)))
        self.d_up[:self.X].copy_(torch.from_numpy(np.ascontiguousarray(self.up_h if up_h is None else up_h)))
        self.lm.start_device(self.x.data_ptr(), self.d_lo.data_ptr(), self.d_up.data_ptr(), self.g.data_ptr(), self.jac.data_ptr(),
                             stream or st)

    def step(self, k=1, stream=None):
        _, _, st = torch_ctx()
        for _ in range(k):
            self.lm.step_device(stream or st)

    def read(self, stream=None):
        """(x, state records [P, 8]) on the host."""
        torch, _, st = torch_ctx()
        self.lm.state_device(self.rec.data_ptr(), stream or st)
        torch.cuda.synchronize()
        return self.x.cpu().numpy()[:self.X].copy(), self.rec.cpu().numpy()[:ta.JacLm.REC * self.P].reshape(self.P, -1).copy()

    def run(self, steps=STEPS, **start):
        """[(x, records)] after the start and after every step."""
        self.start(**start)
        hist = [self.read()]
        for _ in range(steps):
            self.step()
            hist.append(self.read())
        return hist


# ---------------------------------------------------------------- hipGraph

def capture(step):
    """step(stream) run once on a side stream (the warm-up: module load stays outside the capture), then captured on a
    non-default stream of its own; the graph.  step is a single chain: no parallel branches."""
    torch, _, _ = torch_ctx()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(torch.cuda.current_stream().cuda_stream)
    return graph


def assert_replay_equals_eager(step, graph, reset, outs):
    """reset(), a replay, a snapshot of outs; reset() again, step run eagerly: every output has the replay's bits."""
    torch, _, _ = torch_ctx()
    reset()
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in outs]
    reset()
    step(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for a, e in zip(got, outs):
        assert same_bits(a.cpu().numpy(), e.cpu().numpy())
