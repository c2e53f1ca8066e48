"""The bound-constrained Levenberg-Marquardt driver on the device (twr_jac_lsq_solve_masked, twr_jac_free_set, twr_jac_lm_*) on
12 problems: the hopper C1 (n = 339, odd: every later problem starts on an odd offset, the 8-byte load path), the hopper and the
biped with TWR_SETS_ALL (optimised timings: box bounds on every phase duration), ANYmal at towr's default grids (n = 640 > 512:
the lanes of a workgroup loop), a structure without rows (a biped, n = 315); x = x_perturbed(seed), the bounds of
twr_structure_variable_bounds for the start and goal the guess interpolates (scripts/lm_box_cpu.py::case_bounds).  A twr_batch
holds structures of one foot count only, so the problems make three ragged batches (GROUPS of tests/jac_ref.py, which the CPU
tests share), one per robot; every test runs on each of them.

Bounds of the comparisons:
  * the masked step against a dense direct solve on the free columns of the ORACLE's Jacobian: those of
    tests/jac_ref.py::check_scaled_step (tol 1e-10, mu = 1e-2 lambda_max; true residual <= 2 tol, |e - direct| <= 101 * 2 tol
    |direct|, under 200 iterations): the same iteration on fewer columns.
  * against scripts/lm_box_cpu.py (numpy on the CPU oracle) on the same inputs: the merit after one step within 1e-6 relative (the
    CPU run moves by up to 1.3e-7 under a 2e-8 relative jitter of its steps on these inputs), the final merit after 8 steps within
    [0.5, 2] of the CPU's.  The seeds were chosen on the CPU alone: under that jitter (16 draws per problem) the CPU's own final
    merit moves by a factor of at most 1.03 on these inputs with unchanged accept sequences (other seeds flip an
    accept and move by 1.6 or 100, which would test the jitter, not the driver).
Hostile inputs (NaN, Inf, 1e300 in x, lo > up, a NaN bound, a first phase duration of zero whose box the test opens -- inside its
box [0.2, 1] the projection would simply repair it) are inputs, not provoked faults: every index comes from host tables."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import towr_amd as ta

from .jac_device import F, LmBatch, dev, lm_inputs, nan, torch_ctx
from .jac_ref import GROUPS, ITERS, REJECTS_FIRST, ROOT, STEPS, TOL, bits, check_scaled_step, lam_max, lm_case, same_bits

sys.path.insert(0, os.path.join(ROOT, "scripts"))

import lm_box_cpu as lb  # noqa: E402

pytestmark = pytest.mark.gpu

groups = pytest.mark.parametrize("group", list(GROUPS))


@functools.lru_cache(maxsize=None)
def _cpu(name, seed):
    case, (lo, up) = lm_case(name)
    return lb.lm_box(case, case.x_perturbed(seed), lo, up, steps=STEPS)


@functools.lru_cache(maxsize=None)
def _main(group):
    """The batch of a group and its eager run of STEPS steps: shared, never changed."""
    B = LmBatch(GROUPS[group])
    return B, B.run()


def _norows(B, p):
    return B.problems[p][0] == "norows"


def _linearise(B, x_h):
    """The chain of a step up to the free set with the public calls, at x_h: device tensors."""
    torch, _, st = torch_ctx()
    x, lo, up = dev(x_h), dev(B.lo_h), dev(B.up_h)
    g, jac = B.eval(x)
    r, wa, _ = B.violation(g, merit=False)
    b = -r
    q, c = B.col_scale(jac, wa)
    z, cf, nf = nan(B.X), nan(B.X), nan(B.P)
    t = wa * b
    B.ops.tmul_device(jac.data_ptr(), t.data_ptr(), z.data_ptr(), st)
    B.lsq.free_set_device(x.data_ptr(), lo.data_ptr(), up.data_ptr(), z.data_ptr(), cf.data_ptr(), nf.data_ptr(), d_scale_in=c.data_ptr(),
                          stream=st)
    torch.cuda.synchronize()
    return dict(x=x, lo=lo, up=up, jac=jac, b=b, wa=wa, q=q, c=c, z=z, cf=cf, nf=nf)


def _oracle(B, p, x_h):
    """(A, r, w) of problem p at x_h from the CPU oracle."""
    case = lm_case(B.problems[p][0])[0]
    S = case.S
    out = case.P.eval(x_h[B.xs(p)])
    glo, ghi = S.bounds()
    r = out[0] - np.clip(out[0], glo, ghi)
    return sp.csr_matrix((out[3], S.col_idx, S.row_ptr), shape=(S.m, S.n)), r, (r != 0).astype(np.float64)


def _oracle_z(problems, xo, p, x_h):
    """z = J^T(w o b) of problem p at x_h from the CPU oracle."""
    case = lm_case(problems[p][0])[0]
    out = case.P.eval(x_h[xo[p]:xo[p + 1]])
    glo, ghi = case.S.bounds()
    r = out[0] - np.clip(out[0], glo, ghi)
    return sp.csr_matrix((out[3], case.S.col_idx, case.S.row_ptr), shape=(case.S.m, case.S.n)).T @ -r


def _place_on_bounds(problems, xo, x, lo, up, count):
    """Puts `count` boxed variables of x (in place) on a bound, alternating lower and upper, such that at the final x every one
    of them has |z_k| > 1e-3 max|z| on the CPU oracle (moving one duration changes z): candidates in the order of a seeded
    permutation, one kept only if it and those placed before it in its problem stay clear.  Returns their indices."""
    boxed = np.nonzero((lo != up) & ((lo > -1e19) | (up < 1e19)))[0]
    hand = []
    for k in boxed[np.random.default_rng(8).permutation(len(boxed))]:
        if len(hand) == count:
            break
        p = int(np.searchsorted(xo, k, side="right") - 1)
        old = x[k]
        x[k] = lo[k] if len(hand) % 2 == 0 else up[k]
        z = _oracle_z(problems, xo, p, x)
        mine = [j for j in hand + [k] if xo[p] <= j < xo[p + 1]]
        if (np.abs(z[np.array(mine) - xo[p]]) > 1e-3 * np.abs(z).max()).all():
            hand.append(int(k))
        else:
            x[k] = old
    return np.array(hand, dtype=np.int64)


# ---------------------------------------------------------------- 1. the masked step

@groups
def test_masked_step_against_a_direct_solve_on_the_free_columns(group):
    B, _ = _main(group)
    xp = np.clip(B.x0, B.lo_h, B.up_h)
    L = _linearise(B, xp)
    b_h, w_h, c_h, cf_h, jac_h, q_h = (L[k].cpu().numpy() for k in ("b", "wa", "c", "cf", "jac", "q"))
    assert np.isfinite(c_h[:B.X]).all() and (c_h[:B.X] > 0).all()
    free = cf_h[:B.X] != 0
    assert same_bits(cf_h[:B.X][free], c_h[:B.X][free]) and not np.signbit(cf_h[:B.X][~free]).any()
    mu_h = np.zeros(B.P)
    for p in range(B.P):
        S = B.structs[B.order[p]]
        A = sp.csr_matrix((jac_h[B.jo[p]:B.jo[p + 1]], S.col_idx, S.row_ptr), shape=(S.m, S.n))
        mu_h[p] = 1e-2 * lam_max((A @ sp.diags(cf_h[B.xs(p)])).tocsr(), w_h[B.gs(p)])
    d, info = B.solve(L["jac"], L["b"], L["wa"], dev(mu_h), L["cf"], "masked")
    assert np.isfinite(d).all()
    assert not bits(d[~free]).any(), "a masked variable did not get an exact +0"
    for p in range(B.P):
        fp = free[B.xs(p)]
        fixed = B.lo_h[B.xs(p)] == B.up_h[B.xs(p)]
        assert not fp[fixed].any(), (p, "a fixed variable on its value is free")
        if _norows(B, p):
            assert np.array_equal(info[p], [0, 0, 0, 0]) and not d[B.xs(p)].any()
            continue
        A, _, _ = _oracle(B, p, xp)
        Af = A[:, np.nonzero(fp)[0]].tocsr()
        w = w_h[B.gs(p)]
        zero = q_h[B.xs(p)][fp] == 0   # the device's column norms, as tests/test_jac_scaled.py takes them
        check_scaled_step(Af, b_h[B.gs(p)], w, mu_h[p], c_h[B.xs(p)][fp], d[B.xs(p)][fp], info[p], zero,
                          "problem %d %s, %d free of %d" % (p, B.problems[p], fp.sum(), fp.size))
    # no zero in c: the bits of twr_jac_lsq_solve_scaled, d and info, under the cap and converged
    for iters, tol in ((ITERS, TOL), (7, 0.0)):
        d0, i0 = B.solve(L["jac"], L["b"], L["wa"], dev(np.maximum(mu_h, 1e-3)), L["c"], "scaled", iters, tol)
        d1, i1 = B.solve(L["jac"], L["b"], L["wa"], dev(np.maximum(mu_h, 1e-3)), L["c"], "masked", iters, tol)
        assert same_bits(d0, d1) and same_bits(i0, i1) and d0.any()
    # a negative, NaN or Inf c_k stays bad input, in its problem alone; an all-zero c converges at once with d = 0
    cbad = L["cf"].clone()
    values = (-1.0, float("nan"), float("inf"))
    bad = {p: values[(p // 2) % 3] for p in range(1, B.P, 2)}   # every second problem; the first one gets an all-zero c
    for p, v in bad.items():
        cbad[int(B.xo[p]) + int(np.nonzero(free[B.xs(p)])[0][5])] = v
    cbad[B.xs(0)] = 0.0
    d2, i2 = B.solve(L["jac"], L["b"], L["wa"], dev(mu_h), cbad, "masked")
    for p in range(B.P):
        if p in bad:
            assert i2[p, 3] == 2 and not d2[B.xs(p)].any(), (p, i2[p])
        elif p == 0:
            assert np.array_equal(i2[p], [0, 0, 0, 0]) and not bits(d2[B.xs(p)]).any()
        else:
            assert same_bits(d2[B.xs(p)], d[B.xs(p)]) and same_bits(i2[p], info[p]), p


# ---------------------------------------------------------------- 2. the free set

@groups
def test_free_set_against_numpy(group):
    torch, device, st = torch_ctx()
    B, _ = _main(group)
    x = np.clip(B.x0, B.lo_h, B.up_h)
    fixed = B.lo_h == B.up_h
    bounded = ~fixed & ((B.lo_h > -1e19) | (B.up_h < 1e19))
    # 8 durations placed on a bound by hand, alternating sides, among those whose z is far from 0 (ANYmal here has no box)
    assert bounded.sum() >= 16 or group == "anymal"
    hand = _place_on_bounds(B.problems, B.xo, x, B.lo_h, B.up_h, 8)
    assert len(hand) == 8 or group == "anymal"
    L = _linearise(B, x)
    cf, c, z_d, nf = (L[k].cpu().numpy() for k in ("cf", "c", "z", "nf"))
    got_blocked = cf[:B.X] == 0
    compared = np.zeros(B.X, dtype=bool)
    ref_blocked = np.zeros(B.X, dtype=bool)
    for p in range(B.P):
        s = B.xs(p)
        A, r, w = _oracle(B, p, x)
        z = A.T @ (w * -r)
        thr = 1e-6 * np.abs(z).max() if z.size else 0.0
        ref = lb.blocked(x[s], B.lo_h[s], B.up_h[s], z)
        sure = fixed[s] | (bounded[s] & (np.abs(z) > thr))   # every variable of this kind is compared: none is left out
        compared[s], ref_blocked[s] = sure, ref
        assert np.array_equal(got_blocked[s][sure], ref[sure]), (p, np.nonzero((got_blocked[s] != ref) & sure)[0])
        assert not got_blocked[s][~fixed[s] & ~bounded[s]].any(), (p, "a variable without bounds is blocked")
        unsure = int((bounded[s] & ~sure & ((x[s] <= B.lo_h[s]) | (x[s] >= B.up_h[s]))).sum())   # on a bound, z within 1e-6 of 0
        assert nf[p] == (~got_blocked[s]).sum(), (p, nf[p])
        assert abs(nf[p] - (~ref).sum()) <= unsure, (p, nf[p], (~ref).sum(), unsure)
    assert compared[hand].all(), "a hand-placed variable was left out of the comparison"
    outcomes = int(ref_blocked[hand].sum())
    assert 0 < outcomes or group == "anymal", "no hand-placed variable is blocked: the comparison is vacuous"
    assert same_bits(cf[:B.X][~got_blocked], c[:B.X][~got_blocked]) and not bits(cf[:B.X][got_blocked]).any()
    # without a scale: ones
    ones, nf1 = nan(B.X), nan(B.P)
    B.lsq.free_set_device(L["x"].data_ptr(), L["lo"].data_ptr(), L["up"].data_ptr(), L["z"].data_ptr(), ones.data_ptr(), nf1.data_ptr(),
                          stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(ones.cpu().numpy()[:B.X], (~got_blocked).astype(np.float64)) and same_bits(nf1.cpu().numpy(), nf)
    print("free set %s: %d hand-placed on a bound, %d of them blocked; %d variables compared, free counts %s"
          % (group, len(hand), outcomes, compared.sum(), nf[:B.P]))


# ---------------------------------------------------------------- 3. after 1 and 8 steps

@groups
def test_steps_honour_the_box_and_keep_their_books(group):
    B, hist = _main(group)
    fixed = B.lo_h == B.up_h
    par = B.lm.params
    x_start, rec_start = hist[0]
    assert same_bits(x_start, np.clip(B.x0, B.lo_h, B.up_h)), "start does not project x onto the box"
    rejected = 0
    for k in range(1, STEPS + 1):
        (x0, r0), (x1, r1) = hist[k - 1], hist[k]
        assert same_bits(x1[fixed], B.lo_h[fixed]), (k, "a fixed variable lost the bits of its bound")
        assert ((x1 >= B.lo_h) & (x1 <= B.up_h)).all(), k
        for p in range(B.P):
            a, b = r0[p], r1[p]
            n_fixed = int(fixed[B.xs(p)].sum())
            if _norows(B, p):
                continue
            assert a[F["state"]] == b[F["state"]] == ta.JacLm.RUNNING, (k, p, b)
            assert b[F["steps"]] == k and b[F["merit_start"]] == rec_start[p, F["merit_start"]] == rec_start[p, F["merit"]]
            ok = b[F["accepted"]] - a[F["accepted"]]
            assert ok in (0.0, 1.0)
            if ok:
                assert b[F["merit"]] < a[F["merit"]] and not same_bits(x1[B.xs(p)], x0[B.xs(p)]), (k, p)
                assert b[F["mu"]] == min(max(a[F["mu"]] * par.mu_down, par.mu_min), par.mu_max), (k, p)
            else:
                rejected += 1
                assert same_bits(b[F["merit"]:F["merit"] + 1], a[F["merit"]:F["merit"] + 1]), (k, p)
                assert same_bits(x1[B.xs(p)], x0[B.xs(p)]), (k, p, "a rejected step moved x")
                assert b[F["mu"]] == min(max(a[F["mu"]] * par.mu_up, par.mu_min), par.mu_max), (k, p)
            assert 0 < b[F["free"]] <= B.xo[p + 1] - B.xo[p] - n_fixed and b[F["free"]] == int(b[F["free"]])
            assert 0 < b[F["cg_iters"]] <= par.cg_iters
    if REJECTS_FIRST in B.problems:
        assert hist[1][1][B.problems.index(REJECTS_FIRST), F["accepted"]] == 0, "biped SETS_ALL seed 1 accepted its first step"
    assert rejected >= 1
    final = hist[-1][1]
    assert (final[:, F["merit"]] <= final[:, F["merit_start"]]).all()
    moved = [len(set(h[1][p, F["free"]] for h in hist[1:])) for p in range(B.P)]
    assert max(moved) > 1 or group == "anymal", "no free count moved between steps: the active set is not exercised"
    print("accepted of %d steps: %s; free counts at the end %s" % (STEPS, final[:, F["accepted"]], final[:, F["free"]]))


def test_mu_is_clamped():
    B = LmBatch(GROUPS["hopper"][:4], mu_min=0.5, mu_max=2.0)
    hist = B.run(3)
    par = B.lm.params
    for k in range(len(hist)):
        mu = hist[k][1][:, F["mu"]]
        assert ((mu >= 0.5) & (mu <= 2.0)).all(), (k, mu)
        if k:
            ok = hist[k][1][:, F["accepted"]] - hist[k - 1][1][:, F["accepted"]]
            want = np.clip(hist[k - 1][1][:, F["mu"]] * np.where(ok == 1, par.mu_down, par.mu_up), 0.5, 2.0)
            assert same_bits(mu, want), (k, mu, want)
    assert (hist[-1][1][:, F["mu"]] == 0.5).any() or (hist[-1][1][:, F["mu"]] == 2.0).any(), "the clamp never bound"


# ---------------------------------------------------------------- 4. against the CPU restatement

@groups
def test_merits_against_the_cpu_restatement(group):
    B, hist = _main(group)
    lines, bad = [], []
    for p in range(B.P):
        C = _cpu(*B.problems[p])
        dev1, devN = hist[1][1][p, F["merit"]], hist[-1][1][p, F["merit"]]
        cpu0, cpu1, cpuN = C["merit"][0], C["merit"][1] if len(C["merit"]) > 1 else C["merit"][0], C["merit"][-1]
        if _norows(B, p):
            assert dev1 == devN == cpuN == 0.0
            continue
        rel0 = abs(hist[0][1][p, F["merit"]] - cpu0) / cpu0
        rel1, ratio = abs(dev1 - cpu1) / cpu1, devN / cpuN
        dev_acc = [int(hist[k][1][p, F["accepted"]] - hist[k - 1][1][p, F["accepted"]]) for k in range(1, STEPS + 1)]
        lines.append("problem %2d %-10s seed %d: merit %.6e (rel %.1e) -> step 1 %.6e (rel %.1e) -> step %d %.6e, device / CPU %.4f; "
                     "accepted device %s CPU %s; mu0 device %.6e CPU %.6e"
                     % (p, *B.problems[p], cpu0, rel0, dev1, rel1, STEPS, devN, ratio, dev_acc, C["accepted"],
                        hist[0][1][p, F["mu"]], C["mu"][0]))
        if not (rel1 <= 1e-6 and 0.5 <= ratio <= 2.0):
            bad.append(p)
    print("\n".join(lines))
    assert not bad, bad


# ---------------------------------------------------------------- 5. bits

@groups
def test_bits_do_not_depend_on_the_batch_the_stream_or_the_graph(group):
    torch, device, st = torch_ctx()
    B, hist = _main(group)
    PROBLEMS = GROUPS[group]
    xA, rA = hist[-1]
    # the same problems at other places of another batch (some twice, the last one first), on another stream
    perm = list(range(B.P))[::-1][:B.P - 1] + [1, B.P - 1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        C = LmBatch([PROBLEMS[i] for i in perm])
        C.start(stream=side.cuda_stream)
        C.step(STEPS, stream=side.cuda_stream)
        xC, rC = C.read(stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    for q, i in enumerate(perm):
        assert same_bits(xC[C.xs(q)], xA[B.xs(i)]) and same_bits(rC[q], rA[i]), (q, i, rC[q], rA[i])
    # eager against captured-and-replayed steps, then the replay on a fresh x after a new start
    D = LmBatch(PROBLEMS)
    with torch.cuda.stream(side):   # warm-up outside the capture (module load)
        D.start(stream=side.cuda_stream)
        D.step(stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    D.start()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # two steps in one graph
        D.step(2, stream=torch.cuda.current_stream().cuda_stream)
    for _ in range(STEPS // 2):
        graph.replay()
    xD, rD = D.read()
    assert same_bits(xD, xA) and same_bits(rD, rA), "captured steps differ from eager ones"
    x1 = np.concatenate([lm_case(name)[0].x_perturbed(100 + seed) for name, seed in PROBLEMS])
    D.start(x_h=x1)
    for _ in range(2):
        graph.replay()
    xD1, rD1 = D.read()
    E = LmBatch(PROBLEMS)
    E.start(x_h=x1)
    E.step(4)
    xE, rE = E.read()
    assert same_bits(xD1, xE) and same_bits(rD1, rE), "the replay on a fresh x differs from eager steps"
    assert not same_bits(xD1, xA) and (rE[:, F["accepted"]] > 0).any()
    print("%s: %d problems at other places on another stream, 4 replays of a 2-step graph, 2 more on a fresh x: same bits" % (group, len(perm)))


# ---------------------------------------------------------------- 6. containment

HOSTILE = {"hopper": {1: "zero duration", 2: "lo > up", 4: "nan x"}, "biped": {2: "1e300 x", 3: "nan bound"}, "anymal": {1: "inf x"}}


@groups
def test_hostile_inputs_stay_in_their_problem(group):
    B, hist = _main(group)
    hostile = HOSTILE[group]
    x, lo, up = B.x0.copy(), B.lo_h.copy(), B.up_h.copy()
    late = []   # bad from the first linearisation on (the others: from the projection on)
    for p, what in hostile.items():
        k = int(B.xo[p]) + int(np.nonzero(lo[B.xs(p)] != up[B.xs(p)])[0][7])   # a variable that is not fixed
        if what == "nan x":
            x[k] = float("nan")
        elif what == "inf x":
            x[k] = float("-inf")
        elif what == "1e300 x":
            x[k] = 1e300
        elif what == "lo > up":
            lo[k], up[k] = 1.0, -1.0
        elif what == "nan bound":
            up[k] = float("nan")
        else:   # the first phase duration; outside a box, so that the projection cannot repair it
            case = lm_case(B.problems[p][0])[0]
            k = int(B.xo[p]) + [v for v in case.S.var_sets if v["name"].startswith("ee-schedule")][0]["offset"]
            x[k], lo[k], up[k] = 0.0, -1e20, 1e20
            late.append(p)
    H = LmBatch(GROUPS[group])
    got = H.run(x_h=x, lo_h=lo, up_h=up)
    for p in range(B.P):
        s = B.xs(p)
        if p not in hostile:
            for k in (0, 1, STEPS):
                assert same_bits(got[k][0][s], hist[k][0][s]) and same_bits(got[k][1][p], hist[k][1][p]), (p, k)
            continue
        assert got[-1][1][p, F["state"]] == ta.JacLm.BAD and got[1][1][p, F["state"]] == ta.JacLm.BAD, (p, hostile[p], got[-1][1][p])
        for k in range(1, STEPS + 1):
            assert same_bits(got[k][0][s], got[0][0][s]), (p, hostile[p], k, "x of a bad problem changed after the start")
        if p not in late:   # bad from the start: not even projected
            assert got[0][1][p, F["state"]] == ta.JacLm.BAD and same_bits(got[0][0][s], x[s]), (p, hostile[p])
        else:
            assert same_bits(got[0][0][s], np.clip(x[s], lo[s], up[s]))
        assert got[-1][1][p, F["steps"]] == 0 and got[-1][1][p, F["accepted"]] == 0


# ---------------------------------------------------------------- 7. done problems

@groups
def test_done_problems_are_frozen(group):
    B, hist = _main(group)
    feasible = [p for p in range(B.P) if _norows(B, p)]
    assert feasible or group != "biped"
    for p in feasible:   # the structure without rows starts feasible (merit 0)
        for k in range(STEPS + 1):
            x, rec = hist[k]
            assert rec[p, F["state"]] == ta.JacLm.DONE and rec[p, F["merit"]] == 0.0 and rec[p, F["steps"]] == 0
            assert same_bits(x[B.xs(p)], hist[0][0][B.xs(p)]) and same_bits(rec[p], hist[0][1][p])
    # every problem done at its first linearisation: nothing moves, whatever the solve and the trial do
    D = LmBatch(GROUPS[group], merit_done=1e300)
    got = D.run()
    assert (got[0][1][:, F["state"]] == ta.JacLm.DONE).all()
    for k in range(1, STEPS + 1):
        assert same_bits(got[k][0], got[0][0]) and same_bits(got[k][1], got[0][1]), k
    assert same_bits(got[0][0], hist[0][0]) and same_bits(got[0][1][:, F["mu"]], hist[0][1][:, F["mu"]])
    assert (got[0][1][:, F["merit"]] > 0).sum() == B.P - len(feasible)


# ---------------------------------------------------------------- 8. mismatched handles

def test_create_refuses_a_batch_of_another_layout():
    B, _ = _main("hopper")
    structs, order, _, _, _ = lm_inputs(GROUPS["hopper"][:5])
    other = ta.Batch(structs, order, device=0)
    with pytest.raises(ta.TowrError, match="layout"):
        ta.JacLm(other, B.lsq)
    swapped = ta.Batch(B.structs, B.order[::-1], device=0)
    with pytest.raises(ta.TowrError, match="layout"):
        ta.JacLm(swapped, B.lsq)
    with pytest.raises(ta.TowrError):
        ta.JacLm(B.batch, B.lsq, mu_min=2.0, mu_max=1.0)
    with pytest.raises(ta.TowrError):
        ta.JacLm(B.batch, B.lsq, cg_iters=-1)
    with pytest.raises(TypeError):
        ta.JacLm(B.batch, B.lsq, no_such_parameter=1)
    assert B.lm.bytes()["resident"] >= 8 * (7 * B.X + 5 * B.G + 16 * B.P)
