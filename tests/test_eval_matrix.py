"""Every row of the instantiation matrix (tests/eval_matrix.py) on the device, against the oracle.

Per row and per call -- every flag set, without and with per-kernel events (profile_begin(1)):
  - Batch.eval_plan on this device contains the instantiations the row claims for the call;
  - g and jac live inside larger allocations filled with a sentinel, 4096 doubles of guard on either side: afterwards no
    sentinel is left inside a requested output, every guard is intact, and an output that was not requested is untouched;
  - the outputs meet the parity bar of tests/common.py against OracleProblem.eval, at x_perturbed points (even problems) and
    x_wild points (odd problems): every problem of a cheap / wide row; of a chunk / nt row at least six (all, where the row has
    fewer), among them the first, the last and one of every distinct structure;
  - the fused plan (events off) and the separate launches (events on) write the same bits;
  - EVAL_BOTH of problem p is the bits its structure gives alone in a one-problem batch, which selects another NIT / XC / store
    variant (values only: parity, it is another algorithm).
Rows that claim scoring launches also run eval_scores_device / eval_score_best_device: the table against numpy on the oracle's g
and bounds exactly as tests/test_eval_scores.py does, index and total against towr_amd.dist.best_candidate.
Each test prints the worst error it saw as a fraction of the parity bar (run with -s)."""
import functools

import numpy as np
import pytest

import towr_amd as ta
from tests import eval_matrix
from tests.common import FLOOR, RTOL, assert_parity, linear_row_scale, row_scale, set_scale
from tests.test_eval_scores import _oracle_scores

pytestmark = pytest.mark.gpu

SENTINEL = 1.2345e300   # what the outputs hold before an evaluation
GUARD = 4096            # doubles before and after each output
POOL = 4                # distinct points per structure and kind
ROWS = eval_matrix.parse()[1]


def _kind(p):
    return "perturbed" if p % 2 == 0 else "wild"


@functools.lru_cache(maxsize=None)
def _x(name, kind, i):
    case = eval_matrix.make_case(name)
    return case.x_perturbed(i) if kind == "perturbed" else case.x_wild(i)


@functools.lru_cache(maxsize=None)
def _ref(name, kind, i):
    rg, _, _, rj = eval_matrix.make_case(name).P.eval(_x(name, kind, i))
    return rg, rj


class _Out:
    """One output array inside a larger allocation: guard | values | guard, all SENTINEL."""

    def __init__(self, n):
        import torch
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
        self.view = self.buf[GUARD:GUARD + n]

    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())

    def fully_written(self):
        return not bool((self.view == SENTINEL).any())


def _run(batch, d_x, flags, events, what):
    import torch
    g, j = _Out(int(batch.g_off[-1])), _Out(int(batch.jac_off[-1]))
    if events:
        batch.profile_begin(1)
    batch.eval_device(d_x.data_ptr(), g.ptr(), j.ptr(), flags, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if events:
        batch.profile_end()
    assert g.guards_intact(), what + ": a guard of g was written"
    assert j.guards_intact(), what + ": a guard of jac was written"
    if flags & ta.EVAL_VALUES:
        assert g.fully_written(), what + ": constraint values left unwritten"
    else:
        assert g.untouched(), what + ": g written although not requested"
    if flags & ta.EVAL_JACOBIAN:
        assert j.fully_written(), what + ": Jacobian values left unwritten"
    else:
        assert j.untouched(), what + ": jac written although not requested"
    return g.view, j.view


@functools.lru_cache(maxsize=None)
def _solo(name, kind, i):
    """EVAL_BOTH of one problem alone in a batch, as numpy."""
    import torch
    case = eval_matrix.make_case(name)
    batch = ta.Batch([case.S], [0], device=0)
    g, j = _run(batch, torch.from_numpy(_x(name, kind, i)).cuda(), ta.EVAL_BOTH, False, "%s alone" % name)
    return g.cpu().numpy(), j.cpu().numpy()


def _bar_fraction(S, got, ref, scale):
    tol = RTOL * np.abs(ref) + FLOOR * scale
    ok = tol > 0
    return float((np.abs(got - ref)[ok] / tol[ok]).max(initial=0.0))


def _sampled(row):
    n = len(row["order"])
    if row["kind"] in ("cheap", "wide") or n <= 6:
        return list(range(n))
    names = [row["structs"][s] for s in row["order"]]
    picks = [0, n - 1] + [names.index(nm) for nm in dict.fromkeys(names)]
    picks += [n // 3 | 1, (2 * n // 3) & ~1, n // 2 | 1]   # both kinds of point among them
    return sorted(set(picks))


def _same_bits(a, b):
    import torch
    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_row(row):
    import torch
    names = [row["structs"][s] for s in row["order"]]
    n = len(names)
    occurrence, seen = [], {}
    for nm in names:
        occurrence.append(seen.get(nm, 0) % POOL)
        seen[nm] = seen.get(nm, 0) + 1
    key = [(names[p], _kind(p), occurrence[p]) for p in range(n)]
    cases = [eval_matrix.make_case(nm) for nm in row["structs"]]
    batch = ta.Batch([c.S for c in cases], row["order"], device=0)
    assert batch.streaming_stores() == row["nt"], "the device's store policy is not the row's"
    d_x = torch.from_numpy(np.concatenate([_x(*k) for k in key])).cuda()
    sampled = _sampled(row)
    with_x = row["kind"] in ("cheap", "wide")   # (the scale of the linear sets needs x: a Python loop over their rows)
    worst = 0.0
    flag_sets = (ta.EVAL_BOTH, ta.EVAL_JACOBIAN) if row["kind"] == "nt" else (ta.EVAL_BOTH, ta.EVAL_JACOBIAN, ta.EVAL_VALUES)
    for flags in flag_sets:
        out = {}
        for events in (False, True):
            what = "%s flags %d events %d" % (row["name"], flags, events)
            planned = {s["instantiation"] for s in batch.eval_plan(flags, events)}
            missing = set(eval_matrix.claims_of(row, flags, events)) - planned
            assert not missing, "%s: the device plans %s, the row claims %s as well" % (what, sorted(planned), sorted(missing))
            out[events] = _run(batch, d_x, flags, events, what)
            for p in sampled:
                S = cases[row["order"][p]].S
                rg, rj = _ref(*key[p])
                x = _x(*key[p]) if with_x else None
                g = out[events][0][batch.g_off[p]:batch.g_off[p + 1]].cpu().numpy() if flags & ta.EVAL_VALUES else rg
                j = out[events][1][batch.jac_off[p]:batch.jac_off[p + 1]].cpu().numpy() if flags & ta.EVAL_JACOBIAN else rj
                gscale = set_scale(S.con_sets, rg)
                if x is not None:
                    gscale = np.maximum(gscale, linear_row_scale(S, rj, x))
                worst = max(worst, _bar_fraction(S, g, rg, gscale), _bar_fraction(S, j, rj, row_scale(S.row_ptr, rj)))
                assert_parity(S, g, j, rg, rj, "%s problem %d (%s, %s point)" % (what, p, key[p][0], key[p][1]), x=x)
                if flags == ta.EVAL_BOTH and not events:   # the same bits as the structure alone in a batch
                    sg, sj = _solo(*key[p])
                    assert np.array_equal(g.view(np.int64), sg.view(np.int64)), "%s problem %d: g differs from the one-problem batch" % (what, p)
                    assert np.array_equal(j.view(np.int64), sj.view(np.int64)), "%s problem %d: jac differs from the one-problem batch" % (what, p)
        if flags & ta.EVAL_VALUES:
            assert _same_bits(out[False][0], out[True][0]), "%s flags %d: g differs between the fused and the separate launches" % (row["name"], flags)
        if flags & ta.EVAL_JACOBIAN:
            assert _same_bits(out[False][1], out[True][1]), "%s flags %d: jac differs between the fused and the separate launches" % (row["name"], flags)
        del out
    if row["claims"]["scores"]:
        _check_scores(row, batch, cases, key, d_x)
    if row["kind"] in ("nt", "chunk"):   # (their points, references and one-problem results are large: not kept for the session)
        for cache in (_x, _ref, _solo, eval_matrix.make_case):
            cache.cache_clear()
    print("\n%s: %d problems, %d compared with the oracle, worst error %.3g of the parity bar" % (row["name"], n, len(sampled), worst))


def _check_scores(row, batch, cases, key, d_x):
    import torch
    from towr_amd.dist import best_candidate
    n, st = batch.n_problems, torch.cuda.current_stream().cuda_stream
    for request in ("scores", "score_best"):
        planned = {s["instantiation"] for s in batch.eval_plan(request=request)}
        claimed = set(row["claims"]["scores"]) | ({"best_kernel"} if request == "score_best" else set())
        assert claimed <= planned, "%s %s: the device plans %s" % (row["name"], request, sorted(planned))
    g = _Out(int(batch.g_off[-1]))
    scores = torch.full((n, 16), -1.0, dtype=torch.float64, device="cuda")
    batch.eval_scores_device(d_x.data_ptr(), scores.data_ptr(), d_g=0 if batch.scores_without_g else g.ptr(), stream=st)
    torch.cuda.synchronize()
    assert g.guards_intact() and (g.untouched() if batch.scores_without_g else g.fully_written())
    table = scores.cpu().numpy()
    for p in range(n):
        want = _oracle_scores(cases[row["order"][p]], _x(*key[p]))
        got = table[p].reshape(8, 2)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (row["name"], p, got, want)
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= 1e-9 * np.abs(want[ok]) + 1e-9), (row["name"], p, got, want)
    best = torch.zeros(2, dtype=torch.float64, device="cuda")
    again = torch.full((n, 16), -1.0, dtype=torch.float64, device="cuda")
    for fam, off in (((0, 1, 3, 4), 0), ((1, 4), 1000)):
        batch.eval_score_best_device(d_x.data_ptr(), again.data_ptr(), best.data_ptr(), families=fam, index_offset=off,
                                     d_g=0 if batch.scores_without_g else g.ptr(), stream=st)
        torch.cuda.synchronize()
        assert torch.equal(again, scores), "%s: the two scoring entry points give different tables" % row["name"]
        idx, total = best_candidate(again, families=fam)
        assert (int(best[0]), float(best[1])) == (off + idx, total), (row["name"], fam, best.cpu(), idx, total)
