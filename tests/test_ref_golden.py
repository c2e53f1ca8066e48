"""tests/golden/ref_*.npz are recorded outputs of the reference's OWN code (oracle/ref_golden.py, run where the reference
sources are): per case the description, the Jacobian pattern, constraint and variable bounds, the set tables and, for
several x, g and the Jacobian values.  They carry the reference to boxes that do not have it.

CPU tier: the oracle and ta.Structure against every fixture -- set tables, pattern, bounds, variable bounds, g and
Jacobian through assert_parity with the fixture as `ref`, every entry -- plus negative controls on the comparison.
GPU tier: the device against every fixture, EVERY entry, no allow-list (the force-row x foothold entries that the mpmath
fixtures cannot speak about included); the expected values come from tests/golden/ only, never from the oracle.
The bar is the project's (tests/common.py): 1e-9 |ref| + 1e-12 scale."""
import glob
import os

import numpy as np
import pytest

import towr_amd as ta
from oracle import ref_run

from .common import Case, assert_parity, row_scale, set_scale

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "ref_*.npz")))
IDS = [os.path.basename(p)[4:-4] for p in FIXTURES]
FIELDS = ref_run.PARAM_KEYS   # the order of the fixtures' "params" array


class Fixture:
    def __init__(self, path):
        d = np.load(path)
        self.name = os.path.basename(path)[4:-4]
        self.d = {k: d[k] for k in d.files}
        durs, o = [], 0
        for k in d["n_phases"]:
            durs.append(d["phase_durations"][o:o + k])
            o += k
        params = dict(zip(FIELDS, d["params"]))
        for k in ("polys_per_swing", "polys_per_stance_force"):
            params[k] = int(params[k])
        if params["base_z_init"] != params["base_z_init"]:
            del params["base_z_init"]
        grid = d["csv_heights"] if "csv_heights" in d.files else None
        self._case_args = (str(d["robot"]), str(d["terrain"]), ta.schedule(durs, list(d["contact_at_start"])))
        self._case_kw = dict(grid=grid, constraint_sets=int(d["constraint_sets"]), **params)
        self._case = None
        # the structure alone (what the GPU tier needs: the oracle stays out of that path); `case` adds the oracle
        self.grid = ta.TerrainGrid(grid) if grid is not None else None
        self.S = ta.Structure(ta.model_preset(*self._case_args[:2]), self._case_args[2], ta.params_default(**self._case_kw_params()),
                              grid=self.grid)
        self.x, self.g, self.jac = d["x"], d["g"], d["jac_val"]
        self.row_ptr = np.concatenate([[0], np.cumsum(np.bincount(d["jac_row"], minlength=self.g.shape[1]))]).astype(np.int32)

    def _case_kw_params(self):
        return {k: v for k, v in self._case_kw.items() if k != "grid"}

    @property
    def case(self):
        """tests.common.Case of the fixture's problem: structure + oracle (CPU tier)"""
        if self._case is None:
            self._case = Case(*self._case_args, **self._case_kw)
        return self._case

    def check_structure(self, what):
        """set tables, pattern and bounds of the structure builder against the fixture"""
        S, d = self.S, self.d
        assert (S.n, S.m, S.nnz) == (self.x.shape[1], self.g.shape[1], self.jac.shape[1]), what
        assert [s["name"] for s in S.con_sets] == list(d["con_names"]) and [s["size"] for s in S.con_sets] == list(d["con_rows"]), what
        assert [s["name"] for s in S.var_sets] == list(d["var_names"]) and [s["size"] for s in S.var_sets] == list(d["var_rows"]), what
        assert np.array_equal(S.row_ptr, self.row_ptr) and np.array_equal(S.col_idx, d["jac_col"]), what + ": pattern"
        assert np.all(np.diff(d["jac_row"]) >= 0), what

    def compare(self, k, got_g, got_j, what):
        """g and the Jacobian values at the fixture's k-th x against the fixture, every entry"""
        assert_parity(self.S, got_g, got_j, self.g[k], self.jac[k], "%s x[%d] %s" % (self.name, k, what), x=self.x[k])

    def worst(self, k, got_g, got_j):
        S = self.S
        gs = np.maximum(set_scale(S.con_sets, self.g[k]), 1e-300)
        js = np.maximum(row_scale(S.row_ptr, self.jac[k]), 1e-300)
        return float((np.abs(got_g - self.g[k]) / gs).max()), float((np.abs(got_j - self.jac[k]) / js).max())


def _close(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= 1e-9 * np.abs(b) + 1e-12))


def test_the_fixture_set_is_complete_and_within_budget():
    """What the fixtures are there for (every robot, every terrain with curvature, every constraint family, optimised
    timings, the odd schedules, the BASELINE sizes) -- and the size budget: no file above the largest mpmath fixture, all
    of them together no more than the mpmath fixtures."""
    assert len(FIXTURES) >= 30
    mp = [os.path.getsize(p) for p in glob.glob(os.path.join(HERE, "golden", "mp_*.npz"))]
    sizes = [os.path.getsize(p) for p in FIXTURES]
    assert max(sizes) <= max(mp) and sum(sizes) <= sum(mp) and max(sizes) <= 1 << 20, (max(sizes), sum(sizes))
    robots, terrains, families, masks, phases = set(), set(), set(), set(), set()
    for p in FIXTURES:
        d = np.load(p)
        robots.add(str(d["robot"])), terrains.add(str(d["terrain"])), masks.add(int(d["constraint_sets"])), phases.update(int(v) for v in d["n_phases"])
        families.update(str(n).split("-")[0] for n in d["con_names"])
    assert robots == {"monoped", "biped", "hyq", "anymal", "go1"}
    assert terrains >= {"flat", "block", "stairs", "gap", "slope", "chimney", "chimney_lr", "csv"}
    assert families == {"terrain", "dynamic", "splineacc", "rangeofmotion", "force", "swing", "totalduration", "baseMotion"}
    assert {63, 127, 255} <= masks and {1, 31} <= phases


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_oracle_and_structure_match_the_reference_fixture(path):
    fx = Fixture(path)
    case, d = fx.case, fx.d
    fx.check_structure(fx.name)
    S, P = case.S, case.P
    assert list(P.con_sets) == list(zip(d["con_names"], d["con_rows"])) and list(P.var_sets) == list(zip(d["var_names"], d["var_rows"]))
    lin0, lin1, ee0 = ref_run.formulation_states(case)
    init, final = np.zeros(12), np.zeros(12)
    init[:3], final[:3] = lin0, lin1
    for who in (S, P):
        lo, up = who.bounds()
        assert _close(lo, d["g_bounds"][0]) and _close(up, d["g_bounds"][1]), fx.name + ": constraint bounds"
        lo, up = who.variable_bounds(init, final, ee0)
        assert _close(lo, d["x_bounds"][0]) and _close(up, d["x_bounds"][1]), fx.name + ": variable bounds"
    for k in range(len(fx.x)):
        og, rp, ci, ov = P.eval(fx.x[k])
        assert np.array_equal(rp, fx.row_ptr) and np.array_equal(ci, d["jac_col"]), fx.name + ": oracle pattern"
        fx.compare(k, og, ov, "oracle")


def _quirk_entries(fx):
    """positions (in the fixture's value array) of the force-row x foothold-column entries"""
    S = fx.case.S
    rows = np.repeat(np.arange(S.m), np.diff(S.row_ptr))
    force = np.zeros(S.m, dtype=bool)
    for s in S.con_sets:
        if s["name"].startswith("force-"):
            force[s["offset"]:s["offset"] + s["size"]] = True
    motion = np.zeros(S.n, dtype=bool)
    for v in S.var_sets:
        if v["name"].startswith("ee-motion"):
            motion[v["offset"]:v["offset"] + v["size"]] = True
    return np.nonzero(force[rows] & motion[S.col_idx])[0], rows


def test_negative_controls_on_the_comparison():
    """The comparison must see what it is there to see.  On a copy of ref_quirk_gap (x[0] is the x of
    mp_full_anymal_trot_gap): (a) one non-zero scaled by 1 + 1e-8, (b) one explicit zero set to 1e-9 x its row scale,
    (c) one quirk entry replaced by the mpmath chain-rule value of the same entry -- each must be reported."""
    fx = Fixture(os.path.join(HERE, "golden", "ref_quirk_gap.npz"))
    assert str(fx.d["x_family"][0]).startswith("mp_full_anymal_trot_gap")
    S, P = fx.case.S, fx.case.P
    og, _, _, ov = P.eval(fx.x[0])
    fx.compare(0, og, ov, "untouched")
    quirk, rows = _quirk_entries(fx)
    scale = row_scale(S.row_ptr, fx.jac[0])
    truth = fx.jac[0].copy()

    def reported(k, value):
        fx.jac[0] = truth.copy()
        fx.jac[0][k] = value
        try:
            fx.compare(0, og, ov, "tampered")
        except AssertionError as e:
            return "Jacobian values off" in str(e)
        finally:
            fx.jac[0] = truth.copy()
        return False

    big = int(np.argmax(np.abs(truth) == scale))           # an entry that is the largest of its row
    assert truth[big] != 0 and reported(big, truth[big] * (1 + 1e-8)), "(a) a relative error of 1e-8 went unnoticed"
    zeros = np.nonzero((truth == 0) & (scale > 0))[0]
    assert zeros.size, "the fixture should hold explicit zeros in non-empty rows"
    assert reported(int(zeros[0]), 1e-9 * scale[zeros[0]]), "(b) an explicit zero that became 1e-9 of its row scale went unnoticed"
    # (c) the same problem with towr's default sets is what mp_full_anymal_trot_gap holds: map its force rows onto this
    # fixture's rows through the set tables, and take the quirk entry where chain rule and reference differ most
    mp = np.load(os.path.join(HERE, "golden", "mp_full_anymal_trot_gap.npz"))
    assert np.array_equal(mp["x"], fx.x[0])
    from oracle import binding as ob

    durs = fx.case.sched.durations()
    full = ob.OracleProblem("anymal", "gap", durs, fx.case.sched.contact(), constraint_sets=int(mp["constraint_sets"]))
    full_off, o = {}, 0
    for name, n in full.con_sets:
        full_off[name] = o
        o += n
    to_full = np.zeros(S.m, dtype=int)
    for s in S.con_sets:
        to_full[s["offset"]:s["offset"] + s["size"]] = full_off[s["name"]] + np.arange(s["size"])
    chain = {(int(r), int(c)): v for r, c, v in zip(mp["jac_row"], mp["jac_col"], mp["jac_val"])}
    cr = np.array([chain.get((int(to_full[rows[k]]), int(S.col_idx[k])), 0.0) for k in quirk])
    diff = np.abs(cr - truth[quirk])
    k = int(quirk[np.argmax(diff)])
    assert diff.max() > 1e-6 * scale[k], "the chain-rule value and the reference's should differ on the Gap"
    assert reported(k, cr[np.argmax(diff)]), "(c) a quirk entry replaced by its chain-rule value went unnoticed"
    # and the other way round: the non-quirk entries of the force rows agree with mpmath at the project's bar
    rest = np.setdiff1d(np.nonzero(np.isin(rows, np.unique(rows[quirk])))[0], quirk)
    cr_rest = np.array([chain.get((int(to_full[rows[k]]), int(S.col_idx[k])), 0.0) for k in rest])
    assert np.all(np.abs(cr_rest - truth[rest]) <= 1e-9 * np.abs(truth[rest]) + 1e-12 * scale[rest])


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def _groups():
    """the fixtures by number of feet: {n_ee: [Fixture]}"""
    out = {}
    for p in FIXTURES:
        fx = Fixture(p)
        out.setdefault(fx.S.n_ee, []).append(fx)
    return out


def _problems(fxs):
    """one problem per (fixture, x): (structure index, fixture, k)"""
    return [(i, fx, k) for i, fx in enumerate(fxs) for k in range(len(fx.x))]


def _eval_nan_prefilled(batch, x_host, flags):
    import torch

    x = torch.from_numpy(x_host).cuda()
    g = torch.full((int(batch.g_off[-1]),), float("nan"), dtype=torch.float64, device="cuda")
    j = torch.full((int(batch.jac_off[-1]),), float("nan"), dtype=torch.float64, device="cuda")
    batch.eval_device(x.data_ptr(), g.data_ptr(), j.data_ptr(), flags, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return g.cpu().numpy(), j.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n_ee", [1, 2, 4])
def test_device_matches_the_reference_fixtures(n_ee):
    """All fixture problems with the same number of feet in one ragged batch, NaN-prefilled outputs: EVAL_BOTH, then
    EVAL_VALUES and EVAL_JACOBIAN alone (other instruction sequences), every problem and every x against the fixture,
    every entry."""
    fxs = _groups()[n_ee]
    for fx in fxs:
        fx.check_structure(fx.name)
    probs = _problems(fxs)
    batch = ta.Batch([fx.S for fx in fxs], [i for i, _, _ in probs], device=0)
    x = np.concatenate([fx.x[k] for _, fx, k in probs])
    worst = [0.0, 0.0]
    for flags, what in ((ta.EVAL_BOTH, "both"), (ta.EVAL_VALUES, "values alone"), (ta.EVAL_JACOBIAN, "Jacobian alone")):
        g, j = _eval_nan_prefilled(batch, x, flags)
        if not flags & ta.EVAL_VALUES:
            assert np.isnan(g).all(), "EVAL_JACOBIAN wrote g"
        if not flags & ta.EVAL_JACOBIAN:
            assert np.isnan(j).all(), "EVAL_VALUES wrote the Jacobian"
        for p, (_, fx, k) in enumerate(probs):
            gd = g[batch.g_off[p]:batch.g_off[p + 1]] if flags & ta.EVAL_VALUES else fx.g[k]
            jd = j[batch.jac_off[p]:batch.jac_off[p + 1]] if flags & ta.EVAL_JACOBIAN else fx.jac[k]
            fx.compare(k, gd, jd, "device, " + what)
            eg, ej = fx.worst(k, gd, jd)
            worst = [max(worst[0], eg), max(worst[1], ej)]
    print("n_ee %d: %d problems of %d fixtures, device vs reference worst error / scale: g %.3e, Jacobian %.3e" % (n_ee, len(probs), len(fxs), *worst))


@pytest.mark.gpu
@pytest.mark.parametrize("n_ee", [1, 2, 4])
def test_device_matches_the_reference_fixtures_in_a_large_batch(n_ee):
    """The same problems tiled to a batch of >= 2048, where the terrain / force / splineacc / swing rows go through the
    persistent node_chunk_kernel: the first and the last tile against the fixtures, every other tile bit-equal to the
    first (same problems, same x)."""
    fxs = _groups()[n_ee]
    probs = _problems(fxs)
    tiles = -(-2048 // len(probs))
    batch = ta.Batch([fx.S for fx in fxs], [i for i, _, _ in probs] * tiles, device=0)
    assert batch.n_problems >= 2048
    x = np.tile(np.concatenate([fx.x[k] for _, fx, k in probs]), tiles)
    g, j = _eval_nan_prefilled(batch, x, ta.EVAL_BOTH)
    assert not np.isnan(g).any() and not np.isnan(j).any()
    n = len(probs)
    for t in (0, tiles - 1):
        for q, (_, fx, k) in enumerate(probs):
            p = t * n + q
            fx.compare(k, g[batch.g_off[p]:batch.g_off[p + 1]], j[batch.jac_off[p]:batch.jac_off[p + 1]], "device, tile %d of %d" % (t, tiles))
    gt, jt = g.reshape(tiles, -1), j.reshape(tiles, -1)
    assert np.array_equal(gt, np.broadcast_to(gt[0], gt.shape)) and np.array_equal(jt, np.broadcast_to(jt[0], jt.shape))


@pytest.mark.gpu
def test_device_scores_without_g_match_the_reference_fixtures():
    """twr_batch_eval_scores on the values-only path (fixed timings, no g written) against the bound violations computed on
    the host from the fixture's g and the fixture's bounds, per constraint family: inf-norm and 1-norm at the bar of
    test_eval_scores.test_oracle_parity_without_g (1e-9 relative + 1e-9)."""
    import torch

    checked = 0
    for n_ee, group in sorted(_groups().items()):   # (all structures of a batch share the number of feet)
        fxs = [fx for fx in group if not int(fx.d["constraint_sets"]) & 64 and fx.S.n <= 2046]
        probs = _problems(fxs)
        batch = ta.Batch([fx.S for fx in fxs], [i for i, _, _ in probs], device=0)
        assert batch.scores_without_g
        x = torch.from_numpy(np.concatenate([fx.x[k] for _, fx, k in probs])).cuda()
        got = torch.full((len(probs), 16), -1.0, dtype=torch.float64, device="cuda")
        batch.eval_scores_device(x.data_ptr(), got.data_ptr(), d_g=0, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for p, (_, fx, k) in enumerate(probs):
            lo, up = fx.d["g_bounds"]
            viol = np.maximum(np.maximum(lo - fx.g[k], fx.g[k] - up), 0.0)
            want = np.zeros((8, 2))
            for cs in fx.S.con_sets:
                fam = [i for i, f in enumerate(ta.FAMILIES) if cs["name"].startswith(f)][0]
                v = viol[cs["offset"]:cs["offset"] + cs["size"]]
                want[fam, 0] = max(want[fam, 0], v.max(initial=0.0))
                want[fam, 1] += v.sum()
            s = got[p].reshape(8, 2)
            assert np.all(np.abs(s - want) <= 1e-9 * np.abs(want) + 1e-9), (fx.name, k, s, want)
            checked += 1
    assert checked >= 25
