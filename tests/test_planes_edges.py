"""twr_batch_contact_planes through the C ABI on the scenes of tests/plane_points.py: the footholds of a hand-written plan
buffer are the query points, so that plane_kernel meets every polygon boundary, tie and special value that
tests/test_plane_probe.py puts to the device functions alone -- and its own guards: the contact flag, counts, the thread total,
what lies behind the index buffer.

One four-legged batch of 3 problems is shared; a scene's points are dealt to the problems in thirds, four feet per footstep
state, one contact_planes_device call per scene.  The expected indices are the recorded ones of tests/golden/refplane.npz."""
import functools

import numpy as np
import pytest

import towr_amd as ta

from . import plane_points as pp
from .probe import bits
from .test_plane_probe import scene_refs

N_EE, N_PROBLEMS = 4, 3
REC = 2 + 4 * N_EE
SENTINEL, GUARD = -7, 256
CLOSED_SCENES = ("argmin/one", "argmin/two", "argmin/many33", "argmin/nested_outer_first", "argmin/tie")


@functools.lru_cache(maxsize=None)
def _batch():
    S = ta.Structure(ta.model_preset("anymal", "flat"), ta.gait_combo(4, 1, 2.0))
    return ta.Batch([S], [0] * N_PROBLEMS, device=0)


def plan_of(points, max_steps=None, flag=1.0):
    """(plan (3, max_steps, REC), counts (3,), where (n, 3) = problem, state, foot of every point): the points dealt to the problems
    in thirds, four per state; the feet left over are in the air (flag 0) at a position inside every scene"""
    n = len(points)
    third = -(-n // N_PROBLEMS)
    steps = max(1, -(-third // N_EE))
    max_steps = steps if max_steps is None else max_steps
    assert max_steps >= steps
    plan = np.zeros((N_PROBLEMS, max_steps, REC))
    where = np.zeros((n, 3), dtype=np.int64)
    for i, (x, y) in enumerate(points):
        p, k = divmod(i, third)
        s, e = divmod(k, N_EE)
        where[i] = (p, s, e)
        plan[p, s, 2 + e] = flag
        plan[p, s, 2 + N_EE + 3 * e:2 + N_EE + 3 * e + 3] = (x, y, 0.25)
    return plan, np.full(N_PROBLEMS, max_steps, dtype=np.int32), where


def lookup(planes, plan, counts):
    """one twr_batch_contact_planes call: (indices (3, max_steps, 4), the guard region behind them)"""
    import torch
    dev = torch.device("cuda", 0)
    max_steps = plan.shape[1]
    total = N_PROBLEMS * max_steps * N_EE
    d_plan = torch.from_numpy(np.ascontiguousarray(plan)).to(dev)
    d_counts = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(dev)
    idx = torch.full((total + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    _batch().contact_planes_device(planes, d_plan.data_ptr(), d_counts.data_ptr(), max_steps, idx.data_ptr(), 0)
    torch.cuda.synchronize()
    h = idx.cpu().numpy()
    return h[:total].reshape(N_PROBLEMS, max_steps, N_EE), h[total:]


def _check_scene(k, planes):
    s, (_, index, _) = pp.scenes()[k], scene_refs()[k]
    plan, counts, where = plan_of(s["points"])
    got, guard = lookup(planes, plan, counts)
    mine = got[where[:, 0], where[:, 1], where[:, 2]]
    bad = np.nonzero(mine != index)[0]
    assert len(bad) == 0, (s["name"], [(tuple(s["points"][i]), mine[i], index[i]) for i in bad[:5]])
    rest = np.ones(got.shape, dtype=bool)
    rest[where[:, 0], where[:, 1], where[:, 2]] = False
    assert (got[rest] == -1).all() and (guard == SENTINEL).all(), s["name"]
    return len(index)


@pytest.mark.gpu
def test_identity_scenes_through_the_c_abi():
    """every scene of identity regions (the empty ring, which twr_planes_create refuses, left out): Planes.world_xy is the input bit
    for bit, and every foothold gets the recorded index -- vertices, edges, verticals, ulp neighbours, ties, collapse pairs and
    the NaN / Inf / 1e300 footholds between ordinary ones"""
    n = 0
    for k, s in enumerate(pp.scenes()):
        if not pp.is_identity(s) or any(len(r) == 0 for r in s["rings"]):
            continue
        planes = ta.Planes(s["regions"], s["rings"], device=0)
        if s["rings"]:
            assert np.array_equal(bits(planes.world_xy), bits(np.concatenate(s["rings"]))), s["name"]
        n += _check_scene(k, planes)
    print("\ncontact planes: %d footholds of identity scenes equal the reference" % n)
    assert n > 15000


@pytest.mark.gpu
def test_rotated_scenes_through_the_c_abi():
    """regions with random, non-unit, identity and half-turn quaternions at non-zero positions: Planes.world_xy is the recorded
    output of the reference's tf transform bit for bit, and the indices are the recorded ones"""
    ks = [k for k, s in enumerate(pp.scenes()) if not pp.is_identity(s)]
    assert len(ks) >= 2
    for k in ks:
        s, (world, _, _) = pp.scenes()[k], scene_refs()[k]
        planes = ta.Planes(s["regions"], s["rings"], device=0)
        assert np.array_equal(bits(planes.world_xy), bits(np.concatenate(world))), s["name"]
        assert not np.array_equal(planes.world_xy, np.concatenate(s["rings"]))
        _check_scene(k, planes)


def test_special_footholds_are_minus_one_in_the_reference():
    """(CPU tier) over closed polygons the recorded index of every NaN / Inf / 1e300 foothold is -1, though polygons exist"""
    for name in CLOSED_SCENES:
        k = [i for i, s in enumerate(pp.scenes()) if s["name"] == name][0]
        special = pp.scenes()[k]["kind"] == pp.POINT_SPECIAL
        assert special.sum() >= 2 and (scene_refs()[k][1][special] == -1).all(), name
        assert (scene_refs()[k][1][~special] >= 0).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps", [50, 64])
def test_flags_counts_totals_and_guard(max_steps):
    """one scene, 12 * max_steps threads (600: no multiple of 256; 768: one): a contact flag of 0.0 and of -0.0 gives -1; states at
    or beyond counts[p] give -1 with counts of 0, of exactly max_steps and of more than max_steps; the sentinel behind the index
    buffer stays; a repeated call gives the same bits; the special footholds leave their neighbours alone"""
    k = [i for i, s in enumerate(pp.scenes()) if s["name"] == "argmin/two"][0]
    s, (_, index, _) = pp.scenes()[k], scene_refs()[k]
    planes = ta.Planes(s["regions"], s["rings"], device=0)
    plan, counts, where = plan_of(s["points"], max_steps)
    assert (N_PROBLEMS * max_steps * N_EE) % 256 == (0 if max_steps == 64 else 88)
    p_, s_, e_ = where[:, 0], where[:, 1], where[:, 2]
    full, guard = lookup(planes, plan, counts)
    assert np.array_equal(full[p_, s_, e_], index) and (guard == SENTINEL).all()
    special = s["kind"] == pp.POINT_SPECIAL
    assert (full[p_, s_, e_][special] == -1).all() and (full[p_, s_, e_][~special] >= 0).all()
    again, _ = lookup(planes, plan, counts)
    assert np.array_equal(full, again)
    # contact flags: every third foothold 0.0, the next -0.0
    flagged = plan.copy()
    off = np.arange(len(where)) % 3
    flagged[p_[off == 1], s_[off == 1], 2 + e_[off == 1]] = 0.0
    flagged[p_[off == 2], s_[off == 2], 2 + e_[off == 2]] = -0.0
    got, guard = lookup(planes, flagged, counts)
    assert np.array_equal(got[p_, s_, e_], np.where(off == 0, index, -1)) and (guard == SENTINEL).all()
    # counts: problem 0 none, problem 1 exactly max_steps, problem 2 more than max_steps; then a cut in the middle
    for c in ([0, max_steps, max_steps + 5], [3, 0, 1 << 30], [max_steps - 1, 1, 2]):
        got, guard = lookup(planes, plan, np.array(c, dtype=np.int32))
        want = np.where(s_ < np.array(c)[p_], index, -1)
        assert np.array_equal(got[p_, s_, e_], want), c
        live = np.arange(max_steps)[None, :, None] < np.array(c)[:, None, None]
        assert (got[~np.broadcast_to(live, got.shape)] == -1).all() and (guard == SENTINEL).all(), c
