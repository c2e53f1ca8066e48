"""Feet for the leg inverse-kinematics tests (tests/test_ik_ref.py, test_ik_probe.py, test_joints.py) and a numpy restatement of
the reference's formulas.  Deterministic: the only randomness is numpy's default_rng on fixed seeds.

Leg level: feet in the hip frame of the front-left leg, each taken with both knee bends, in classes
  interior      0.05 <= r <= 0.42, both law-of-cosines arguments within +-0.999, every angle at least 1e-3 rad inside its limits
  over_reach    r >= (lu + ll) (1 + 1e-6)
  stretch       r within 8 ulp of lu + ll, along four directions
  branch        y = +-0 with z > 0, z = +-0 with both signs of x, the eight signed (0, 0, 0), and feet whose HAA or HFE limit
                is enforced (KFE = gamma - pi lies in [-pi, 0] by construction: its limits are never enforced)
  non_finite    NaN / +Inf / -Inf in each coordinate
Whole body: four feet in the base frame (LF RF LH RH) around Go1's nominal stance, and a few far outside it."""
import functools

import numpy as np

LU = LL = 0.213
REACH = LU + LL
PI = float(np.pi)
Q_MIN = np.array([-180 / 180.0 * PI, -90 / 180.0 * PI, -180 / 180.0 * PI])
Q_MAX = np.array([90 / 180.0 * PI, 90 / 180.0 * PI, 0 / 180.0 * PI])
BASE_TO_HIP = np.array([0.1881, 0.04675 + 0.08, 0.0])
MIRROR = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [-1.0, 1.0, 1.0], [-1.0, -1.0, 1.0]])
KNEE_BEND = np.array([0, 0, 1, 1])
CLASSES = ("interior", "over_reach", "stretch", "branch", "non_finite")
N_INTERIOR = 2048


def ik_numpy(p, bend):
    """GetJointAngles + EnforceLimits (go1leg_inverse_kinematics.cc:16-115) on feet p[n, 3] in the hip frame with knee bends
    bend[n], in numpy doubles, operation for operation: returns q[n, 3], flags[n], cos_beta, cos_gamma, r.  flags as the
    device's: 1 / 2 the HFE / KFE cosine lay outside [-1, 1] (a NaN counts), 4 / 8 / 16 a limit was enforced, 32 a NaN angle."""
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    bend = np.broadcast_to(np.asarray(bend), (len(p),))
    with np.errstate(all="ignore"):
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        q_haa = -np.arctan2(y, -z)
        c, s = np.cos(q_haa), np.sin(q_haa)
        xr0 = 1.0 * x + 0.0 * y + 0.0 * z
        xr2 = 0.0 * x + s * y + c * z
        xr0, xr2 = xr0 + 0.0, xr2 + 0.0
        sq = xr0 * xr0 + xr2 * xr2
        alpha = np.where(bend == 0, np.arctan2(-xr2, xr0), np.arctan2(-xr2, -xr0)) - 0.5 * PI
        r = np.sqrt(sq)
        cb = (LU * LU + sq - LL * LL) / (2. * LU * r)
        cg = (LL * LL + LU * LU - sq) / (2. * LL * LU)

        def clamp(v):      # std::max(-1, std::min(1, v)): a NaN becomes +1
            m = np.where(v < 1.0, v, 1.0)
            return np.where(-1.0 < m, m, -1.0)

        q_hfe = alpha + np.arccos(clamp(cb))
        q_kfe = np.arccos(clamp(cg)) - PI
        flags = np.where(~((-1.0 <= cb) & (cb <= 1.0)), 1, 0) | np.where(~((-1.0 <= cg) & (cg <= 1.0)), 2, 0)
        q = np.column_stack([q_haa, q_hfe, q_kfe])
        for j, bit in enumerate((4, 8, 16)):
            over = q[:, j] > Q_MAX[j]
            q[:, j] = np.where(over, Q_MAX[j], q[:, j])
            under = q[:, j] < Q_MIN[j]
            q[:, j] = np.where(under, Q_MIN[j], q[:, j])
            flags = flags | np.where(over | under, bit, 0)
        flags = flags | np.where(np.isnan(q).any(axis=1), 32, 0)
    return q, flags.astype(np.int64), cb, cg, r


def body_to_hip(feet_b):
    """GetAllJointAngles' mirroring (inverse_kinematics_go1.cc:23-42): feet_b[n, 4, 3] in the base frame -> hip-frame feet"""
    return np.asarray(feet_b, dtype=np.float64).reshape(-1, 4, 3) * MIRROR[None] - BASE_TO_HIP[None, None]


def fk(q, bend=None):
    """the foot of joint angles q[n, 3] in the hip frame: the inverse of ik_numpy on its interior (HAA about x, HFE and KFE about y)"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    # in the HFE frame the thigh points down at angle q_hfe from -z, the shank at q_hfe + q_kfe
    xh = -LU * np.sin(q[:, 1]) - LL * np.sin(q[:, 1] + q[:, 2])
    zh = -LU * np.cos(q[:, 1]) - LL * np.cos(q[:, 1] + q[:, 2])
    if bend is not None:
        xh = np.where(np.asarray(bend) == 0, xh, -xh)
    c, s = np.cos(q[:, 0]), np.sin(q[:, 0])
    # xr = R p with R = Rx(q_haa): p = R^T xr, xr = (xh, 0, zh)
    return np.column_stack([xh, s * zh, c * zh])


def _ulp_steps(v, k):
    out = np.float64(v)
    for _ in range(abs(k)):
        out = np.nextafter(out, np.inf if k > 0 else -np.inf)
    return float(out)


@functools.lru_cache(maxsize=None)
def leg_families():
    """{class: feet[n, 3]}, each foot to be taken with both bends"""
    rng = np.random.default_rng(20240607)
    fam = {}
    pts = []
    while len(pts) < N_INTERIOR:
        r = rng.uniform(0.05, 0.42, size=4096)
        th = rng.uniform(-1.4, 1.4, size=4096)
        ph = rng.uniform(-1.3, 1.3, size=4096)
        p = np.column_stack([r * np.sin(th), r * np.cos(th) * np.sin(ph), -r * np.cos(th) * np.cos(ph)])
        ok = np.ones(len(p), dtype=bool)
        for bend in (0, 1):
            q, fl, cb, cg, rr = ik_numpy(p, bend)
            margin = np.minimum(q - Q_MIN, Q_MAX - q).min(axis=1)
            ok &= (fl == 0) & (rr >= 0.05) & (rr <= 0.42) & (np.abs(cb) <= 0.999) & (np.abs(cg) <= 0.999) & (margin >= 1e-3)
        pts.extend(p[ok])
    fam["interior"] = np.array(pts[:N_INTERIOR])
    r = rng.uniform(REACH * (1 + 1e-6), 1.0, size=255)
    th, ph = rng.uniform(-1.4, 1.4, size=255), rng.uniform(-1.3, 1.3, size=255)
    fam["over_reach"] = np.vstack([[0.0, 0.0, -0.5], np.column_stack([r * np.sin(th), r * np.cos(th) * np.sin(ph), -r * np.cos(th) * np.cos(ph)])])
    st = []
    for k in range(-8, 9):
        a = _ulp_steps(REACH, k)
        st += [[0.0, 0.0, -a], [a * 0.6, 0.0, -a * 0.8], [-a * 0.6, 0.0, -a * 0.8], [0.0, a * 0.6, -a * 0.8], [a * 0.28, a * 0.0, -a * 0.96]]
    fam["stretch"] = np.array(st)
    br = []
    for y in (0.0, -0.0):
        for x in (0.0, 0.1, -0.1, -0.0):
            br.append([x, y, 0.3])
    for z in (0.0, -0.0):
        for x in (0.3, -0.3):
            for y in (0.0, -0.0, 0.1, -0.1):
                br.append([x, y, z])
    for sx in (0.0, -0.0):
        for sy in (0.0, -0.0):
            for sz in (0.0, -0.0):
                br.append([sx, sy, sz])
    br += [[0.0, 0.0, -0.3], [-0.0, 0.0, -0.3], [0.0, -0.0, -0.3]]                      # HAA = -+0
    br += [[0.1, -0.2, 0.1], [0.0, -0.3, 0.05], [-0.1, -0.05, 0.2], [0.05, -1e-3, 0.3]]   # HAA beyond +90 deg
    br += [[-0.3, 0.0, -0.1], [-0.25, 0.05, -0.05], [0.3, 0.0, -0.1], [0.25, -0.05, -0.05], [-0.35, 0.1, -0.02], [0.35, 0.1, -0.02]]   # HFE beyond +90 deg for one bend each
    fam["branch"] = np.array(br)
    nf = []
    base = [0.05, 0.02, -0.3]
    for d in range(3):
        for v in (np.nan, np.inf, -np.inf):
            p = list(base)
            p[d] = v
            nf.append(p)
    nf += [[np.nan, np.nan, np.nan], [np.inf, -np.inf, 0.0], [np.nan, 0.0, -0.3]]
    fam["non_finite"] = np.array(nf)
    for v in fam.values():
        v.flags.writeable = False
    return fam


@functools.lru_cache(maxsize=None)
def leg_points():
    """(feet[n, 3], bend[n], {class: slice}): every family with bend 0, then with bend 1"""
    fam = leg_families()
    feet, bends, sl, at = [], [], {}, 0
    for name in CLASSES:
        n = len(fam[name])
        feet += [fam[name], fam[name]]
        bends += [np.zeros(n), np.ones(n)]
        sl[name] = slice(at, at + 2 * n)
        at += 2 * n
    feet, bends = np.vstack(feet), np.concatenate(bends)
    feet.flags.writeable = False
    bends.flags.writeable = False
    return feet, bends, sl


@functools.lru_cache(maxsize=None)
def body_points():
    """feet[n, 4, 3] in the base frame: 256 around the nominal stance (every leg interior), 16 far outside it"""
    rng = np.random.default_rng(977)
    nominal = np.array([[0.1881, 0.12675, -0.3], [0.1881, -0.12675, -0.3], [-0.1881, 0.12675, -0.3], [-0.1881, -0.12675, -0.3]])
    near = nominal[None] + rng.uniform(-0.08, 0.08, size=(256, 4, 3))
    far = nominal[None] + rng.uniform(-0.6, 0.6, size=(16, 4, 3))
    out = np.vstack([near, far])
    out.flags.writeable = False
    return out


N_BODY_NEAR = 256
