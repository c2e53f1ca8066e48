"""The check record of twr_batch_checks restated in numpy, in the order of operations that towr_amd/csrc/kernels/checks.h states
(the kernels contract nothing, so plainly rounded doubles in the same order are the same bits), the fold of
twr_batch_check_scores, and what the tests of both share.  Needs no GPU.

Record in:   [ t | base p v a | q wxyz | omega | omega_dot | per ee: contact, p v a, f ]          20 + 13 n_ee
Record out:  [ t | angular residual 3 | linear residual 3 | per ee: contact, clearance, f_n, cone, rom ]   7 + 5 n_ee"""
import numpy as np

from .test_joints import frame_rotation, frame_vector

HEAD, LEG = 7, 5
CONTACT, CLEAR, FN, CONE, ROM = range(5)     # fields of a leg of a check record
U = 2.0 ** -53


def consts_of(model):
    """what the device reads: mass, gravity, friction and the inertia entries of DevStruct (structure.cc: (0,0) (0,1) (0,2) (1,1)
    (1,2) (2,2) with the sign of single_rigid_body_dynamics.cc:40-42), nominal stance and maximum deviation of the model"""
    I = list(model.inertia)
    n_ee = int(model.n_ee)
    return dict(n_ee=n_ee, mass=float(model.mass), gravity=float(model.gravity), mu=float(model.friction),
                Ib=np.array([I[0], -I[3], -I[4], I[1], -I[5], I[2]], dtype=np.float64),
                nominal=np.array([[model.nominal_stance[e][d] for d in range(3)] for e in range(n_ee)], dtype=np.float64),
                max_dev=np.array(list(model.max_dev), dtype=np.float64))


def flat_terrain(height=0.0):
    return lambda x, y: (np.full(len(x), float(height)), np.zeros(len(x)), np.zeros(len(x)))


def oracle_terrain(P):
    """(h, hx, hy) at arrays of points from the oracle problem's terrain_probe_full, which tests/test_terrain_probe.py pins to the
    device's terrain_eval bit for bit"""
    def fn(x, y):
        out = np.array([P.terrain_probe_full(a, b)[:3] for a, b in zip(x, y)], dtype=np.float64).reshape(-1, 3)
        return out[:, 0], out[:, 1], out[:, 2]
    return fn


def inertia_rows(Ib):
    return [[Ib[0], Ib[1], Ib[2]], [Ib[1], Ib[3], Ib[4]], [Ib[2], Ib[4], Ib[5]]]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def checks_numpy(record, consts, terrain_fn):
    """(n, 7 + 5 n_ee) check records of sample records (n, 20 + 13 n_ee); terrain_fn(x, y) -> (h, hx, hy) on arrays"""
    r = np.atleast_2d(np.asarray(record, dtype=np.float64))
    n_ee, m, g, mu = consts["n_ee"], consts["mass"], consts["gravity"], consts["mu"]
    assert r.shape[1] == 20 + 13 * n_ee
    out = np.empty((len(r), HEAD + LEG * n_ee))
    with np.errstate(all="ignore"):
        R = frame_rotation(r[:, 10:14])
        B = inertia_rows(consts["Ib"])
        A = [[R[i][0] * B[0][j] + R[i][1] * B[1][j] + R[i][2] * B[2][j] for j in range(3)] for i in range(3)]
        W = [[A[i][0] * R[j][0] + A[i][1] * R[j][1] + A[i][2] * R[j][2] for j in range(3)] for i in range(3)]
        om, od = [r[:, 14 + d] for d in range(3)], [r[:, 17 + d] for d in range(3)]
        wd = [W[i][0] * od[0] + W[i][1] * od[1] + W[i][2] * od[2] for i in range(3)]
        wo = [W[i][0] * om[0] + W[i][1] * om[1] + W[i][2] * om[2] for i in range(3)]
        cr = cross(om, wo)
        ang = [wd[i] + cr[i] for i in range(3)]
        lin = [m * r[:, 7 + d] for d in range(3)]
        pb = r[:, 1:4]
        tau, fsum = [np.zeros(len(r)) for _ in range(3)], [np.zeros(len(r)) for _ in range(3)]
        for e in range(n_ee):
            l = r[:, 20 + 13 * e:33 + 13 * e]
            pe, f = l[:, 1:4], [l[:, 10], l[:, 11], l[:, 12]]
            d = [pb[:, k] - pe[:, k] for k in range(3)]
            c = cross(f, d)
            for k in range(3):
                tau[k] = tau[k] + c[k]
                fsum[k] = fsum[k] + f[k]
            h, hx, hy = terrain_fn(pe[:, 0], pe[:, 1])
            one, zero = np.ones(len(r)), np.zeros(len(r))
            dots = []
            for v in ([-hx, -hy, one], [one, zero, hx], [zero, one, hy]):
                nr = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
                u = [v[0] / nr, v[1] / nr, v[2] / nr]
                dots.append(f[0] * u[0] + f[1] * u[1] + f[2] * u[2])
            foot = frame_vector(R, pb, pe)
            rom = np.abs(foot[:, 0] - consts["nominal"][e][0]) - consts["max_dev"][0]
            for k in (1, 2):
                rom = np.maximum(rom, np.abs(foot[:, k] - consts["nominal"][e][k]) - consts["max_dev"][k])      # (NaN wins)
            o = out[:, HEAD + LEG * e:HEAD + LEG * (e + 1)]
            o[:, CONTACT] = l[:, 0]
            o[:, CLEAR] = pe[:, 2] - h
            o[:, FN] = dots[0]
            o[:, CONE] = mu * dots[0] - np.maximum(np.abs(dots[1]), np.abs(dots[2]))
            o[:, ROM] = rom
        out[:, 0] = r[:, 0]
        for k in range(3):
            out[:, 1 + k] = ang[k] - tau[k]
        out[:, 4] = lin[0] - fsum[0]
        out[:, 5] = lin[1] - fsum[1]
        out[:, 6] = (lin[2] - fsum[2]) + m * g
    return out


def legs_of(checks, n_ee):
    """[n, n_ee, 5] view of the legs of check records (n, 7 + 5 n_ee)"""
    return checks[:, HEAD:].reshape(len(checks), n_ee, LEG)


def fold(checks, n_ee):
    """the eight scores of one problem's check records: maxima, minima and a count, a NaN among the contributing values wins"""
    legs = legs_of(checks, n_ee)
    stance = legs[:, :, CONTACT] != 0.0
    red = lambda a, op, empty: (np.nan if np.isnan(a).any() else float(op(a))) if a.size else empty
    return np.array([len(checks), red(np.abs(checks[:, 4:7]), np.max, 0.0), red(np.abs(checks[:, 1:4]), np.max, 0.0),
                     red(legs[:, :, CLEAR][~stance], np.min, 1e20), red(np.abs(legs[:, :, CLEAR][stance]), np.max, 0.0),
                     red(legs[:, :, FN][stance], np.min, 1e20), red(legs[:, :, CONE][stance], np.min, 1e20),
                     red(legs[:, :, ROM], np.max, -np.inf)], dtype=np.float64)


# ---------------------------------------------------------------- the residual in exact arithmetic, and its bound
# Rounding errors of the residual, first order in u = 2^-53, counted along checks.h:
#   quaternion  the norm's square has 4 products and 3 sums (4u), its root halves that and rounds (3u), a quotient adds 1: each
#               component 4u relative.  An entry of R is 1 - (p + q) or p +- q with products p, q of two components and an exact
#               factor 2 (9u each, |p|, |q| <= 2... their sum <= 2 for a unit quaternion), one sum (1u) and, on the diagonal,
#               one difference from 1 (1u of an entry <= 1): at most 21u absolute.  C_R = 24 leaves room for the second order.
#   A = R B     per entry sum_k (C_R u + 3u) |B_kj| (a product and two sums: 3u), |R| <= 1
#   W = A R^T   per entry sum_k ((C_R + 3) + C_R + 3) u beta_k, beta_k = sum_m |B_mk| >= |A_ik|: (2 C_R + 6) u beta, beta the sum of all |B|
#   W v         (2 C_R + 6 + 3) u beta |v|_1
#   omega x (W omega)   two products and a difference on top: (2 C_R + 9 + 2) u beta |omega|_1 per product, two products
#   tau         p_base - p_e (1u), a product (1u), the difference of two (1u), at most n_ee sums (4u), the final difference (1u): 8u
#   the sum wd + cross and the difference from tau: 2u
# so with S_ang = beta (|omega_dot|_1 + 2 |omega|_1 max|omega|) + sum_e (|f_a| |d_b| + |f_b| |d_a|) the angular error is at most
# (2 C_R + 9 + 2 + 2) u S_ang = 61 u S_ang, and with S_lin = |m a| + sum_e |f_e| (+ m g on z) the linear one at most 6u S_lin (a
# product, four sums, m g and its sum).  One constant for both:
C_R = 24.0
C_CHECK = 2 * C_R + 9 + 2 + 2


def residual_scales(record, consts):
    """(n, 6) the magnitudes S_ang (3) and S_lin (3) the bound C_CHECK * U * S refers to"""
    r = np.atleast_2d(np.asarray(record, dtype=np.float64))
    n_ee, m, g = consts["n_ee"], consts["mass"], consts["gravity"]
    beta = float(np.abs(np.array(inertia_rows(consts["Ib"]))).sum())
    om, od = np.abs(r[:, 14:17]), np.abs(r[:, 17:20])
    s = np.empty((len(r), 6))
    s[:, :3] = (beta * (od.sum(axis=1) + 2.0 * om.sum(axis=1) * om.max(axis=1)))[:, None]
    s[:, 3:] = np.abs(m * r[:, 7:10])
    s[:, 5] += m * g
    for e in range(n_ee):
        l = r[:, 20 + 13 * e:33 + 13 * e]
        f, d = np.abs(l[:, 10:13]), np.abs(r[:, 1:4] - l[:, 1:4])
        for i, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
            s[:, i] += f[:, a] * d[:, b] + f[:, b] * d[:, a]
        s[:, 3:] += f
    return s


def residual_mp(rec, consts, dps=40):
    """the six residuals of ONE record in mpmath at `dps` digits: the formulas of the header, the inputs taken as the doubles they are"""
    import mpmath
    mp = mpmath.mp
    mp.dps = dps
    f = lambda v: mp.mpf(float(v))
    n_ee, m, g = consts["n_ee"], f(consts["mass"]), f(consts["gravity"])
    w, x, y, z = (f(v) for v in rec[10:14])
    n = mp.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    R = mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    B = mp.matrix([[f(v) for v in row] for row in inertia_rows(consts["Ib"])])
    W = R * B * R.T
    om, od = mp.matrix([f(v) for v in rec[14:17]]), mp.matrix([f(v) for v in rec[17:20]])
    mcross = lambda a, b: mp.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    pb = mp.matrix([f(v) for v in rec[1:4]])
    tau, fsum = mp.matrix([0, 0, 0]), mp.matrix([0, 0, 0])
    for e in range(n_ee):
        l = rec[20 + 13 * e:33 + 13 * e]
        pe, fe = mp.matrix([f(v) for v in l[1:4]]), mp.matrix([f(v) for v in l[10:13]])
        tau += mcross(fe, pb - pe)
        fsum += fe
    ang = W * od + mcross(om, W * om) - tau
    lin = m * mp.matrix([f(v) for v in rec[7:10]]) - fsum + mp.matrix([0, 0, m * g])
    return [ang[0], ang[1], ang[2], lin[0], lin[1], lin[2]]


def random_records(n, consts, seed):
    """seeded sample records in a walking robot's ranges: a quaternion anywhere on the sphere (scaled a little off unit norm), rates
    of a few rad/s, feet around the nominal stance under the base, forces of the order of the weight"""
    rng = np.random.default_rng(seed)
    n_ee = consts["n_ee"]
    r = np.zeros((n, 20 + 13 * n_ee))
    r[:, 0] = 0.01 * np.arange(n)
    r[:, 1:4] = rng.normal(size=(n, 3)) * [1.0, 0.3, 0.05] + [0.0, 0.0, 0.3]
    r[:, 4:7] = rng.normal(size=(n, 3)) * 0.5
    r[:, 7:10] = rng.normal(size=(n, 3)) * 3.0
    q = rng.normal(size=(n, 4))
    r[:, 10:14] = q / np.linalg.norm(q, axis=1)[:, None] * rng.uniform(0.9, 1.1, size=(n, 1))
    r[:, 14:17] = rng.normal(size=(n, 3)) * 2.0
    r[:, 17:20] = rng.normal(size=(n, 3)) * 10.0
    weight = consts["mass"] * consts["gravity"]
    for e in range(n_ee):
        l = r[:, 20 + 13 * e:33 + 13 * e]
        l[:, 0] = rng.integers(2, size=n)
        l[:, 1:4] = r[:, 1:4] + consts["nominal"][e] + rng.normal(size=(n, 3)) * 0.08
        l[:, 4:10] = rng.normal(size=(n, 6))
        l[:, 10:13] = rng.normal(size=(n, 3)) * [0.2, 0.2, 0.5] * weight
    return r
