"""oracle/ref_dump/subset/Eigen is the restatement of Eigen's primitives on which the reference's own sources run where
Eigen itself is absent (oracle/ref_dump/CMakeLists.txt).  It is test infrastructure, and it is tested here on its own:
tests/eigen_subset_driver.cc applies every member the reference uses to seeded random inputs of towr's shapes (3, 6,
3 x 3, 3 x n, 6 x n, n up to 300, sparse rows with explicit zeros) and dumps inputs and results; this module redoes
each operation with numpy (values, in extended precision so that the expected value carries no error of its own) and
scipy.sparse (patterns, on matrices of ones) and compares.

Values: an entry that is a sum of k products a_i * b_i must lie within (k + 2) * 2^-53 * sum |a_i| |b_i| of the exact
value (the standard dot-product bound, gamma_k <= (k + 2) u for the k roundings of the products and sums plus the
final conversion); a chain of two products (A B) C is bounded with k = k1 + k2 + 2 on |A| |B| |C|, which dominates both
stages.  Anything without arithmetic (views, transposes, inserts, initialisers) must be bit-equal.
Patterns: which entries are stored must be exactly what the rule stated in the subset says, explicit zeros included;
the known-answer cases below pin each rule on values where the numeric and the structural result differ."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
L = np.longdouble


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eigen_subset") / "driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "oracle", "ref_dump", "subset"),
                           os.path.join(ROOT, "tests", "eigen_subset_driver.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True).stdout.split("\n")
    rec, i = {}, 0
    while i < len(out) and out[i]:
        t = out[i].split()
        r, c = int(t[2]), int(t[3])
        if t[0] == "D":
            vals = [float.fromhex(v) for v in out[i + 1:i + 1 + r * c]]
            rec[t[1]] = np.array(vals).reshape(r, c)
            i += 1 + r * c
        else:
            n = int(t[4])
            trip = [ln.split() for ln in out[i + 1:i + 1 + n]]
            rec[t[1]] = dict(shape=(r, c), row=np.array([int(a[0]) for a in trip], dtype=int), col=np.array([int(a[1]) for a in trip], dtype=int),
                             val=np.array([float.fromhex(a[2]) for a in trip]))
            i += 1 + n
    assert len(rec) > 500
    return rec


def dense_of(s):
    d = np.zeros(s["shape"])
    d[s["row"], s["col"]] = s["val"]
    return d


def pat_of(s):
    p = np.zeros(s["shape"], dtype=bool)
    p[s["row"], s["col"]] = True
    assert p.sum() == len(s["row"]), "an entry is stored twice"
    return p


def check_order(s, name):
    key = s["row"] * (s["shape"][1] + 1) + s["col"]
    assert np.all(np.diff(key) > 0), name + ": entries not in increasing (row, column) order"


def within(got, exact, bound, name):
    """|got - exact| <= bound entrywise; exact and bound in extended precision"""
    err = np.abs(got.astype(L) - exact)
    assert got.shape == exact.shape, name
    bad = ~(err <= bound)
    assert not bad.any(), "%s: worst error %.3e against the bound %.3e" % (name, float(err[bad].max()), float(np.asarray(bound)[bad].max() if np.ndim(bound) else bound))


def prod_check(got, factors, name, extra_k=0):
    """got = product of the dense factors: k = sum of the inner sizes (+ 2 per extra stage), bound on the product of |factors|"""
    exact, absprod = factors[0].astype(L), np.abs(factors[0]).astype(L)
    k = 0
    for f in factors[1:]:
        k += f.shape[0] + (2 if k else 0)
        exact, absprod = exact @ f.astype(L), absprod @ np.abs(f).astype(L)
    within(got, exact, (k + extra_k + 2) * L(U) * absprod, name)


def sparse_check(got, exact_dense, bound, pattern, name):
    check_order(got, name)
    assert got["shape"] == pattern.shape, name
    assert np.array_equal(pat_of(got), pattern), name + ": stored pattern differs"
    within(dense_of(got), exact_dense, bound, name)


def pattern_product(*pats):
    """structural product on matrices of ones (scipy.sparse): an entry wherever one stored factor meets another"""
    m = sp.csr_matrix(pats[0].astype(np.int64))
    for p in pats[1:]:
        m = m @ sp.csr_matrix(p.astype(np.int64))
    return m.toarray() > 0


@pytest.mark.parametrize("n", [5, 6, 37, 300])
def test_dense_members_against_numpy(dump, n):
    t = "d%d_" % n
    g = lambda k: dump[t + k]
    a3, b3, a6, an, bn, A, B, A3n, A6n, Ann, s = (g(k) for k in ("a3", "b3", "a6", "an", "bn", "A", "B", "A3n", "A6n", "Ann", "s"))
    s = s[0, 0]
    aL, bL = an.astype(L), bn.astype(L)
    # one rounding each (k = 1 product, or a sum of two terms taken as two products by 1)
    within(g("add"), aL + bL, 4 * L(U) * (np.abs(aL) + np.abs(bL)), "add")
    within(g("sub"), aL - bL, 4 * L(U) * (np.abs(aL) + np.abs(bL)), "sub")
    within(g("pluseq"), aL + bL, 4 * L(U) * (np.abs(aL) + np.abs(bL)), "+=")
    within(g("minuseq"), g("pluseq").astype(L) - aL, 4 * L(U) * (np.abs(g("pluseq")) + np.abs(aL)), "-=")
    assert np.array_equal(g("neg"), -an) and np.array_equal(g("int_scal"), -an)
    for k in ("scal_l", "scal_r"):
        within(g(k), L(s) * aL, 3 * L(U) * np.abs(L(s) * aL), k)
    within(g("div"), aL / L(s), 3 * L(U) * np.abs(aL / L(s)), "div")
    within(g("cwise"), aL * bL, 3 * L(U) * np.abs(aL * bL), "cwiseProduct")
    prod_check(g("AB"), [A, B], "3x3 * 3x3")
    prod_check(g("Aa3"), [A, a3], "3x3 * 3")
    prod_check(g("A3n_an"), [A3n, an], "3xn * n")
    prod_check(g("A6n_an"), [A6n, an], "6xn * n")
    prod_check(g("Ann_an"), [Ann, an], "mxn * n")
    prod_check(g("AtB"), [A.T, B], "transpose * matrix")
    prod_check(g("inner"), [an.T, bn], "a^T b")
    prod_check(g("dot"), [an.T, bn], "dot")
    # a3^T (b3 - s a3): the difference is formed first (two roundings), then three products
    d3 = b3.astype(L) - L(s) * a3.astype(L)
    within(g("inner3"), a3.astype(L).T @ d3, (3 + 2 + 2) * L(U) * (np.abs(a3).T.astype(L) @ (np.abs(b3) + abs(s) * np.abs(a3)).astype(L)), "a^T (b - s a)")
    cr = np.cross(a3[:, 0].astype(L), b3[:, 0].astype(L)).reshape(3, 1)
    crb = np.array([abs(a3[1, 0] * b3[2, 0]) + abs(a3[2, 0] * b3[1, 0]), abs(a3[2, 0] * b3[0, 0]) + abs(a3[0, 0] * b3[2, 0]),
                    abs(a3[0, 0] * b3[1, 0]) + abs(a3[1, 0] * b3[0, 0])], dtype=L).reshape(3, 1)
    within(g("cross"), cr, 4 * L(U) * crb, "cross")
    sq = (aL * aL).sum()
    within(g("sqnorm"), sq.reshape(1, 1), (n + 2) * L(U) * sq, "squaredNorm")
    within(g("sum"), aL.sum().reshape(1, 1), (n + 2) * L(U) * np.abs(aL).sum(), "sum")
    # sqrt halves the relative error of its argument and adds one rounding: (n + 2) u still bounds it
    within(g("norm"), np.sqrt(sq).reshape(1, 1), (n + 2) * L(U) * np.sqrt(sq), "norm")
    # v / norm: the norm's relative error plus one division
    within(g("normalized"), aL / np.sqrt(sq), (n + 4) * L(U) * np.abs(aL) / np.sqrt(sq), "normalized")
    sq3 = (a3.astype(L) ** 2).sum()
    within(g("normalized3"), a3.astype(L) / np.sqrt(sq3), 7 * L(U) * np.abs(a3).astype(L) / np.sqrt(sq3), "normalized (3)")
    dL = aL - bL
    quad = (dL * aL * dL).sum()
    within(g("diag_quad"), quad.reshape(1, 1), (n + 2 + 6) * L(U) * (np.abs(aL) * (np.abs(aL) + np.abs(bL)) ** 2).sum(), "d^T diag(a) d")
    within(g("mat_diag"), A3n.astype(L) * aL.T, 3 * L(U) * np.abs(A3n.astype(L) * aL.T), "matrix * diagonal")
    # no arithmetic: bit-equal
    eq = lambda k, ref: (np.array_equal(g(k), ref) or pytest.fail("%s%s differs" % (t, k)))
    eq("transpose", A3n.T), eq("vtranspose", an.T), eq("segment", an[1:n - 1]), eq("middleRows", A6n[2:5]), eq("row", A6n[4:5])
    eq("col", A6n[:, n - 1:n]), eq("topRows", A6n[:2]), eq("topRows2", a3[:2])
    w = np.zeros((n, 1))
    w[1:4] = a3
    w[n - 3:] = b3            # (n = 5, 6: the second assignment overwrites part of the first, as in the driver)
    eq("segment_w", w)
    assert np.array_equal(g("segment_w6")[:3], a3)
    prod_check(g("segment_w6")[3:], [A, b3], "segment = product")
    W = np.zeros((6, n))
    W[3:6] = A3n
    W[0] = an[:, 0]
    W[:, 2] = a6[:, 0]
    W[:, 3] -= a6[:, 0]
    W[:, 2] += a6[:, 0]
    eq("views_w", W)
    W[0] = bn[:, 0]
    eq("topRows_w", W)
    eq("setIdentity", np.eye(3)), eq("resize", np.zeros((n, 1))), eq("setOnes", np.ones((n, 1))), eq("setZero", np.zeros((n, 1)))
    eq("comma_m", np.arange(1.0, 10.0).reshape(3, 3)), eq("comma_v", np.array([[s], [2.0], [-1.0]]))
    eq("comma_finished", np.array([[s], [-3.5]]))
    ws = np.zeros((n, 1))
    ws[1:4] = a3
    eq("segment_fixed_w", ws), eq("segment_fixed", a3)
    eq("unit", np.array([[0.0], [1.0], [0.0]])), eq("zero3", np.zeros((3, 1))), eq("zero_rc", np.zeros((2, n))), eq("zero_n", np.zeros((n, 1)))
    eq("xyz", np.array([[an[0, 0]], [an[1, 0]], [an[0, 0] + 1.0]])), eq("xy", np.array([[1.5], [-2.5]])), eq("map", an)
    eq("rows_cols", np.array([[6.0], [float(n)], [float(n)]]))


@pytest.mark.parametrize("n", [5, 6, 37, 300])
def test_sparse_members_against_numpy_and_scipy(dump, n):
    t = "s%d_" % n
    g = lambda k: dump[t + k]
    P, Q, R3, N, v = (g(k) for k in ("P", "Q", "R3", "N", "v"))
    Md, xn, x3, s = g("Md"), g("xn"), g("x3"), g("s")[0, 0]
    for k in ("P", "Q", "R3", "N", "v"):
        check_order(g(k), k)
    assert (P["val"] == 0).any() or (Q["val"] == 0).any() or (N["val"] == 0).any(), "the inputs should hold explicit zeros"
    Pd, Qd, Rd, Nd, vd = (dense_of(m).astype(L) for m in (P, Q, R3, N, v))
    Pp, Qp, Rp, Np, vp = (pat_of(m) for m in (P, Q, R3, N, v))
    u = L(U)
    # sum / difference: union pattern, also where the values cancel
    sparse_check(g("add"), Pd + Qd, 4 * u * (abs(Pd) + abs(Qd)), Pp | Qp, "A + B")
    sparse_check(g("sub"), Pd - Qd, 4 * u * (abs(Pd) + abs(Qd)), Pp | Qp, "A - B")
    sparse_check(g("self_sub"), 0 * Pd, 0, Pp, "A - A")
    sparse_check(g("pluseq"), Pd + Qd, 4 * u * (abs(Pd) + abs(Qd)), Pp | Qp, "A += B")
    pe = dense_of(g("pluseq")).astype(L)
    sparse_check(g("minuseq"), pe - Pd, 4 * u * (abs(pe) + abs(Pd)), Pp | Qp, "A -= B")
    # scalar multiples keep the pattern, also for the factor 0
    sparse_check(g("neg"), -Pd, 0, Pp, "-A"), sparse_check(g("int_scal"), -Pd, 0, Pp, "-1 * A"), sparse_check(g("scal_0"), 0 * Pd, 0, Pp, "0 * A")
    sparse_check(g("scal_l"), L(s) * Pd, 3 * u * abs(L(s) * Pd), Pp, "s * A"), sparse_check(g("scal_r"), L(s) * Pd, 3 * u * abs(L(s) * Pd), Pp, "A * s")
    # sparse * sparse: structural product, nothing pruned
    sparse_check(g("prod"), Rd @ Pd, 5 * u * (abs(Rd) @ abs(Pd)), pattern_product(Rp, Pp), "A * B")
    sparse_check(g("prod3"), Rd @ Pd @ Nd, (3 + n + 4) * u * (abs(Rd) @ abs(Pd) @ abs(Nd)), pattern_product(Rp, Pp, Np), "A * B * C")
    sparse_check(g("row_prod"), vd @ Pd, 5 * u * (abs(vd) @ abs(Pd)), pattern_product(vp, Pp), "row vector * B")
    sparse_check(g("rowblock_prod"), Rd[1:2] @ Pd, 5 * u * (abs(Rd[1:2]) @ abs(Pd)), pattern_product(Rp[1:2], Pp), "A.row(i) * B")
    ML = Md.astype(L)
    sparse_check(g("view_prod"), ML @ Rd @ ML.T, (3 + 3 + 4) * u * (abs(ML) @ abs(Rd) @ abs(ML.T)), pattern_product(Md != 0, Rp, Md.T != 0),
                 "sparseView * A * sparseView")
    row2 = Rd[2:3] @ Qd
    sparse_check({**g("row_sum_w"), "shape": g("row_sum_w")["shape"]}, np.vstack([0 * row2, vd @ Pd + row2, 0 * row2]),
                 (3 + 2 + 2) * u * np.vstack([0 * row2, abs(vd) @ abs(Pd) + abs(Rd[2:3]) @ abs(Qd), 0 * row2]),
                 np.vstack([np.zeros((1, n), bool), pattern_product(vp, Pp) | pattern_product(Rp[2:3], Qp), np.zeros((1, n), bool)]), "row(i) = a + b")
    # sparse * dense
    within(g("sp_dense"), Pd @ xn.astype(L), (n + 2) * u * (abs(Pd) @ abs(xn).astype(L)), "A * x")
    within(g("sp_dense3"), Rd @ ML.T @ x3.astype(L), (3 + 3 + 4) * u * (abs(Rd) @ abs(ML.T) @ abs(x3).astype(L)), "A * M^T * x")
    within(g("dense_sp"), ML @ Pd, 5 * u * (abs(ML) @ abs(Pd)), "M * A")
    within(g("spT_diag_vec"), Pd.T @ (x3.astype(L) ** 2), (3 + 2 + 2) * u * (abs(Pd.T) @ (x3.astype(L) ** 2)), "A^T diag(x) x")
    sparse_check(g("sp_diag"), Pd * xn.astype(L).T, 3 * u * abs(Pd * xn.astype(L).T), Pp, "A * diagonal")
    # views, conversions, inserts: bit-equal
    z = lambda m: np.zeros_like(m)
    sparse_check(g("sparseView"), ML, 0, Md != 0, "sparseView()"), sparse_check(g("sparseView_all"), ML, 0, np.ones((3, 3), bool), "sparseView(1, -1)")
    assert (Md == 0).sum() == 2
    sparse_check(g("vec_sparseView_all"), x3.T.astype(L), 0, np.ones((1, 3), bool), "v^T.sparseView(1, -1)")
    sparse_check(g("transpose"), Pd.T, 0, Pp.T, "transpose"), sparse_check(g("const_row"), Pd[2:3], 0, Pp[2:3], "row(i) const")
    sparse_check(g("const_middleRows"), Pd[1:3], 0, Pp[1:3], "middleRows const")
    assert np.array_equal(g("to_dense"), dense_of(R3))
    sparse_check(g("middleRows_w"), np.vstack([Pd, L(s) * Qd]), np.vstack([z(Pd), 3 * u * abs(L(s) * Qd)]), np.vstack([Pp, Qp]), "middleRows(a, n) = B")
    top, x0 = Qd - Pd, x3[0, 0]
    want = np.vstack([top, L(s) * Qd[0:1], Pd[0:1], L(s) * Qd[2:3] + Pd[1:2] + L(x0) * Pd[2:3]])
    bound = np.vstack([4 * u * (abs(Pd) + abs(Qd)), 3 * u * abs(L(s) * Qd[0:1]), z(Pd[0:1]),
                       8 * u * (abs(L(s) * Qd[2:3]) + abs(Pd[1:2]) + abs(L(x0) * Pd[2:3]))])
    sparse_check(g("rows_w"), want, bound, np.vstack([Pp | Qp, Qp[0:1], Pp[0:1], Qp[2:3] | Pp[1:2] | Pp[2:3]]), "row(i) = / += after middleRows =")
    c = np.zeros((3, n))
    cp = np.zeros((3, n), bool)
    c[0, 1], c[2, n - 1], c[1, 3] = s, 2.0 + s, 4.0
    cp[0, 2] = cp[0, 1] = cp[2, n - 1] = cp[1, 0] = cp[1, 3] = True
    sparse_check(g("coeffRef"), c.astype(L), 0, cp, "coeffRef / insert")
    assert g("nonZeros")[0, 0] == 5 and np.array_equal(g("coeff")[:, 0], [s, 0.0, 2.0 + s]) and g("empty_nonZeros")[0, 0] == 0
    comp = g("compressed")
    assert np.array_equal(comp[0], g("coeffRef")["val"]) and np.array_equal(comp[1], g("coeffRef")["col"])
    assert np.array_equal(comp[2, :4], np.concatenate([[0], np.cumsum(cp.sum(axis=1))]))
    assert g("resize")["shape"] == (2, 4) and len(g("resize")["val"]) == 0


def test_structural_rules_known_answers(dump):
    """One known answer per structural rule, on values where the numeric and the structural result differ."""
    def stored(name):
        s = dump[name]
        check_order(s, name)
        return [(int(r), int(c), float(v)) for r, c, v in zip(s["row"], s["col"], s["val"])]

    # a 3 x 3 with two exact zeros through both sparseView forms
    assert stored("ka_sparseView") == [(0, 0, 1.0), (0, 2, 2.0), (1, 1, 3.0), (1, 2, 4.0), (2, 0, 5.0), (2, 1, 6.0), (2, 2, 7.0)]
    assert stored("ka_sparseView_all") == [(0, 0, 1.0), (0, 1, 0.0), (0, 2, 2.0), (1, 0, 0.0), (1, 1, 3.0), (1, 2, 4.0), (2, 0, 5.0), (2, 1, 6.0),
                                           (2, 2, 7.0)]
    # A + B with disjoint rows: the union
    assert stored("ka_disjoint_sum") == [(0, 1, 1.0), (0, 3, 2.0), (2, 0, 3.0), (3, 3, 4.0)]
    # 1*2 + 2*(-1) = 0 stays an entry; an explicit zero factor makes entries too
    assert stored("ka_structural_product") == [(0, 0, 0.0), (0, 1, 10.0), (1, 0, -0.0), (1, 1, 0.0)]
    assert stored("ka_coeffRef_zero") == [(0, 2, 0.0)]
    assert stored("ka_scaled_zero") == [(0, 1, 0.0), (0, 3, 0.0), (2, 0, 0.0), (3, 3, 0.0)]
    assert stored("ka_cancel") == [(0, 1, 0.0), (0, 3, 0.0)]
    # row(i) = replaces the whole row, row(i) += merges
    assert stored("ka_row_assign") == [(1, 1, 1.0), (1, 3, 2.0), (2, 1, 1.0), (2, 3, 6.0)]
    # middleRows(a, n) = replaces those rows and leaves the others
    assert stored("ka_middleRows_assign") == [(0, 0, 3.0), (1, 3, 4.0), (3, 2, 1.0)]


def test_quaternion_of_rotation_matrix_against_scipy(dump):
    """Quaterniond(R) vs scipy.spatial.transform.Rotation on 64 rotations over all four branches, trace <= 0 included, up
    to sign.  Bound 64 * 2^-53: the entries of R carry a few roundings each, the conversion divides sums of two of them by
    twice the largest quaternion component (>= 1/2, so no amplification beyond a factor 4), and scipy's own conversion
    rounds as often."""
    from scipy.spatial.transform import Rotation

    low_trace = 0
    for i in range(64):
        R, q = dump["quat_R%d" % i], dump["quat_q%d" % i][0]
        low_trace += np.trace(R) <= 0
        ref = Rotation.from_matrix(R).as_quat()   # x, y, z, w
        err = min(np.abs(q - ref).max(), np.abs(q + ref).max())
        assert err <= 64 * U, (i, q, ref, err)
        assert abs(np.linalg.norm(q) - 1.0) <= 64 * U
    assert low_trace >= 8
