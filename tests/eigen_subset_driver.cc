// TEST INFRASTRUCTURE ONLY -- exercises every member of oracle/ref_dump/subset/Eigen that the reference's sources use, on
// seeded random inputs of the shapes towr uses, and dumps inputs and results as text; tests/test_eigen_subset.py redoes
// every operation with numpy / scipy from the dumped inputs and compares.
//   D <name> <rows> <cols>  then rows*cols hex floats, row by row
//   S <name> <rows> <cols> <stored>  then "row col hexvalue" per stored entry in storage order
#include <Eigen/Dense>
#include <Eigen/Sparse>

#include <cstdint>
#include <cstdio>
#include <string>

using namespace Eigen;
using Sp = SparseMatrix<double, RowMajor>;
using SpRow = SparseVector<double, RowMajor>;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double rnd() {   // uniform in (-2, 2), splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (static_cast<double>(z >> 11) / 9007199254740992.0) * 4.0 - 2.0;
}
static void D(const std::string& name, const Dense& m) {
  std::printf("D %s %d %d\n", name.c_str(), (int)m.rows(), (int)m.cols());
  for (Index i = 0; i < m.rows(); ++i)
    for (Index j = 0; j < m.cols(); ++j) std::printf("%a\n", m(i, j));
}
static void D(const std::string& name, double v) {
  Dense m(1, 1);
  m(0, 0) = v;
  D(name, m);
}
static void S(const std::string& name, const Sp& m) {
  std::printf("S %s %d %d %d\n", name.c_str(), (int)m.rows(), (int)m.cols(), (int)m.nonZeros());
  for (int r = 0; r < m.outerSize(); ++r)
    for (Sp::InnerIterator it(m, r); it; ++it) std::printf("%d %d %a\n", (int)it.row(), (int)it.col(), it.value());
}
static VectorXd rvec(int n) {
  VectorXd v(n);
  for (int i = 0; i < n; ++i) v(i) = rnd();
  return v;
}
static MatrixXd rmat(int r, int c) {
  MatrixXd m = MatrixXd::Zero(r, c);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < c; ++j) m(i, j) = rnd();
  return m;
}
// a random sparse r x c: about `fill` of the entries stored, one in five of them an explicit zero
static Sp rsp(int r, int c, double fill) {
  Sp m(r, c);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < c; ++j)
      if (rnd() + 2.0 < 4.0 * fill) m.coeffRef(i, j) = (rnd() > 1.2) ? 0.0 : rnd();
  return m;
}

static void dense_ops(const std::string& t, int n) {
  Vector3d a3 = rvec(3), b3 = rvec(3);
  Matrix<double, 6, 1> a6 = rvec(6);
  VectorXd an = rvec(n), bn = rvec(n);
  Matrix3d A = rmat(3, 3), B = rmat(3, 3);
  MatrixXd A3n = rmat(3, n), A6n = rmat(6, n), Ann = rmat(n > 40 ? 40 : n, n);
  const double s = rnd();
  D(t + "a3", a3); D(t + "b3", b3); D(t + "a6", a6); D(t + "an", an); D(t + "bn", bn);
  D(t + "A", A); D(t + "B", B); D(t + "A3n", A3n); D(t + "A6n", A6n); D(t + "Ann", Ann); D(t + "s", s);
  // arithmetic
  D(t + "add", an + bn); D(t + "sub", an - bn); D(t + "neg", -an); D(t + "scal_l", s * an); D(t + "scal_r", an * s);
  D(t + "div", an / s); D(t + "int_scal", -1 * an);
  D(t + "AB", A * B); D(t + "Aa3", A * a3); D(t + "A3n_an", A3n * an); D(t + "A6n_an", A6n * an); D(t + "Ann_an", Ann * an);
  D(t + "AtB", A.transpose() * B);
  const double inner = an.transpose() * bn;   // 1 x 1 -> scalar
  D(t + "inner", inner);
  const double inner3 = a3.transpose() * (b3 - s * a3);
  D(t + "inner3", inner3);
  D(t + "dot", an.dot(bn)); D(t + "cross", a3.cross(b3)); D(t + "norm", an.norm()); D(t + "sqnorm", an.squaredNorm());
  D(t + "sum", an.sum()); D(t + "normalized", an.normalized()); D(t + "normalized3", a3.normalized());
  D(t + "cwise", an.cwiseProduct(bn));
  D(t + "diag_quad", (an - bn).transpose() * an.asDiagonal() * (an - bn));
  D(t + "mat_diag", A3n * an.asDiagonal());
  VectorXd acc = an; acc += bn; D(t + "pluseq", acc); acc -= an; D(t + "minuseq", acc);
  // views and initialisers: no arithmetic
  D(t + "transpose", A3n.transpose()); D(t + "vtranspose", an.transpose());
  D(t + "segment", an.segment(1, n - 2)); D(t + "middleRows", A6n.middleRows(2, 3)); D(t + "row", A6n.row(4));
  D(t + "col", A6n.col(n - 1)); D(t + "topRows", A6n.topRows(2));
  Vector2d top2 = a3.topRows<2>(); D(t + "topRows2", top2);
  VectorXd w = VectorXd::Zero(n);
  w.segment(1, 3) = a3; w.middleRows(n - 3, 3) = b3; D(t + "segment_w", w);
  Matrix<double, 6, 1> w6; w6.segment(0, 3) = a3; w6.segment(3, 3) = A * b3; D(t + "segment_w6", w6);
  MatrixXd W = MatrixXd::Zero(6, n);
  W.middleRows(3, 3) = A3n; W.row(0) = an.transpose(); W.col(2) = a6; W.col(3) -= a6; W.col(2) += a6; D(t + "views_w", W);
  W.topRows(1) = bn.transpose(); D(t + "topRows_w", W);
  Matrix3d I3; I3.setIdentity(); D(t + "setIdentity", I3);
  VectorXd o; o.resize(n); D(t + "resize", o); o.setOnes(); D(t + "setOnes", o); o.setZero(); D(t + "setZero", o);
  Matrix3d C; C << 1, 2, 3, 4, 5, 6, 7, 8, 9; D(t + "comma_m", C);
  VectorXd cv(3); cv << s, 2.0, -1.0; D(t + "comma_v", cv);
  VectorXd fin = (VectorXd(2) << s, -3.5).finished(); D(t + "comma_finished", fin);
  VectorXd ws = VectorXd::Zero(n); ws.segment<3>(1) = a3; D(t + "segment_fixed_w", ws);
  const VectorXd& cws = ws; Vector3d rs = cws.segment<3>(1); D(t + "segment_fixed", rs);
  D(t + "unit", Vector3d::Unit(1)); D(t + "zero3", Vector3d::Zero()); D(t + "zero_rc", MatrixXd::Zero(2, n)); D(t + "zero_n", VectorXd::Zero(n));
  Vector3d xyz(an(0), an(1), an(2)); xyz.z() = xyz.x() + 1.0; D(t + "xyz", xyz);
  Vector2d xy(1.5, -2.5); D(t + "xy", xy);
  D(t + "map", VectorXd(Map<const VectorXd>(an.data(), n)));
  D(t + "rows_cols", Vector3d((double)A6n.rows(), (double)A6n.cols(), (double)an.rows()));
}

static void sparse_ops(const std::string& t, int n) {
  Sp P = rsp(3, n, 0.4), Q = rsp(3, n, 0.4), R3 = rsp(3, 3, 0.7), N = rsp(n, n > 60 ? 60 : n, 0.1);
  SpRow v = rsp(1, 3, 0.9);
  MatrixXd Md = rmat(3, 3);
  Md(0, 1) = 0.0; Md(2, 2) = 0.0;
  VectorXd xn = rvec(n);
  Vector3d x3 = rvec(3);
  const double s = rnd();
  S(t + "P", P); S(t + "Q", Q); S(t + "R3", R3); S(t + "N", N); S(t + "v", v); D(t + "Md", Md); D(t + "xn", xn); D(t + "x3", x3); D(t + "s", s);
  S(t + "add", P + Q); S(t + "sub", P - Q); S(t + "self_sub", P - P); S(t + "neg", -P); S(t + "scal_l", s * P); S(t + "scal_r", P * s);
  S(t + "scal_0", 0.0 * P); S(t + "int_scal", -1 * P);
  S(t + "prod", R3 * P); S(t + "prod3", R3 * P * N); S(t + "row_prod", v * P); S(t + "rowblock_prod", R3.row(1) * P);
  S(t + "view_prod", Md.sparseView() * R3 * Md.transpose().sparseView());
  D(t + "sp_dense", P * xn); D(t + "sp_dense3", R3 * Md.transpose() * x3); D(t + "dense_sp", Md * P);
  S(t + "sparseView", Md.sparseView()); S(t + "sparseView_all", Md.sparseView(1.0, -1.0));
  S(t + "vec_sparseView_all", x3.transpose().sparseView(1.0, -1.0));
  S(t + "transpose", P.transpose());
  Matrix3d back = R3; D(t + "to_dense", back);
  Sp J(6, n);
  J.middleRows(0, 3) = P;
  J.middleRows(3, 3) = s * Q;
  S(t + "middleRows_w", J);
  J.middleRows(0, 3) = Q - P;       // replaces whole rows: nothing of P's pattern may survive outside the union
  J.row(4) = P.row(0);
  J.row(5) += P.row(1);
  J.row(5) += x3(0) * P.row(2);
  S(t + "rows_w", J);
  Sp K(3, n);
  K.row(1) = v * P + R3.row(2) * Q;
  S(t + "row_sum_w", K);
  Sp pe = P; pe += Q; S(t + "pluseq", pe); pe -= P; S(t + "minuseq", pe);
  const Sp Pc = P;
  S(t + "const_row", Pc.row(2)); S(t + "const_middleRows", Pc.middleRows(1, 2));
  Sp c(3, n);
  c.coeffRef(0, 2) = 0.0; c.coeffRef(0, 1) = s; c.coeffRef(0, 2) += 0.0; c.coeffRef(2, n - 1) += 2.0; c.coeffRef(2, n - 1) += s;
  c.insert(1, 0) = 0.0; c.insert(1, 3) = 4.0;
  S(t + "coeffRef", c);
  D(t + "nonZeros", (double)c.nonZeros()); D(t + "coeff", Vector3d(c.coeff(0, 1), c.coeff(0, 0), c.coeff(2, n - 1)));
  c.makeCompressed();
  Dense comp(3, c.nonZeros());
  for (Index k = 0; k < c.nonZeros(); ++k) { comp(0, k) = c.valuePtr()[k]; comp(1, k) = c.innerIndexPtr()[k]; }
  for (Index r = 0; r < 4; ++r) comp(2, r) = c.outerIndexPtr()[r];
  D(t + "compressed", comp);
  Sp z(2, 5); D(t + "empty_nonZeros", (double)z.nonZeros());
  Sp rs = P; rs.resize(2, 4); S(t + "resize", rs);
  S(t + "sp_diag", P * xn.asDiagonal());
  VectorXd grad = P.transpose() * x3.asDiagonal() * x3; D(t + "spT_diag_vec", grad);
}

// known answers for the structural rules (values chosen so that numeric and structural results differ)
static void structural_known_answers() {
  Matrix3d M;
  M << 1, 0, 2, 0, 3, 4, 5, 6, 7;
  S("ka_sparseView", M.sparseView()); S("ka_sparseView_all", M.sparseView(1.0, -1.0));
  Sp A(4, 4), B(4, 4);
  A.coeffRef(0, 1) = 1.0; A.coeffRef(0, 3) = 2.0;
  B.coeffRef(2, 0) = 3.0; B.coeffRef(3, 3) = 4.0;
  S("ka_disjoint_sum", A + B);
  // product whose numeric result is 0 but whose structural result is an entry: 1 * 2 + 2 * (-1) = 0 at (0, 0), and an
  // explicit zero factor at (1, 1)
  Sp L(2, 2), Rm(2, 2);
  L.coeffRef(0, 0) = 1.0; L.coeffRef(0, 1) = 2.0; L.coeffRef(1, 1) = 0.0;
  Rm.coeffRef(0, 0) = 2.0; Rm.coeffRef(1, 0) = -1.0; Rm.coeffRef(1, 1) = 5.0;
  S("ka_structural_product", L * Rm);
  Sp Z(1, 3);
  Z.coeffRef(0, 2) = 0.0;
  S("ka_coeffRef_zero", Z); S("ka_scaled_zero", 0.0 * (A + B)); S("ka_cancel", A - A);
  Sp T(3, 4);
  T.coeffRef(1, 0) = 9.0; T.coeffRef(1, 2) = 9.0;
  T.row(1) = A.row(0);   // replaces: (1,0) and (1,2) are gone
  T.row(2) += A.row(0);
  T.row(2) += B.row(3);   // merges: union {1, 3}, 2 + 4 at column 3
  S("ka_row_assign", T);
  Sp U(4, 4);
  U.coeffRef(0, 0) = 1.0; U.coeffRef(3, 2) = 1.0;
  U.middleRows(0, 2) = B.middleRows(2, 2);   // rows 0, 1 replaced; row 3 untouched
  S("ka_middleRows_assign", U);
}

static void quaternions() {
  // rotation matrices of quaternions spread over all four branches (w, x, y or z largest); the matrix is an input
  for (int i = 0; i < 64; ++i) {
    double q[4] = {rnd(), rnd(), rnd(), rnd()};
    q[i % 4] *= 4.0;
    if (i >= 48) q[0] *= 0.01;   // half turns: trace <= 0
    const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
    Matrix3d R;
    R << 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
         2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y);
    Quaterniond got(R);
    Dense o(1, 4);
    o(0, 0) = got.x(); o(0, 1) = got.y(); o(0, 2) = got.z(); o(0, 3) = got.w();
    D("quat_R" + std::to_string(i), R);
    D("quat_q" + std::to_string(i), o);
  }
}

int main() {
  const int ns[] = {5, 6, 37, 300};
  for (int n : ns) {
    dense_ops("d" + std::to_string(n) + "_", n);
    sparse_ops("s" + std::to_string(n) + "_", n);
  }
  structural_known_answers();
  quaternions();
  return 0;
}
