// TEST INFRASTRUCTURE ONLY -- stand-in for tf/transform_datatypes.h (see ../ros/ros.h for the rules): tf::Quaternion,
// tf::Vector3 and tf::Matrix3x3 as nearest_plane_lookup.h uses them.  Published behaviour (ROS geometry, tf/LinearMath,
// the Bullet linear-math classes in double precision):
//   Quaternion(x, y, z, w)            stores the four coefficients; length2() = x x + y y + z z + w w in that order
//   Matrix3x3(q) = setRotation(q)     d = q.length2(), s = 2 / d, xs = x s, ys = y s, zs = z s, wx = w xs, wy = w ys,
//                                     wz = w zs, xx = x xs, xy = x ys, xz = x zs, yy = y ys, yz = y zs, zz = z zs;
//                                     rows (1 - (yy + zz), xy - wz, xz + wy), (xy + wz, 1 - (xx + zz), yz - wx),
//                                     (xz - wy, yz + wx, 1 - (xx + yy)) -- no normalisation of q beyond the division by d
//   Matrix3x3 * Vector3               (row0 . v, row1 . v, row2 . v) with a . b = a.x b.x + a.y b.y + a.z b.z
//   Vector3 + Vector3                 coefficient-wise
#pragma once

namespace tf {

class Vector3 {
 public:
  Vector3() = default;
  Vector3(double x, double y, double z) : m_{x, y, z} {}
  double x() const { return m_[0]; }
  double y() const { return m_[1]; }
  double z() const { return m_[2]; }
  double dot(const Vector3& v) const { return m_[0] * v.m_[0] + m_[1] * v.m_[1] + m_[2] * v.m_[2]; }

 private:
  double m_[3] = {0.0, 0.0, 0.0};
};
inline Vector3 operator+(const Vector3& a, const Vector3& b) { return Vector3(a.x() + b.x(), a.y() + b.y(), a.z() + b.z()); }

class Quaternion {
 public:
  Quaternion(double x, double y, double z, double w) : m_{x, y, z, w} {}
  double x() const { return m_[0]; }
  double y() const { return m_[1]; }
  double z() const { return m_[2]; }
  double w() const { return m_[3]; }
  double length2() const { return m_[0] * m_[0] + m_[1] * m_[1] + m_[2] * m_[2] + m_[3] * m_[3]; }

 private:
  double m_[4];
};

class Matrix3x3 {
 public:
  explicit Matrix3x3(const Quaternion& q) { setRotation(q); }
  void setRotation(const Quaternion& q) {
    const double d = q.length2();
    const double s = 2.0 / d;
    const double xs = q.x() * s, ys = q.y() * s, zs = q.z() * s;
    const double wx = q.w() * xs, wy = q.w() * ys, wz = q.w() * zs;
    const double xx = q.x() * xs, xy = q.x() * ys, xz = q.x() * zs;
    const double yy = q.y() * ys, yz = q.y() * zs, zz = q.z() * zs;
    row_[0] = Vector3(1.0 - (yy + zz), xy - wz, xz + wy);
    row_[1] = Vector3(xy + wz, 1.0 - (xx + zz), yz - wx);
    row_[2] = Vector3(xz - wy, yz + wx, 1.0 - (xx + yy));
  }
  const Vector3& operator[](int i) const { return row_[i]; }

 private:
  Vector3 row_[3];
};
inline Vector3 operator*(const Matrix3x3& m, const Vector3& v) { return Vector3(m[0].dot(v), m[1].dot(v), m[2].dot(v)); }

}  // namespace tf
