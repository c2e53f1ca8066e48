// TEST INFRASTRUCTURE ONLY -- driver of tests/test_ros_subset.py: applies the stand-ins under
// oracle/ref_dump/subset/fpowr_deps (tf, boost::geometry, xpp_states) to the cases in the file named on the command
// line and prints the results as hex floats, one record per input line:
//   R qx qy qz qw px py pz lx ly     -> world x y z of tf::Matrix3x3(q) * (lx, ly, 0) + (px, py, pz)
//   D n x0 y0 ... x(n-1) y(n-1) qx qy -> boost::geometry::distance(point(qx, qy), polygon with those outer points appended)
//   E n                              -> the xpp facts: GetEECount, GetEEsOrdered, enumeration values, initial flags
#include <boost/geometry.hpp>
#include <boost/geometry/geometries/point_xy.hpp>
#include <boost/geometry/geometries/polygon.hpp>
#include <tf/transform_datatypes.h>
#include <xpp_states/convert.h>
#include <xpp_states/endeffector_mappings.h>
#include <xpp_states/endeffectors.h>
#include <xpp_states/robot_state_cartesian.h>
#include <xpp_states/state.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>

// a number written as a hex float (istream's >> does not read those)
static double num(std::istream& in) {
  std::string tok;
  in >> tok;
  return std::strtod(tok.c_str(), nullptr);
}

namespace bg = boost::geometry;
using point_t = bg::model::d2::point_xy<double>;
using polygon_t = bg::model::polygon<point_t>;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    char kind = 0;
    ls >> kind;
    if (kind == 'R') {
      double q[4], p[3], lx, ly;
      for (double& v : q) v = num(ls);
      for (double& v : p) v = num(ls);
      lx = num(ls);
      ly = num(ls);
      tf::Quaternion quat(q[0], q[1], q[2], q[3]);
      tf::Matrix3x3 R(quat);
      tf::Vector3 w = R * tf::Vector3(lx, ly, 0.0) + tf::Vector3(p[0], p[1], p[2]);
      std::printf("R %a %a %a\n", w.x(), w.y(), w.z());
    } else if (kind == 'D') {
      int n = 0;
      ls >> n;
      polygon_t poly;
      for (int i = 0; i < n; ++i) {
        const double x = num(ls), y = num(ls);
        bg::append(poly.outer(), point_t(x, y));
      }
      const double qx = num(ls), qy = num(ls);
      std::printf("D %a\n", bg::distance(point_t(qx, qy), poly));
    } else if (kind == 'E') {
      int n = 0;
      ls >> n;
      xpp::Endeffectors<double> e(n);
      std::printf("E %d", e.GetEECount());
      for (auto id : e.GetEEsOrdered()) {
        e.at(id) = 10.0 + id;
        std::printf(" %u", id);
      }
      for (auto id : e.GetEEsOrdered()) std::printf(" %g", e.at(id));
      bool threw = false;
      try {
        e.at(static_cast<xpp::EndeffectorID>(n));
      } catch (const std::out_of_range&) {
        threw = true;
      }
      xpp::EndeffectorsContact c(n);
      xpp::RobotStateCartesian st(n);
      bool all_false = true, all_true = st.ee_contact_.GetEECount() == n && st.ee_motion_.GetEECount() == n && st.ee_forces_.GetEECount() == n;
      for (auto id : c.GetEEsOrdered()) {
        all_false = all_false && !c.at(id);
        all_true = all_true && st.ee_contact_.at(id);
      }
      st.ee_contact_.at(0) = false;   // a real reference into Endeffectors<bool>
      xpp::StateLinXd s(3);
      s.p_ << 1.0, 2.0, 3.0;
      s.v_ << 4.0, 5.0, 6.0;
      s.a_ << 7.0, 8.0, 9.0;
      st.ee_motion_.at(0) = s;
      xpp::StateLin3d s3 = st.ee_motion_.at(0);
      std::printf(" %d %d %d %d %g %g %g", threw ? 1 : 0, all_false ? 1 : 0, all_true ? 1 : 0, st.ee_contact_.at(0) ? 1 : 0, s3.p_(2), s3.v_(0), s3.a_(1));
      std::printf(" %d %d %d %d %d %d\n", (int)xpp::biped::L, (int)xpp::biped::R, (int)xpp::quad::LF, (int)xpp::quad::RF, (int)xpp::quad::LH,
                  (int)xpp::quad::RH);
    }
  }
  return 0;
}
