// TEST INFRASTRUCTURE ONLY -- driver for the REAL reference (see CMakeLists.txt next to this file): builds the NLP the
// way towr/test/hopper_example.cc:45-90 and fpowr/src/footstep_plan_server.cc:147-220 do, sets the variables to a given
// x and dumps what Ipopt would be handed: g = Problem::EvaluateConstraints(x), the Jacobian triplets of
// Problem::GetJacobianOfConstraints() (explicit zeros included), the bounds on constraints and variables, the names and
// sizes of the constraint and variable sets in composite order and the contact schedule the formulation ran on:
//   <out prefix>_x.txt _g.txt _jac.txt ("row col value")  _bounds.txt _xbounds.txt ("lower upper")
//   <out prefix>_sets.txt ("con|var <name> <rows>")  _phases.txt (the format of --phases)
// tests/test_ref_dump.py compares the dump with the oracle and the structure builder -- for the built-in cases, for
// EVERY golden fixture of tests/golden/mp_*.npz and for a walk over random problems -- when the executable exists;
// oracle/ref_golden.py records it as the fixtures tests/golden/ref_*.npz.
//
//   ref_dump <robot id> <terrain id> <gait combo> <T> <constraint mask (TWR_SET_* bits)> <x file (one double per line, or
//            "guess")> <goal x> <out prefix> [options]
//   options:
//     --phases FILE      explicit contact schedule instead of <gait combo>/<T>: one line per end-effector,
//                        "<in contact at start 0|1> <d0> <d1> ..." (what the fixtures and the sweep candidates carry)
//     --dt DYN ROM       dt_constraint_dynamic_ / dt_constraint_range_of_motion_ (BASELINE sizes: T / (K - 1.5))
//     --params DUR_BASE_POLY POLYS_PER_SWING POLYS_PER_STANCE_FORCE DT_BASE_MOTION BASE_Z
//                        duration_base_polynomial_, ee_polynomials_per_swing_phase_, force_polynomials_per_stance_phase_,
//                        dt_constraint_base_motion_ and the z of the initial base position (the centre of baseMotion's
//                        z bound); a value <= 0 (or "nan" for BASE_Z) keeps the reference's default
//     --csv FILE         terrain = HeightMapFromCSV(FILE) instead of <terrain id>
//     --grid-map FILE RES PX PY   terrain = the `Grid` height map fpowr runs on (towr/include/towr/terrain/grid_height_map.h,
//                        fpowr/src/footstep_plan_server.cc:155) over the float "elevation" layer in FILE (first line
//                        "<size_x> <size_y>", then size_x * size_y values, x index fastest = grid_map's column-major
//                        storage), resolution RES, map position (PX, PY).  Needs grid_map_ros and
//                        convex_plane_decomposition_msgs (ROS) on the box: exit code 4 where they are missing
//     --binding          ALSO build the device sets through towr_amd/csrc/towr_binding.h on the same NlpFormulation and
//                        compare them with the reference's own sets on this x: names, rows, bounds, values, Jacobian
//                        (needs -DTOWR_AMD_ROOT=<repository> at configure time, libtowr_amd.so and a GPU); exit code 3
//                        when they differ by more than 1e-9 relative
//   the extractors fpowr runs on a solution (fpowr/include/fpowr/{footstep_plan_extractor,initial_guess_extractor,
//   nearest_plane_lookup}.h, included below where they lie), on the splines as EvaluateConstraints(x) left them.  They
//   compile on the stand-ins for ROS / xpp / tf / boost::geometry under subset/fpowr_deps; exit code 4 where the build has
//   them compiled out, exit code 5 for a sample time the reference's Spline::GetSegmentID is not defined for
//   (t > T + 1e-10, which GetTrajectory's own loop reaches when an accumulated t falls into (T + 1e-10, T + 1e-5]):
//     --sample DT        <out prefix>_traj.txt: fpowr::GetTrajectory(solution, DT), one line per state,
//                        [t | base lin p v a (9) | q w x y z | w (3) | wd (3) | per foot: contact, p v a (9), force (3)],
//                        the feet in xpp order (fpowr_xpp_ee_map.h is executed)
//     --guess-times FILE <out prefix>_guess.txt: fpowr::ExtractInitialGuesses for the times in FILE (one per line, in
//                        that order), 49 doubles per line: time, state (12), controls (36)
//     --planes FILE HORIZON   <out prefix>_plan.txt: what fpowr::ExtractFootstepPlan puts into the message for the planar
//                        regions in FILE (one line per region: position x y z, orientation x y z w, number of boundary
//                        points, then their local x y) and the time horizon: per footstep state one line, the
//                        duration, then the contact_set (plane index per foot, -1 = in the air)
//   ref_dump --terrain-points IN OUT [--csv FILE]   the terrains alone at given points, see TerrainPoints() below
//                        (oracle/ref_golden.py --terrain records it as tests/golden/refterrain_*.npz)
//   ref_dump --segment-points IN OUT   Spline::GetSegmentID / GetLocalTime on given duration lists and times, or
//                        PhaseDurations::SetVariables + ConvertPhaseToPolyDurations on given schedule variables, see
//                        SegmentPoints() below (oracle/ref_golden.py --segments records it as tests/golden/refsegment.npz);
//                        exit code 5 for a time the lookup is not defined for
//   ref_dump --plane-points IN OUT   PlanarRegionsToPolygons and NearestPlaneLookup::GetNearestPlaneIndex on given regions and
//                        points, with bg::distance per region, see PlanePoints() below (oracle/ref_golden.py --planes records
//                        it as tests/golden/refplane.npz)
//   ref_dump --attitude-points IN OUT   Eigen::Quaterniond(R) on given matrices, or EulerConverter's rotation matrix, quaternion,
//                        angular velocity and acceleration on given states of the Euler-angle spline, see AttitudePoints() below
//                        (oracle/ref_golden.py --attitude records it as tests/golden/refattitude.npz)
#include <ifopt/problem.h>
#include <towr/initialization/gait_generator.h>
#include <towr/nlp_formulation.h>
#include <towr/terrain/examples/height_map_examples.h>
#include <towr/terrain/height_map_from_csv.h>
#include <towr/variables/euler_converter.h>
#include <towr/variables/node_spline.h>
#include <towr/variables/nodes_variables_all.h>
#include <towr/variables/nodes_variables_phase_based.h>
#include <towr/variables/phase_durations.h>
#include <towr/variables/spline.h>
#if __has_include(<grid_map_ros/grid_map_ros.hpp>) && __has_include(<convex_plane_decomposition_msgs/PlanarTerrain.h>)
#include <towr/terrain/grid_height_map.h>
#define TWR_REF_HAVE_GRID_MAP 1
#endif

#ifdef TWR_REF_EXTRACTORS
// one translation unit only: the three headers define non-inline functions
#include <fpowr/footstep_plan_extractor.h>
#include <fpowr/initial_guess_extractor.h>
#include <fpowr/nearest_plane_lookup.h>
#endif

#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#ifdef TWR_WITH_BINDING
#include "towr_binding.h"
#endif

#ifdef TWR_REF_EXTRACTORS
// true when GetTrajectory(solution, dt) stays inside what Spline::GetSegmentID defines: the loop of
// footstep_plan_extractor.h:22-50 repeated on the times alone
static bool SampleTimesDefined(double T, double dt) {
  if (!(dt > 0.0)) return false;
  for (double t = 0.0; t <= T + 1e-5; t += dt)
    if (t > T + 1e-10) return false;
  return true;
}
#endif

// ref_dump --terrain-points IN OUT [--csv FILE]: the reference's terrains alone, no NLP.  IN holds raw doubles, four per
// point: terrain id (HeightMap::TerrainID 0..6, 7 = HeightMapFromCSV(FILE)), x, y, and a flag.  OUT receives raw doubles:
// per point GetHeight, GetDerivativeOfHeightWrt(X_), (Y_) and the second derivative wrt x twice -- Gap's public
// GetHeightDerivWrtXX; no other terrain overrides the base class's (private) zero, written here as 0 -- and, where the flag
// is set, 27 more: GetNormalizedBasis(Normal | Tangent1 | Tangent2) (3 x 3), then GetDerivativeOfNormalizedBasisWrt(basis,
// dim) for basis = Normal, Tangent1, Tangent2 and dim = X_, Y_ in that order (6 x 3), which carry every second derivative
static int TerrainPoints(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: ref_dump --terrain-points IN OUT [--csv FILE]\n");
    return 2;
  }
  std::string csv_file;
  for (int i = 4; i < argc; ++i) {
    if (std::string(argv[i]) == "--csv" && i + 1 < argc) csv_file = argv[++i];
    else {
      std::fprintf(stderr, "unknown option %s\n", argv[i]);
      return 2;
    }
  }
  std::vector<double> in;
  {
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot read %s\n", argv[2]);
      return 2;
    }
    double buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
  }
  if (in.empty() || in.size() % 4) {
    std::fprintf(stderr, "%s: %zu doubles do not make whole points\n", argv[2], in.size());
    return 2;
  }
  std::vector<towr::HeightMap::Ptr> maps;
  for (int id = 0; id < towr::HeightMap::TERRAIN_COUNT; ++id) maps.push_back(towr::HeightMap::MakeTerrain(static_cast<towr::HeightMap::TerrainID>(id)));
  if (!csv_file.empty()) maps.push_back(std::make_shared<HeightMapFromCSV>(csv_file));
  const towr::Gap gap;
  std::vector<double> out;
  using H = towr::HeightMap;
  for (size_t k = 0; k < in.size(); k += 4) {
    const int id = static_cast<int>(in[k]);
    if (id < 0 || id >= static_cast<int>(maps.size())) {
      std::fprintf(stderr, "%s: point %zu names terrain %d\n", argv[2], k / 4, id);
      return 2;
    }
    const H& t = *maps[id];
    const double x = in[k + 1], y = in[k + 2];
    out.push_back(t.GetHeight(x, y));
    out.push_back(t.GetDerivativeOfHeightWrt(towr::X_, x, y));
    out.push_back(t.GetDerivativeOfHeightWrt(towr::Y_, x, y));
    out.push_back(id == H::GapID ? gap.GetHeightDerivWrtXX(x, y) : 0.0);
    if (in[k + 3] != 0.0) {
      for (H::Direction b : {H::Normal, H::Tangent1, H::Tangent2}) {
        const Eigen::Vector3d v = t.GetNormalizedBasis(b, x, y);
        for (int i = 0; i < 3; ++i) out.push_back(v(i));
      }
      for (H::Direction b : {H::Normal, H::Tangent1, H::Tangent2})
        for (towr::Dim2D dim : {towr::X_, towr::Y_}) {
          const Eigen::Vector3d v = t.GetDerivativeOfNormalizedBasisWrt(b, dim, x, y);
          for (int i = 0; i < 3; ++i) out.push_back(v(i));
        }
    }
  }
  std::FILE* f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", argv[3]);
    return 2;
  }
  std::printf("ref_dump: %zu terrain points, %zu values\n", in.size() / 4, out.size());
  return 0;
}

// the protected Spline::GetLocalTime, made callable
struct SegmentSpline : towr::Spline {
  SegmentSpline() : towr::Spline({1.0}, 1) {}
  using towr::Spline::GetLocalTime;
};

// ref_dump --segment-points IN OUT: the segment lookup and the duration conversion alone, no NLP.  IN holds raw doubles, the
// first one the mode.
//   mode 0: the number of lists; per list its length n and n durations; the number of points; per point the index of its
//           list and t.  OUT: per point Spline::GetSegmentID(t, list) and the id and local time of Spline::GetLocalTime(t,
//           list) -- three doubles.  A point with t < 0, or for which no accumulated sum reaches t - 1e-10, is outside what
//           spline.cc:48-66 defines (its asserts): nothing is written and the exit code is 5.
//   mode 1: the number of cases; per case the number of phases n, whether the foot starts in contact, the polynomials per
//           swing phase and per stance phase of the force, the n given durations and the n - 1 schedule variables (their sum
//           below the given total, phase_durations.cc:91).  OUT: per case PhaseDurations::GetPhaseDurations() after
//           SetVariables (n), then the count and the values of ConvertPhaseToPolyDurations of NodesVariablesEEMotion and of
//           NodesVariablesEEForce on them.
static int SegmentPoints(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: ref_dump --segment-points IN OUT\n");
    return 2;
  }
  std::vector<double> in;
  {
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot read %s\n", argv[2]);
      return 2;
    }
    double buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
  }
  size_t at = 0;
  auto have = [&](size_t k) { return at + k <= in.size(); };
  auto bad = [&](const char* what) {
    std::fprintf(stderr, "%s: %s\n", argv[2], what);
    return 2;
  };
  if (!have(2)) return bad("empty");
  const int mode = static_cast<int>(in[at++]);
  std::vector<double> out;
  if (mode == 0) {
    const long n_lists = static_cast<long>(in[at++]);
    std::vector<std::vector<double>> lists;
    for (long l = 0; l < n_lists; ++l) {
      if (!have(1)) return bad("truncated list");
      const long n = static_cast<long>(in[at++]);
      if (n < 1 || !have(n)) return bad("truncated list");
      lists.emplace_back(in.begin() + at, in.begin() + at + n);
      at += n;
    }
    if (!have(1)) return bad("no points");
    const long n_points = static_cast<long>(in[at++]);
    if (n_points < 0 || at + 2 * static_cast<size_t>(n_points) != in.size()) return bad("point count");
    const SegmentSpline spline;
    for (long k = 0; k < n_points; ++k, at += 2) {
      const long l = static_cast<long>(in[at]);
      const double t = in[at + 1];
      if (l < 0 || l >= n_lists) return bad("list index");
      bool found = false;
      double acc = 0.0;
      for (double d : lists[l]) {
        acc += d;
        if (acc >= t - 1e-10) found = true;
      }
      if (!(t >= 0.0) || !found) {
        std::fprintf(stderr, "--segment-points: point %ld (list %ld, t = %.17g) is outside what Spline::GetSegmentID defines\n", k, l, t);
        return 5;
      }
      const auto lt = spline.GetLocalTime(t, lists[l]);
      out.push_back(towr::Spline::GetSegmentID(t, lists[l]));
      out.push_back(lt.first);
      out.push_back(lt.second);
    }
  } else if (mode == 1) {
    const long n_cases = static_cast<long>(in[at++]);
    for (long c = 0; c < n_cases; ++c) {
      if (!have(4)) return bad("truncated case");
      const long n = static_cast<long>(in[at]);
      const bool contact = in[at + 1] != 0.0;
      const int pps = static_cast<int>(in[at + 2]), ppf = static_cast<int>(in[at + 3]);
      at += 4;
      if (n < 1 || pps < 1 || ppf < 1 || !have(2 * n - 1)) return bad("truncated case");
      const std::vector<double> given(in.begin() + at, in.begin() + at + n);
      Eigen::VectorXd x(n - 1);
      for (long i = 0; i < n - 1; ++i) x(i) = in[at + n + i];
      at += 2 * n - 1;
      towr::PhaseDurations pd(0, given, contact, 0.0, 1e20);
      pd.SetVariables(x);
      const std::vector<double> ph = pd.GetPhaseDurations();
      const towr::NodesVariablesEEMotion motion(n, contact, "m", pps);
      const towr::NodesVariablesEEForce force(n, contact, "f", ppf);
      const std::vector<double> md = motion.ConvertPhaseToPolyDurations(ph), fd = force.ConvertPhaseToPolyDurations(ph);
      out.insert(out.end(), ph.begin(), ph.end());
      out.push_back(md.size());
      out.insert(out.end(), md.begin(), md.end());
      out.push_back(fd.size());
      out.insert(out.end(), fd.begin(), fd.end());
    }
    if (at != in.size()) return bad("trailing data");
  } else {
    return bad("unknown mode");
  }
  std::FILE* f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", argv[3]);
    return 2;
  }
  std::printf("ref_dump: segment mode %d, %zu values\n", mode, out.size());
  return 0;
}

// ref_dump --plane-points IN OUT: the nearest-plane lookup alone, no NLP.  IN holds raw doubles: the number of scenes; per scene
// the number of regions, per region position x y z, orientation x y z w, the number k of boundary points and their k local
// (x, y), then the number of query points and their (x, y).  A scene becomes a convex_plane_decomposition_msgs::PlanarTerrain.
// OUT per scene: the world (x, y) of every boundary point as fpowr::PlanarRegionsToPolygons made them, region after region;
// per query point fpowr::NearestPlaneLookup::GetNearestPlaneIndex; per query point and region bg::distance(point, polygon)
// (point-major).  Exit code 4 where the build has the fpowr extractors compiled out.
static int PlanePoints(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: ref_dump --plane-points IN OUT\n");
    return 2;
  }
#ifdef TWR_REF_EXTRACTORS
  std::vector<double> in;
  {
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot read %s\n", argv[2]);
      return 2;
    }
    double buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
  }
  size_t at = 0;
  auto have = [&](size_t k) { return at + k <= in.size(); };
  auto bad = [&](const char* what) {
    std::fprintf(stderr, "%s: %s\n", argv[2], what);
    return 2;
  };
  if (!have(1)) return bad("empty");
  const long n_scenes = static_cast<long>(in[at++]);
  std::vector<double> out;
  size_t n_pairs = 0;
  for (long s = 0; s < n_scenes; ++s) {
    if (!have(1)) return bad("truncated scene");
    const long n_regions = static_cast<long>(in[at++]);
    if (n_regions < 0) return bad("region count");
    convex_plane_decomposition_msgs::PlanarTerrain terrain;
    for (long r = 0; r < n_regions; ++r) {
      if (!have(8)) return bad("truncated region");
      convex_plane_decomposition_msgs::PlanarRegion region;
      auto& pp = region.plane_parameters;
      pp.position.x = in[at], pp.position.y = in[at + 1], pp.position.z = in[at + 2];
      pp.orientation.x = in[at + 3], pp.orientation.y = in[at + 4], pp.orientation.z = in[at + 5], pp.orientation.w = in[at + 6];
      const long k = static_cast<long>(in[at + 7]);
      at += 8;
      if (k < 0 || !have(2 * static_cast<size_t>(k))) return bad("truncated boundary");
      for (long i = 0; i < k; ++i, at += 2) {
        convex_plane_decomposition_msgs::Point2d pt;
        pt.x = in[at];
        pt.y = in[at + 1];
        if (static_cast<double>(pt.x) != in[at] || static_cast<double>(pt.y) != in[at + 1])
          return bad("a boundary point the message's number format does not hold exactly");
        region.boundary.outer_boundary.points.push_back(pt);
      }
      terrain.planarRegions.push_back(region);
    }
    if (!have(1)) return bad("no points");
    const long n_points = static_cast<long>(in[at++]);
    if (n_points < 0 || !have(2 * static_cast<size_t>(n_points))) return bad("truncated points");
    const std::vector<polygon_t> polygons = fpowr::PlanarRegionsToPolygons(terrain);
    for (const polygon_t& poly : polygons)
      for (const point_t& p : poly.outer()) {
        out.push_back(p.x());
        out.push_back(p.y());
      }
    const fpowr::NearestPlaneLookup lookup(terrain);
    Eigen::VectorXd position(2);
    for (long k = 0; k < n_points; ++k) {
      position(0) = in[at + 2 * k];
      position(1) = in[at + 2 * k + 1];
      out.push_back(lookup.GetNearestPlaneIndex(position));
    }
    for (long k = 0; k < n_points; ++k)
      for (const polygon_t& poly : polygons) out.push_back(bg::distance(point_t(in[at + 2 * k], in[at + 2 * k + 1]), poly));
    n_pairs += static_cast<size_t>(n_points) * polygons.size();
    at += 2 * static_cast<size_t>(n_points);
  }
  if (at != in.size()) return bad("trailing data");
  std::FILE* f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", argv[3]);
    return 2;
  }
  std::printf("ref_dump: %ld plane scenes, %zu (ring, point) pairs\n", n_scenes, n_pairs);
  return 0;
#else
  std::fprintf(stderr, "--plane-points: this build has the fpowr extractors compiled out\n");
  return 4;
#endif
}

// ref_dump --attitude-points IN OUT: the attitude of the base alone, no NLP.  IN holds raw doubles, the first one the mode, the
// second the number of points n.
//   mode 0: per point a 3 x 3 matrix, row-major.  OUT per point: Eigen::Quaterniond(R) as x y z w -- of the Eigen this build
//           uses (oracle/_ref/DEPS), the statement of euler_converter.cc:55.
//   mode 1: per point the 12 values [p0 v0 p1 v1] of a NodesVariablesAll with two nodes of three dimensions.  A NodeSpline of one
//           polynomial of duration 1 on them is the Euler-angle spline of an EulerConverter.  OUT per point, 28 doubles: the state
//           NodeSpline::GetPoint(0) returns (angles, rates, accelerations: the input of everything that follows), the matrix of
//           the static GetRotationMatrixBaseToWorld(angles) row-major, the static GetQuaternionBaseToWorld(angles) as x y z w,
//           GetAngularVelocityInWorld(0.0) and GetAngularAccelerationInWorld(0.0) (the static ones are private).
static int AttitudePoints(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: ref_dump --attitude-points IN OUT\n");
    return 2;
  }
  std::vector<double> in;
  {
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) {
      std::fprintf(stderr, "cannot read %s\n", argv[2]);
      return 2;
    }
    double buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
  }
  auto bad = [&](const char* what) {
    std::fprintf(stderr, "%s: %s\n", argv[2], what);
    return 2;
  };
  if (in.size() < 2) return bad("empty");
  const int mode = static_cast<int>(in[0]);
  const long n = static_cast<long>(in[1]);
  if (mode != 0 && mode != 1) return bad("unknown mode");
  const size_t per = mode == 0 ? 9 : 12;
  if (n < 0 || 2 + per * static_cast<size_t>(n) != in.size()) return bad("point count");
  std::vector<double> out;
  const double* p = in.data() + 2;
  if (mode == 0) {
    for (long k = 0; k < n; ++k, p += 9) {
      Eigen::Matrix3d R;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R(r, c) = p[3 * r + c];
      const Eigen::Quaterniond q(R);
      out.insert(out.end(), {q.x(), q.y(), q.z(), q.w()});
    }
  } else {
    auto nodes = std::make_shared<towr::NodesVariablesAll>(2, 3, "attitude");
    auto spline = std::make_shared<towr::NodeSpline>(nodes.get(), std::vector<double>{1.0});
    const towr::EulerConverter converter(spline);
    Eigen::VectorXd x(12);
    for (long k = 0; k < n; ++k, p += 12) {
      for (int i = 0; i < 12; ++i) x(i) = p[i];
      nodes->SetVariables(x);
      const towr::State s = spline->GetPoint(0.0);
      const Eigen::Vector3d angles = s.p();
      for (int i = 0; i < 3; ++i) out.push_back(s.p()(i));
      for (int i = 0; i < 3; ++i) out.push_back(s.v()(i));
      for (int i = 0; i < 3; ++i) out.push_back(s.a()(i));
      const auto R = towr::EulerConverter::GetRotationMatrixBaseToWorld(angles);
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out.push_back(R.coeff(r, c));
      const Eigen::Quaterniond q = towr::EulerConverter::GetQuaternionBaseToWorld(angles);
      out.insert(out.end(), {q.x(), q.y(), q.z(), q.w()});
      const Eigen::Vector3d w = converter.GetAngularVelocityInWorld(0.0), wd = converter.GetAngularAccelerationInWorld(0.0);
      for (int i = 0; i < 3; ++i) out.push_back(w(i));
      for (int i = 0; i < 3; ++i) out.push_back(wd(i));
    }
  }
  std::FILE* f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", argv[3]);
    return 2;
  }
  std::printf("ref_dump: attitude mode %d, %ld points, %zu values\n", mode, n, out.size());
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "--terrain-points") return TerrainPoints(argc, argv);
  if (argc >= 2 && std::string(argv[1]) == "--segment-points") return SegmentPoints(argc, argv);
  if (argc >= 2 && std::string(argv[1]) == "--plane-points") return PlanePoints(argc, argv);
  if (argc >= 2 && std::string(argv[1]) == "--attitude-points") return AttitudePoints(argc, argv);
  if (argc < 9) {
    std::fprintf(stderr, "usage: see the header of ref_dump.cc\n");
    return 2;
  }
  const int robot = std::atoi(argv[1]), terrain = std::atoi(argv[2]), combo = std::atoi(argv[3]);
  const double T = std::atof(argv[4]);
  const int mask = std::atoi(argv[5]);
  const std::string xfile = argv[6], prefix = argv[8];
  const double goal_x = std::atof(argv[7]);
  std::string phases_file, csv_file, grid_file;
  double dt_dyn = 0.0, dt_rom = 0.0, grid_res = 0.0, grid_px = 0.0, grid_py = 0.0;
  double dur_base_poly = 0.0, dt_base_motion = 0.0, base_z = std::nan("");
  int polys_swing = 0, polys_force = 0;
  bool binding = false;
  double sample_dt = 0.0, plan_horizon = 0.0;
  std::string guess_file, planes_file;
  for (int i = 9; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--phases" && i + 1 < argc) phases_file = argv[++i];
    else if (a == "--csv" && i + 1 < argc) csv_file = argv[++i];
    else if (a == "--grid-map" && i + 4 < argc) {
      grid_file = argv[++i];
      grid_res = std::atof(argv[++i]);
      grid_px = std::atof(argv[++i]);
      grid_py = std::atof(argv[++i]);
    }
    else if (a == "--dt" && i + 2 < argc) {
      dt_dyn = std::atof(argv[++i]);
      dt_rom = std::atof(argv[++i]);
    } else if (a == "--params" && i + 5 < argc) {
      dur_base_poly = std::atof(argv[++i]);
      polys_swing = std::atoi(argv[++i]);
      polys_force = std::atoi(argv[++i]);
      dt_base_motion = std::atof(argv[++i]);
      base_z = std::atof(argv[++i]);
    } else if (a == "--binding") binding = true;
    else if (a == "--sample" && i + 1 < argc) sample_dt = std::atof(argv[++i]);
    else if (a == "--guess-times" && i + 1 < argc) guess_file = argv[++i];
    else if (a == "--planes" && i + 2 < argc) {
      planes_file = argv[++i];
      plan_horizon = std::atof(argv[++i]);
    }
    else {
      std::fprintf(stderr, "unknown option %s\n", a.c_str());
      return 2;
    }
  }

  towr::NlpFormulation f;
#ifdef TWR_REF_HAVE_GRID_MAP
  std::shared_ptr<grid_map::GridMap> ref_grid_map;   // (kept for --binding: the device side is built from the same map)
#endif
  if (!grid_file.empty()) {
#ifdef TWR_REF_HAVE_GRID_MAP
    // the message fpowr's action goal carries (args->terrain): a grid_map with an "elevation" layer
    std::ifstream in(grid_file);
    int sx = 0, sy = 0;
    in >> sx >> sy;
    grid_map::GridMap map({"elevation"});
    map.setGeometry(grid_map::Length(sx * grid_res, sy * grid_res), grid_res, grid_map::Position(grid_px, grid_py));
    if (map.getSize()(0) != sx || map.getSize()(1) != sy) {
      std::fprintf(stderr, "grid_map made a %d x %d map of the %d x %d layer\n", map.getSize()(0), map.getSize()(1), sx, sy);
      return 2;
    }
    grid_map::Matrix& e = map["elevation"];
    for (int j = 0; j < sy; ++j)
      for (int i = 0; i < sx; ++i) in >> e(i, j);
    convex_plane_decomposition_msgs::PlanarTerrain msg;
    grid_map::GridMapRosConverter::toMessage(map, msg.gridmap);
    f.terrain_ = std::make_shared<Grid>(msg);
    ref_grid_map = std::make_shared<grid_map::GridMap>(map);
#else
    std::fprintf(stderr, "--grid-map: grid_map_ros / convex_plane_decomposition_msgs are not on this box\n");
    return 4;
#endif
  } else if (csv_file.empty()) f.terrain_ = towr::HeightMap::MakeTerrain(static_cast<towr::HeightMap::TerrainID>(terrain));
  else f.terrain_ = std::make_shared<HeightMapFromCSV>(csv_file);
  f.model_ = towr::RobotModel(static_cast<towr::RobotModel::Robot>(robot));
  const auto nominal = f.model_.kinematic_model_->GetNominalStanceInBase();
  const int n_ee = static_cast<int>(nominal.size());
  f.initial_ee_W_ = nominal;
  for (auto& p : f.initial_ee_W_) p.z() = 0.0;
  f.initial_base_.lin.at(towr::kPos).z() = std::isnan(base_z) ? -nominal.front().z() : base_z;
  f.final_base_.lin.at(towr::kPos) << goal_x, 0.0, -nominal.front().z();
  if (phases_file.empty()) {
    auto gait = towr::GaitGenerator::MakeGaitGenerator(n_ee);
    gait->SetCombo(static_cast<towr::GaitGenerator::Combos>(combo));
    for (int ee = 0; ee < n_ee; ++ee) {
      f.params_.ee_phase_durations_.push_back(gait->GetPhaseDurations(T, ee));
      f.params_.ee_in_contact_at_start_.push_back(gait->IsInContactAtStart(ee));
    }
  } else {
    std::ifstream in(phases_file);
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ls(line);
      int contact;
      if (!(ls >> contact)) continue;
      std::vector<double> d;
      for (double v; ls >> v;) d.push_back(v);
      f.params_.ee_phase_durations_.push_back(d);
      f.params_.ee_in_contact_at_start_.push_back(contact != 0);
    }
    if (static_cast<int>(f.params_.ee_phase_durations_.size()) != n_ee) {
      std::fprintf(stderr, "%s: %d schedules for %d end-effectors\n", phases_file.c_str(), (int)f.params_.ee_phase_durations_.size(), n_ee);
      return 2;
    }
  }
  if (dt_dyn > 0.0) f.params_.dt_constraint_dynamic_ = dt_dyn;
  if (dt_rom > 0.0) f.params_.dt_constraint_range_of_motion_ = dt_rom;
  if (dur_base_poly > 0.0) f.params_.duration_base_polynomial_ = dur_base_poly;
  if (polys_swing > 0) f.params_.ee_polynomials_per_swing_phase_ = polys_swing;
  if (polys_force > 0) f.params_.force_polynomials_per_stance_phase_ = polys_force;
  if (dt_base_motion > 0.0) f.params_.dt_constraint_base_motion_ = dt_base_motion;
  // constraint list from the mask, in the reference's enum order (parameters.h:139-147); bit 6 = OptimizePhaseDurations
  f.params_.constraints_.clear();
  using P = towr::Parameters;
  const P::ConstraintName order[] = {P::Terrain, P::Dynamic, P::BaseAcc, P::EndeffectorRom, P::Force, P::Swing};
  for (int b = 0; b < 6; ++b)
    if (mask & (1 << b)) f.params_.constraints_.push_back(order[b]);
  if (mask & 128) f.params_.constraints_.push_back(P::BaseRom);
  if (mask & 64) f.params_.OptimizePhaseDurations();

  ifopt::Problem nlp;
  towr::SplineHolder solution;
  for (auto c : f.GetVariableSets(solution)) nlp.AddVariableSet(c);
  for (auto c : f.GetConstraints(solution)) nlp.AddConstraintSet(c);

  Eigen::VectorXd x = nlp.GetOptVariables()->GetValues();
  if (xfile != "guess") {
    std::ifstream in(xfile);
    for (int i = 0; i < x.size(); ++i)
      if (!(in >> x[i])) {
        std::fprintf(stderr, "%s holds fewer than %d values\n", xfile.c_str(), (int)x.size());
        return 2;
      }
  }
  const Eigen::VectorXd g = nlp.EvaluateConstraints(x.data());
  auto jac = nlp.GetJacobianOfConstraints();
  std::ofstream og(prefix + "_g.txt"), oj(prefix + "_jac.txt"), ox(prefix + "_x.txt");
  og.precision(17);
  oj.precision(17);
  ox.precision(17);
  for (int i = 0; i < x.size(); ++i) ox << x[i] << "\n";
  for (int i = 0; i < g.size(); ++i) og << g[i] << "\n";
  for (int r = 0; r < jac.outerSize(); ++r)
    for (ifopt::Problem::Jacobian::InnerIterator it(jac, r); it; ++it) oj << it.row() << " " << it.col() << " " << it.value() << "\n";
  {
    std::ofstream ob(prefix + "_bounds.txt"), oxb(prefix + "_xbounds.txt"), os(prefix + "_sets.txt"), op(prefix + "_phases.txt");
    ob.precision(17);
    oxb.precision(17);
    op.precision(17);
    for (const auto& b : nlp.GetBoundsOnConstraints()) ob << b.lower_ << " " << b.upper_ << "\n";
    for (const auto& b : nlp.GetBoundsOnOptimizationVariables()) oxb << b.lower_ << " " << b.upper_ << "\n";
    for (const auto& c : nlp.GetConstraints().GetComponents()) os << "con " << c->GetName() << " " << c->GetRows() << "\n";
    for (const auto& c : nlp.GetOptVariables()->GetComponents()) os << "var " << c->GetName() << " " << c->GetRows() << "\n";
    for (int ee = 0; ee < n_ee; ++ee) {
      op << (f.params_.ee_in_contact_at_start_.at(ee) ? 1 : 0);
      for (double d : f.params_.ee_phase_durations_.at(ee)) op << " " << d;
      op << "\n";
    }
  }
  std::printf("ref_dump: n=%d m=%d nnz=%d\n", (int)x.size(), (int)g.size(), (int)jac.nonZeros());

  if (sample_dt != 0.0 || !guess_file.empty() || !planes_file.empty()) {
#ifdef TWR_REF_EXTRACTORS
    // (`solution` holds x: EvaluateConstraints above set the variables, and the splines observe them)
    const double T_total = solution.base_linear_->GetTotalTime();
    auto goal = std::make_shared<fpowr::FootstepPlanGoal>();
    if (sample_dt != 0.0) {
      if (!SampleTimesDefined(T_total, sample_dt)) {
        std::fprintf(stderr, "--sample %.17g: a sample time beyond T + 1e-10 (T = %.17g)\n", sample_dt, T_total);
        return 5;
      }
      std::ofstream ot(prefix + "_traj.txt");
      ot.precision(17);
      for (const auto& st : fpowr::GetTrajectory(solution, sample_dt)) {
        ot << st.t_global_;
        for (const Eigen::VectorXd* v : {&st.base_.lin.p_, &st.base_.lin.v_, &st.base_.lin.a_})
          for (int d = 0; d < 3; ++d) ot << " " << (*v)(d);
        ot << " " << st.base_.ang.q.w() << " " << st.base_.ang.q.x() << " " << st.base_.ang.q.y() << " " << st.base_.ang.q.z();
        for (int d = 0; d < 3; ++d) ot << " " << st.base_.ang.w(d);
        for (int d = 0; d < 3; ++d) ot << " " << st.base_.ang.wd(d);
        for (auto ee : st.ee_contact_.GetEEsOrdered()) {
          ot << " " << (st.ee_contact_.at(ee) ? 1 : 0);
          for (const Eigen::VectorXd* v : {&st.ee_motion_.at(ee).p_, &st.ee_motion_.at(ee).v_, &st.ee_motion_.at(ee).a_})
            for (int d = 0; d < 3; ++d) ot << " " << (*v)(d);
          for (int d = 0; d < 3; ++d) ot << " " << st.ee_forces_.at(ee)(d);
        }
        ot << "\n";
      }
    }
    if (!guess_file.empty()) {
      std::ifstream in(guess_file);
      for (double t; in >> t;) {
        if (!(t >= 0.0 && t <= T_total + 1e-10)) {
          std::fprintf(stderr, "--guess-times: %.17g lies outside [0, T + 1e-10] (T = %.17g)\n", t, T_total);
          return 5;
        }
        goal->state_sample_times.push_back(t);
      }
      fpowr::InitialGuessArray msg;
      fpowr::ExtractInitialGuesses(goal, solution, msg);
      std::ofstream og2(prefix + "_guess.txt");
      og2.precision(17);
      for (const auto& ig : msg.initial_guesses) {
        og2 << ig.time;
        for (double v : ig.state) og2 << " " << v;
        for (double v : ig.controls) og2 << " " << v;
        og2 << "\n";
      }
    }
    if (!planes_file.empty()) {
      if (!SampleTimesDefined(T_total, 0.01)) {   // (ExtractFootstepPlan samples at its fixed 0.01 s)
        std::fprintf(stderr, "--planes: a sample time of the 0.01 s trajectory lies beyond T + 1e-10 (T = %.17g)\n", T_total);
        return 5;
      }
      std::ifstream in(planes_file);
      std::string line;
      while (std::getline(in, line)) {
        std::istringstream ls(line);
        convex_plane_decomposition_msgs::PlanarRegion region;
        auto& pp = region.plane_parameters;
        int k = 0;
        if (!(ls >> pp.position.x >> pp.position.y >> pp.position.z >> pp.orientation.x >> pp.orientation.y >> pp.orientation.z >>
              pp.orientation.w >> k))
          continue;
        for (int i = 0; i < k; ++i) {
          double px = 0.0, py = 0.0;
          if (!(ls >> px >> py)) {
            std::fprintf(stderr, "%s: a region with fewer boundary points than it announces\n", planes_file.c_str());
            return 2;
          }
          convex_plane_decomposition_msgs::Point2d pt;
          pt.x = px;
          pt.y = py;
          if (static_cast<double>(pt.x) != px || static_cast<double>(pt.y) != py) {
            std::fprintf(stderr, "%s: a boundary point the message's number format does not hold exactly\n", planes_file.c_str());
            return 2;
          }
          region.boundary.outer_boundary.points.push_back(pt);
        }
        goal->terrain.planarRegions.push_back(region);
      }
      fpowr::FootstepPlan plan;
      fpowr::ExtractFootstepPlan(goal, solution, plan_horizon, plan);
      std::ofstream opl(prefix + "_plan.txt");
      opl.precision(17);
      for (const auto& cd : plan.contact_data) {
        opl << cd.duration;
        for (int idx : cd.contact_set) opl << " " << idx;
        opl << "\n";
      }
    }
#else
    std::fprintf(stderr, "--sample / --guess-times / --planes: this build has the fpowr extractors compiled out\n");
    return 4;
#endif
  }

  if (binding) {
#ifdef TWR_WITH_BINDING
    // the maintainer's three-line patch: same variables, the device sets in place of GetConstraints()
    ifopt::Problem dev;
    towr::SplineHolder solution2;
    for (auto c : f.GetVariableSets(solution2)) dev.AddVariableSet(c);
    towr_amd::DeviceTerrain csv_terrain;
    bool own_terrain = !csv_file.empty();
    if (!csv_file.empty()) csv_terrain = towr_amd::CsvTerrain(csv_file);
#if defined(TWR_REF_HAVE_GRID_MAP) && defined(TOWR_AMD_HAVE_GRID_MAP)
    if (ref_grid_map) {
      csv_terrain = towr_amd::GridTerrain(*ref_grid_map);
      own_terrain = true;
    }
#endif
    const auto sets = towr_amd::MakeDeviceConstraints(f, 0, own_terrain ? &csv_terrain : nullptr);
    // (the reference's sets as `nlp` holds them: linked with the variables, so that the sets which size themselves in
    // InitVariableDependedQuantities -- terrain, force, swing, totalduration -- report their rows)
    const auto ref_sets = nlp.GetConstraints().GetComponents();
    // every structural difference is named on stderr (first one per kind), values are compared where the shapes allow it
    int bad = 0;
    auto differs = [&bad](const char* what, const std::string& detail) {
      if (!bad) std::fprintf(stderr, "binding: %s differ: %s\n", what, detail.c_str());
      bad = 1;
    };
    if (sets.size() != ref_sets.size()) differs("set counts", std::to_string(sets.size()) + " vs " + std::to_string(ref_sets.size()));
    for (size_t i = 0; i < sets.size() && i < ref_sets.size(); ++i)
      if (sets[i]->GetName() != ref_sets[i]->GetName() || sets[i]->GetRows() != ref_sets[i]->GetRows())
        differs("sets", "#" + std::to_string(i) + " " + sets[i]->GetName() + " (" + std::to_string(sets[i]->GetRows()) + " rows) vs " +
                            ref_sets[i]->GetName() + " (" + std::to_string(ref_sets[i]->GetRows()) + " rows)");
    for (auto c : sets) dev.AddConstraintSet(c);
    const Eigen::VectorXd gd = dev.EvaluateConstraints(x.data());
    auto jd = dev.GetJacobianOfConstraints();
    double eg = 0, ej = 0, sg = 1e-300, sj = 1e-300;
    if (gd.size() != g.size()) differs("constraint counts", std::to_string(gd.size()) + " vs " + std::to_string(g.size()));
    if (jd.nonZeros() != jac.nonZeros()) differs("Jacobian entry counts", std::to_string(jd.nonZeros()) + " vs " + std::to_string(jac.nonZeros()));
    for (int i = 0; gd.size() == g.size() && i < g.size(); ++i) {
      eg = std::fmax(eg, std::fabs(gd[i] - g[i]));
      sg = std::fmax(sg, std::fabs(g[i]));
    }
    jac.makeCompressed();
    jd.makeCompressed();
    // the pattern is rows AND columns: the rows + 1 row starts, then the column of every entry
    for (int r = 0; jd.outerSize() == jac.outerSize() && jd.nonZeros() == jac.nonZeros() && r <= jac.outerSize(); ++r)
      if (jac.outerIndexPtr()[r] != jd.outerIndexPtr()[r]) differs("Jacobian row starts", "row " + std::to_string(r));
    if (jd.outerSize() != jac.outerSize() || jd.cols() != jac.cols())
      differs("Jacobian shapes", std::to_string(jd.outerSize()) + " x " + std::to_string(jd.cols()) + " vs " + std::to_string(jac.outerSize()) + " x " + std::to_string(jac.cols()));
    for (int k = 0; jd.nonZeros() == jac.nonZeros() && k < jac.nonZeros(); ++k) {
      if (jac.innerIndexPtr()[k] != jd.innerIndexPtr()[k]) differs("Jacobian patterns", "entry " + std::to_string(k));
      ej = std::fmax(ej, std::fabs(jd.valuePtr()[k] - jac.valuePtr()[k]));
      sj = std::fmax(sj, std::fabs(jac.valuePtr()[k]));
    }
    const auto b0 = nlp.GetBoundsOnConstraints(), b1 = dev.GetBoundsOnConstraints();
    if (b0.size() != b1.size()) differs("bound counts", std::to_string(b1.size()) + " vs " + std::to_string(b0.size()));
    for (size_t i = 0; i < b0.size() && i < b1.size(); ++i)
      if (b0[i].lower_ != b1[i].lower_ || b0[i].upper_ != b1[i].upper_) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "row %zu [%.17g, %.17g] vs [%.17g, %.17g]", i, b1[i].lower_, b1[i].upper_, b0[i].lower_, b0[i].upper_);
        differs("bounds", buf);
      }
    std::printf("binding: %zu sets, max|dg|/|g| = %.3g, max|dJ|/|J| = %.3g, structure %s\n", sets.size(), eg / sg, ej / sj, bad ? "DIFFERS" : "equal");
    if (bad || eg > 1e-9 * sg || ej > 1e-9 * sj) return 3;
#else
    std::fprintf(stderr, "--binding: configure with -DTOWR_AMD_ROOT=<towr_amd repository>\n");
    return 2;
#endif
  }
  return 0;
}
