// TEST INFRASTRUCTURE ONLY -- stand-in for xpp_states/endeffectors.h (see ../ros/ros.h for the rules).
// Published behaviour (xpp_states/include/xpp_states/endeffectors.h): EndeffectorID is an unsigned int;
// Endeffectors<T> keeps one T per end-effector in a std::deque (so that at() of Endeffectors<bool> is a real
// reference), at(ee) is bounds-checked, GetEECount() is the number of end-effectors and GetEEsOrdered() lists the ids
// 0, 1, ..., n - 1 in that order.  EndeffectorsContact is Endeffectors<bool>, constructed with a count and one value
// for all (default: not in contact).
#pragma once
#include <Eigen/Dense>
#include <deque>
#include <vector>

#include <xpp_states/state.h>

namespace xpp {

using EndeffectorID = unsigned int;

template <typename T>
class Endeffectors {
 public:
  explicit Endeffectors(int n_ee = 0) : ee_(static_cast<size_t>(n_ee)) {}
  T& at(EndeffectorID ee) { return ee_.at(ee); }
  const T& at(EndeffectorID ee) const { return ee_.at(ee); }
  int GetEECount() const { return static_cast<int>(ee_.size()); }
  std::vector<EndeffectorID> GetEEsOrdered() const {
    std::vector<EndeffectorID> ids;
    for (EndeffectorID ee = 0; ee < ee_.size(); ++ee) ids.push_back(ee);
    return ids;
  }
  void SetAll(const T& value) {
    for (T& e : ee_) e = value;
  }

 private:
  std::deque<T> ee_;
};

using EndeffectorsPos = Endeffectors<Eigen::Vector3d>;
using EndeffectorsMotion = Endeffectors<StateLin3d>;

class EndeffectorsContact : public Endeffectors<bool> {
 public:
  explicit EndeffectorsContact(int n_ee = 0, bool in_contact = false) : Endeffectors<bool>(n_ee) { SetAll(in_contact); }
};

}  // namespace xpp
