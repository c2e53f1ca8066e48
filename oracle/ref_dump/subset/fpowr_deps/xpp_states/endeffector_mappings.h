// TEST INFRASTRUCTURE ONLY -- stand-in for xpp_states/endeffector_mappings.h (see ../ros/ros.h for the rules).
// Published values (xpp_states/include/xpp_states/endeffector_mappings.h): biped feet L = 0, R = 1; quadruped feet
// LF = 0, RF = 1, LH = 2, RH = 3.  fpowr_xpp_ee_map.h maps towr's ids onto these, and ref_dump executes that map.
#pragma once

namespace xpp {
namespace biped {
enum FootIDs { L = 0, R = 1 };
}
namespace quad {
enum FootIDs { LF = 0, RF = 1, LH = 2, RH = 3 };
}
}  // namespace xpp
