// TEST INFRASTRUCTURE ONLY -- stand-in for xpp_states/endeffector_mappings.h: the quadruped's foot order.
#pragma once
namespace xpp {
namespace quad {
enum FootIDs { LF, RF, LH, RH };
}
}  // namespace xpp
