// TEST INFRASTRUCTURE ONLY -- stand-in for xpp_states/convert.h (see ../ros/ros.h for the rules).  The real header
// converts xpp states to and from ROS messages; the three fpowr headers include it and use nothing of it.
#pragma once
