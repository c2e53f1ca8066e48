// TEST INFRASTRUCTURE ONLY -- stand-in for <ros/ros.h>, one of the headers under this directory on which the
// reference's fpowr extractors (footstep_plan_extractor.h, initial_guess_extractor.h, nearest_plane_lookup.h) compile
// where ROS is absent (../../CMakeLists.txt).  Each stand-in holds only the members those three headers use, written
// from those uses and from the third party's published behaviour, cited next to the code.
//
// roscpp's console macros (ros/console.h: ROS_INFO(...), ROS_DEBUG(...)) format and log their arguments and have no
// other effect; here they evaluate nothing.
#pragma once
#define ROS_INFO(...) ((void)0)
#define ROS_DEBUG(...) ((void)0)
