// TEST INFRASTRUCTURE ONLY -- stand-in: everything nearest_plane_lookup.h uses of boost::geometry is in <boost/geometry.hpp>.
#pragma once
#include <boost/geometry.hpp>
