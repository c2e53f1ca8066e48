// TEST INFRASTRUCTURE ONLY -- stand-in for xpp_states/cartesian_declarations.h: the coordinate indices.
#pragma once
namespace xpp {
enum Coords3D { X = 0, Y, Z };
}
