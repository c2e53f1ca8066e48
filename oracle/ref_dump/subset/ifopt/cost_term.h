// TEST INFRASTRUCTURE ONLY -- working stand-in for <ifopt/cost_term.h>: a constraint set with one row whose value is
// GetCost() and which has no bound.
#pragma once
#include "constraint_set.h"
namespace ifopt {
class CostTerm : public ConstraintSet {
 public:
  using Ptr = std::shared_ptr<CostTerm>;
  CostTerm(const std::string& name) : ConstraintSet(1, name) {}
  virtual double GetCost() const = 0;
  VectorXd GetValues() const final {
    VectorXd cost(1);
    cost(0) = GetCost();
    return cost;
  }
  VecBound GetBounds() const final { return VecBound(GetRows(), NoBound); }
};
}  // namespace ifopt
