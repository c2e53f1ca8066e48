// TEST INFRASTRUCTURE ONLY -- working stand-in for <ifopt/problem.h>: the entry points Ipopt's adapter calls, plus the
// ones oracle/ref_dump/ref_dump.cc dumps.
#pragma once
#include "constraint_set.h"
#include "cost_term.h"
#include "variable_set.h"
namespace ifopt {
class Problem {
 public:
  using VectorXd = Component::VectorXd;
  using Jacobian = Component::Jacobian;
  using VecBound = Component::VecBound;
  Problem() : variables_(std::make_shared<Composite>("variable-sets", false)), constraints_("constraint-sets", false), costs_("cost-terms", true) {}
  void AddVariableSet(VariableSet::Ptr s) { variables_->AddComponent(s); }
  void AddConstraintSet(ConstraintSet::Ptr s) {
    s->LinkWithVariables(variables_);
    constraints_.AddComponent(s);
  }
  void AddCostSet(CostTerm::Ptr s) {
    s->LinkWithVariables(variables_);
    costs_.AddComponent(s);
  }
  int GetNumberOfOptimizationVariables() const { return variables_->GetRows(); }
  int GetNumberOfConstraints() const { return constraints_.GetRows(); }
  bool HasCostTerms() const { return !costs_.GetComponents().empty(); }
  VecBound GetBoundsOnConstraints() const { return constraints_.GetBounds(); }
  VecBound GetBoundsOnOptimizationVariables() const { return variables_->GetBounds(); }
  VectorXd GetVariableValues() const { return variables_->GetValues(); }
  void SetVariables(const double* x) { variables_->SetVariables(Eigen::Map<const VectorXd>(x, GetNumberOfOptimizationVariables())); }
  VectorXd EvaluateConstraints(const double* x) {
    SetVariables(x);
    return constraints_.GetValues();
  }
  double EvaluateCostFunction(const double* x) {
    if (!HasCostTerms()) return 0.0;
    SetVariables(x);
    return costs_.GetValues()(0);
  }
  VectorXd EvaluateCostFunctionGradient(const double* x) {
    VectorXd grad = VectorXd::Zero(GetNumberOfOptimizationVariables());
    if (HasCostTerms()) {
      SetVariables(x);
      const Jacobian j = costs_.GetJacobian();
      for (Jacobian::InnerIterator it(j, 0); it; ++it) grad(it.col()) = it.value();
    }
    return grad;
  }
  Jacobian GetJacobianOfConstraints() const { return constraints_.GetJacobian(); }
  void EvalNonzerosOfJacobian(const double* x, double* values) {
    SetVariables(x);
    Jacobian jac = GetJacobianOfConstraints();
    jac.makeCompressed();
    for (int i = 0; i < static_cast<int>(jac.nonZeros()); ++i) values[i] = jac.valuePtr()[i];
  }
  Composite::Ptr GetOptVariables() const { return variables_; }
  const Composite& GetConstraints() const { return constraints_; }
  const Composite& GetCosts() const { return costs_; }

 private:
  Composite::Ptr variables_;
  Composite constraints_;
  Composite costs_;
};
}  // namespace ifopt
