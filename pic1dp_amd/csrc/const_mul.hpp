// const_mul.hpp -- x / lx as a correctly rounded multiplication by the constant C = 1/lx in TWO operations
// (Brisebarre and Muller, "Correctly rounded multiplication by arbitrary precision constants", IEEE TC 2008):
//     yh = RN(C), yl = RN(C - yh),   q = fma(yh, x, RN(yl x))
// equals RN(C x) = RN(x / lx) for every double x for MOST constants; const_mul_decide (const_mul.cpp) decides it
// for a given lx exactly, in integer arithmetic -- no sampling.  Plain C++: no device code, no HIP header
// (tests/const_mul_check.cpp builds it with the host sanitizers).
#pragma once
#include <cstdint>
#include <vector>

namespace pic1dp {

struct ConstMul {
  double hi = 0.0, lo = 0.0;   // yh, yl
  int proven = 0;              // 1: the two operations give RN(x / lx) for every double x with 2^-500 <= |x| <= 2^500
  int candidates = 0;          // significands the decision had to evaluate (the operands nearest to a rounding boundary)
  int failed = 0;              // ... of which the two operations round differently from the division
};
// `worst` (or null) receives the candidates as doubles in [2^52, 2^53): every significand X for which X / lx lies
// close enough to a rounding boundary that the two operations' error could carry it across.  The decision is
// "every one of them, evaluated, rounds as the division does"; all other significands are safe by the error bound.
ConstMul const_mul_decide(double lx, std::vector<double> *worst = nullptr);

// the two operations themselves, with the host's fma (correctly rounded, as the device's)
double const_mul_quotient(double x, double hi, double lo);

}  // namespace pic1dp
