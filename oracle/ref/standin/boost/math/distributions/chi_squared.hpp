#pragma once
/* Stand-in for boost::math::chi_squared: declared so that the typer's sources get through their #include lines; using it ends the process. */
#include "../../../standin_fail.h"
namespace boost { namespace math {
class chi_squared { public: explicit chi_squared(double) {} };
inline double cdf(const chi_squared&, double) { standin::unavailable("boost::math::cdf(chi_squared)"); }
template<class D> struct complemented1 { const D& d; double x; };
template<class D> complemented1<D> complement(const D& d, double x) { return complemented1<D>{d, x}; }
template<class D> double cdf(const complemented1<D>&) { standin::unavailable("boost::math::cdf(complement)"); }
inline double quantile(const chi_squared&, double) { standin::unavailable("boost::math::quantile(chi_squared)"); }
} }
