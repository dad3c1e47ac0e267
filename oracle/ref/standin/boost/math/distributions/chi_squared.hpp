#pragma once
/* Stand-in for boost::math::chi_squared.  The typer's simpleChiSq (hla/HLATyper.cpp:4258-4320) computes 1 - cdf(chi_squared(1), x): the
 * upper tail of the chi-squared distribution with ONE degree of freedom, for which there is a closed form in double precision,
 *     cdf(chi_squared(1), x)             = 1 - erfc(sqrt(x / 2))          (x >= 0)
 *     cdf(complement(chi_squared(1), x)) = 1 - cdf(chi_squared(1), x)
 * (the complement is written as one minus the lower tail, not as erfc itself: the two differ in the last digits for small tails, and
 * the reference subtracts).  Boost is not available to this build, so the p column of
 * R1_columnIncompatibilities_<locus>.txt is pinned to the reference UP TO THIS FORMULA, as the insert-size density is up to normal.hpp;
 * when it is asked and with which counts is the reference's own code.  Any other number of degrees of freedom, and quantile(), end the
 * process: nothing the pinned paths reach uses them. */
#include "../../../standin_fail.h"
#include <cmath>
namespace boost { namespace math {
class chi_squared {
    double df_;
public:
    explicit chi_squared(double df) : df_(df) {}
    double degrees_of_freedom() const { return df_; }
};
inline double cdf(const chi_squared& d, double x)
{
    if(d.degrees_of_freedom() != 1) standin::unavailable("boost::math::cdf(chi_squared) with other than one degree of freedom");
    if(!(x >= 0)) standin::unavailable("boost::math::cdf(chi_squared) of a negative or undefined statistic");
    return 1 - std::erfc(std::sqrt(x / 2));
}
template<class D> struct complemented1 { const D& d; double x; };
template<class D> complemented1<D> complement(const D& d, double x) { return complemented1<D>{d, x}; }
template<class D> double cdf(const complemented1<D>& c) { return 1 - cdf(c.d, c.x); }
inline double quantile(const chi_squared&, double) { standin::unavailable("boost::math::quantile(chi_squared)"); }
} }
