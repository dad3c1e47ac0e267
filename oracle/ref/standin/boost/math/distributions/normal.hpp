#pragma once
/* Stand-in for boost::math::normal and boost::math::pdf, the one stand-in that carries arithmetic.  The density is
 *     pdf(N(m, sd), x) = exp(-(x - m)^2 / (2 sd^2)) / (sd sqrt(2 pi))
 * in double precision.  Boost is not available to this build, so the insert-size term of the pairing step is pinned to the
 * reference UP TO THIS FORMULA: everything around it (which distances are scored, the penalty, the choice of the maximum) is the
 * reference's own code or follows it line by line in ../../ref_driver.cpp. */
#include <cmath>
namespace boost { namespace math {
class normal {
    double m_, sd_;
public:
    normal(double mean = 0, double sd = 1) : m_(mean), sd_(sd) {}
    double mean() const { return m_; }
    double standard_deviation() const { return sd_; }
};
inline double pdf(const normal& d, double x)
{
    double z = x - d.mean();
    return std::exp(-(z * z) / (2 * d.standard_deviation() * d.standard_deviation())) / (d.standard_deviation() * std::sqrt(2 * M_PI));
}
} }
