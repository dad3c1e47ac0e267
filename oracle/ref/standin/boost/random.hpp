#pragma once
#include <random>
namespace boost { typedef std::mt19937 mt19937; namespace random { template<class I=int,class R=double> using poisson_distribution = std::poisson_distribution<I>; template<class I=int> using uniform_int_distribution = std::uniform_int_distribution<I>; } }
