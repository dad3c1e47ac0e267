#pragma once
#include <random>
namespace boost { namespace random { template<class E> struct uniform_01 { E e; uniform_01(E e_) : e(e_) {} double operator()() { return std::generate_canonical<double, 53>(e); } }; } }
