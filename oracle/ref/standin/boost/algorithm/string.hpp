#pragma once
#include <string>
#include <vector>
namespace boost { struct is_iequal {}; struct first_finder_t { std::string sep; };
inline first_finder_t first_finder(const std::string& s, is_iequal) { return first_finder_t{s}; }
template<class V> void iter_split(V& out, const std::string& line, const first_finder_t& f) { out.clear(); size_t p = 0; for(;;) { size_t q = line.find(f.sep, p); if(q == std::string::npos) { out.push_back(line.substr(p)); break; } out.push_back(line.substr(p, q - p)); p = q + f.sep.size(); } }
template<class V> std::string join(const V& v, const std::string& sep) { std::string r; bool first = true; for(const auto& x : v) { if(!first) r += sep; r += x; first = false; } return r; }
namespace algorithm { using boost::join; } }
