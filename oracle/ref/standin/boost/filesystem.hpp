#pragma once
#include <filesystem>
#include <ctime>
#include <sys/stat.h>
namespace boost { namespace filesystem { using std::filesystem::path; using std::filesystem::current_path; using std::filesystem::remove; using std::filesystem::remove_all; using std::filesystem::exists; using std::filesystem::is_directory; using std::filesystem::directory_iterator; using std::filesystem::create_directory; using std::filesystem::create_directories; using std::filesystem::is_regular_file; struct wpath : std::filesystem::path { using std::filesystem::path::path; };
inline std::time_t last_write_time(const wpath& p) { struct stat s; return ::stat(p.c_str(), &s) == 0 ? s.st_mtime : 0; } } }
