// env_flag.hpp -- the library's on/off environment variables: set, not empty and not starting with '0' means on.
// A caller that wants the variable read once per process keeps the answer in a `static const bool` of its own.
#pragma once

#include <cstdlib>

namespace ldpc {

inline bool env_flag(const char *name)
{
    const char *e = std::getenv(name);
    return e && *e && *e != '0';
}

}  // namespace ldpc
