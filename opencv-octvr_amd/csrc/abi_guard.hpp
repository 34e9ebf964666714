// abi_guard.hpp — the C ABI's error boundary (internal): exceptions never cross an extern "C" function;
// every entry point runs its body under guarded(), which turns them into a status code + octvr_last_error().
#pragma once

#include <new>
#include <string>
#include <utility>

#include "host_common.hpp"

namespace octvr {

// octvr_last_error() text of the calling thread.
inline std::string& last_error() {
    thread_local std::string text;
    return text;
}
inline void set_last_error(const std::string& msg) { last_error() = msg; }

// f() as a status code.  `other`: the code of an exception that is neither an OctvrError nor bad_alloc.
template <class F>
int guarded(F&& f, int other = OCTVR_E_PARSE) {
    try {
        std::forward<F>(f)();
        return OCTVR_OK;
    } catch (const OctvrError& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error("out of host memory");
        return OCTVR_E_INVALID;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return other;
    }
}

}  // namespace octvr
