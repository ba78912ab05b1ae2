// capi_error.cpp — the calling thread's last error (chunky_last_error).
#include "capi_error.hpp"

#include <cstdarg>
#include <cstdio>

#include "../../include/chunky_hip.h"

thread_local std::string tls_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    tls_error = buf;
    return code;
}
extern "C" const char* chunky_last_error(void) { return tls_error.c_str(); }
