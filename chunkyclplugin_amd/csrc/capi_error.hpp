// capi_error.hpp — what every file behind include/chunky_hip.h needs to refuse a call: the calling thread's last error, and the
// two copies of a struct that carries its own size.  Plain C++: no HIP type.
#pragma once
#include <cstddef>
#include <cstring>
#include <string>

#pragma GCC visibility push(hidden)  // internal to the library: none of this is part of its surface

extern thread_local std::string tls_error;

int fail(int code, const char* fmt, ...);

// The caller's struct may be older (shorter) or newer (longer) than this library's T; `have` is the size it declares.
// Reading: the bytes both sides know, the rest of *out zero; false (and *out untouched) when the caller's struct is shorter than
// the struct's first version.
template <class T>
bool take_versioned(const T* theirs, size_t have, size_t first_version, T* out) {
    if (have < first_version) return false;
    memset(out, 0, sizeof *out);
    memcpy(out, theirs, have < sizeof *out ? have : sizeof *out);  // a larger struct: only the part known here
    return true;
}
// Writing: the bytes both sides know, and the caller's `size` member as it was.
template <class T>
void give_versioned(const T& ours, T* theirs) {
    const size_t size = theirs->size;
    memcpy(theirs, &ours, size < sizeof ours ? size : sizeof ours);
    theirs->size = size;
}

#pragma GCC visibility pop
