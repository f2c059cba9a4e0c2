// scratch.h -- the caller-owned scratch of the two-call protocol (include/pointseg_postprocess.h, include/pointseg_saliency.h): carved in
// a fixed order by one walk of the entry point's code, which the sizing call makes with no base.
#pragma once

#include "common.h"

namespace ps {

inline size_t pad256(size_t b) { return (b + 255) & ~size_t(255); }
inline unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

// the scratch of one call, carved in a fixed order; the sizing call walks the same code with base == nullptr
struct Carver {
    char* base;
    size_t off = 0;
    template <class T>
    T* take(size_t count)
    {
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += pad256(count * sizeof(T));
        return r;
    }
};

inline int check_scratch(const char* who, const void* scratch, const int64_t* scratch_bytes, size_t need)
{
    PS_CHECK(*scratch_bytes >= (int64_t)need, "%s: *scratch_bytes = %lld, this call needs %lld", who, (long long)*scratch_bytes, (long long)need);
    PS_CHECK((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "%s: scratch must be 256-byte aligned", who);
    return PS_OK;
}

}  // namespace ps
