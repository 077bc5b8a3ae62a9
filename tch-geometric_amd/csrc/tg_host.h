// Host-side helpers of the C ABI: error text, argument checks, HIP call checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/tchgeo.h"

namespace tg {

char *last_error_buffer();

inline int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

// tg_ns_out.rows_prefilled: the slab holds rows[e] = n_seeds + e for THIS launch's n_seeds -> the launch leaves `rows` alone
inline bool ns_rows_prefilled(const tg_ns_out *out, int64_t n_seeds) {
    return out->rows_prefilled != 0 && out->rows_prefilled == n_seeds + 1;
}

// TG_SAMPLER_RECENT keeps a 32-bit position inside the column, 2^32 - 1 marking an empty entry: every column must be
// shorter than that.  A graph with fewer edges cannot have such a column; a larger one has to state its longest column.
inline bool recent_columns_fit(const tg_graph *g) {
    const int64_t limit = 0xFFFFFFFFll;
    return g->n_edges < limit || (g->max_degree > 0 && g->max_degree < limit);
}

} // namespace tg

#define TG_REQUIRE(cond, ...)                                                                                          \
    do {                                                                                                               \
        if (!(cond)) return tg::fail(TG_ERR_INVALID, __VA_ARGS__);                                                     \
    } while (0)

#define TG_HIP(call)                                                                                                   \
    do {                                                                                                               \
        hipError_t e_ = (call);                                                                                        \
        if (e_ != hipSuccess) return tg::fail(TG_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));              \
    } while (0)

#define TG_LAUNCH_CHECK()                                                                                              \
    do {                                                                                                               \
        hipError_t e_ = hipGetLastError();                                                                             \
        if (e_ != hipSuccess) return tg::fail(TG_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e_));          \
    } while (0)
