// common.hpp - error reporting and small host helpers shared by the translation units of
// libdcvc_amd.so:
//   DCVC_HIP / DCVC_REQUIRE / DCVC_LAUNCH_CHECK   return E_HIP / E_ARG with the error text set
//   typed / with_flag                             run one launch expression for an entry's storage type and for a compile-time switch
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>
#include <type_traits>

#include "dcvc_amd.h"

namespace dcvc {

enum { OK = 0, E_ARG = -1, E_HIP = -2, E_MEM = -3, E_STREAM = -4 };

void set_error(const char* fmt, ...);

inline size_t elem_size(int dtype) { return dtype == DCVC_F16 ? 2 : 4; }
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace dcvc

#define DCVC_HIP(expr)                                                                      \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            dcvc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                            __LINE__);                                                      \
            return dcvc::E_HIP;                                                             \
        }                                                                                   \
    } while (0)

#define DCVC_REQUIRE(cond, ...)           \
    do {                                  \
        if (!(cond)) {                    \
            dcvc::set_error(__VA_ARGS__); \
            return dcvc::E_ARG;           \
        }                                 \
    } while (0)

#define DCVC_LAUNCH_CHECK()                                                               \
    do {                                                                                  \
        hipError_t _e = hipGetLastError();                                                \
        if (_e != hipSuccess) {                                                           \
            dcvc::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e),    \
                            __FILE__, __LINE__);                                          \
            return dcvc::E_HIP;                                                           \
        }                                                                                 \
    } while (0)

#ifdef __HIPCC__   // (the host-compiler translation units launch nothing and need not know _Float16)
namespace dcvc {

template <int V>
using IC = std::integral_constant<int, V>;

// launch(T{}) with T the storage type of `dtype`, then the launch check: return typed(dtype, [&](auto tag) { ... });
template <typename F>
int typed(int dtype, F&& launch)
{
    if (dtype == DCVC_F16)
        launch(_Float16{});
    else if (dtype == DCVC_F32)
        launch(float{});
    else {
        set_error("bad dtype %d", dtype);
        return E_ARG;
    }
    DCVC_LAUNCH_CHECK();
    return 0;
}

// f(std::true_type{}) or f(std::false_type{}): decltype(flag)::value is a template argument
template <typename F>
void with_flag(bool flag, F&& f)
{
    if (flag)
        f(std::true_type{});
    else
        f(std::false_type{});
}

}  // namespace dcvc
#endif
