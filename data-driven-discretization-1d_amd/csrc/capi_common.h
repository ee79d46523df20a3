// What the units of the C ABI share (capi.hip: models, integrators, populations;
// capi_train.hip: training, metrics, VJP).  Declarations only, defined in capi.hip; hidden
// visibility keeps the names out of the dynamic symbol table (exports.map).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/ddd1d.h"

namespace ddd {
namespace capi {

// The message behind ddd_last_error: one object per thread for the whole library.
extern thread_local std::string g_error;

// Formats the message into g_error and returns `code`.
int fail(int code, const char* fmt, ...);

#define DDD_HIP(expr)                                                        \
  do {                                                                       \
    hipError_t err__ = (expr);                                               \
    if (err__ != hipSuccess)                                                 \
      return fail(DDD_ERR_HIP, "%s failed: %s (%s:%d)", #expr,              \
                  hipGetErrorString(err__), __FILE__, __LINE__);             \
  } while (0)

// cfg, its struct_size, the equation and its derivative count, num_points, dx, stencil_size
int common_config_checks(const ddd_config* cfg);
bool is_conservative(int eq);
bool is_forced_family(int eq);   // equations.py:276-277: only Burgers adds forcing(t)

// The first check of every entry point that takes an argument struct: `a` and its
// struct_size (`name`: the struct's, for the message).  DDD_CHECK_ARGS returns on failure.
template <typename Args>
int check_struct_size(const Args* a, const char* name) {
  if (a == nullptr) return fail(DDD_ERR_INVALID_ARGUMENT, "args is NULL");
  if (a->struct_size != (int32_t)sizeof(Args))
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "%s.struct_size = %d, library expects %d (ABI mismatch)", name, a->struct_size,
                (int)sizeof(Args));
  return DDD_OK;
}
#define DDD_CHECK_ARGS(a, Args)                                                  \
  do {                                                                           \
    if (int rc__ = ::ddd::capi::check_struct_size<Args>(a, #Args)) return rc__;  \
  } while (0)

}  // namespace capi
}  // namespace ddd
