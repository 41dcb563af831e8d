// Qualifiers and shims for the headers a plain C++17 compiler also builds.
#pragma once

#if defined(__HIPCC__)
#define DN_HD __host__ __device__
#define DN_HD_INLINE __host__ __device__ __forceinline__
#define DN_HD_NOINLINE __host__ __device__ __attribute__((noinline))
#else
#define DN_HD
#define DN_HD_INLINE inline
#define DN_HD_NOINLINE __attribute__((noinline))
#endif

// ---- the shim block: device-only spellings, builtins on the host ----
#if defined(__HIP_DEVICE_COMPILE__)
#define DN_FFSLL(x) __ffsll(x)
#define DN_DOUBLE_AS_LL(x) __double_as_longlong(x)
#define DN_LL_AS_DOUBLE(x) __longlong_as_double(x)
#define DN_TID() ((uint32_t)threadIdx.x)
#define DN_CONST_TABLE __device__ __constant__  // P10_TBL, DIM_TBL
#else
#define DN_FFSLL(x) __builtin_ffsll((long long)(x))
#define DN_DOUBLE_AS_LL(x) __builtin_bit_cast(long long, (double)(x))
#define DN_LL_AS_DOUBLE(x) __builtin_bit_cast(double, (long long)(x))
#define DN_TID() 0u  // the host checker is lane 0 of its block
#define DN_CONST_TABLE static const
#endif
