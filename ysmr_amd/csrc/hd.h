// YSMR_HD: `__host__ __device__` under hipcc, nothing for a plain C++ compiler -- for the headers that a stand-alone host
// program compiles alone as well (tracker_plan.h, set_order.h, fmt.h).  YSMR_HD_FORCE: ... and always inlined (HIP's
// __forceinline__, spelled out): a helper that must compile as if it were written where it is called.
#pragma once
#ifdef __HIPCC__
#define YSMR_HD __host__ __device__
#else
#define YSMR_HD
#endif
#define YSMR_HD_FORCE YSMR_HD inline __attribute__((always_inline))
