// ransac_rng.hpp — cv::RNG as the reference's RANSAC loops use it: seeded with
// (uint64)-1 per call, uniform(0, n) = (unsigned)next() % n
// (core/operations.hpp:383-393).  Shared by box_fit.hpp and homography_core.hpp;
// plain C++ outside hipcc.
#pragma once

#ifndef TBDK_HD
#if defined(__HIPCC__)
#define TBDK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define TBDK_HD inline
#endif
#endif

namespace tbdk {

struct RansacRng {
    unsigned long long state = ~0ull;
    TBDK_HD int draw(int n)
    {
        state = (unsigned long long)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
        return (int)((unsigned)state % (unsigned)n);
    }
};

}  // namespace tbdk
