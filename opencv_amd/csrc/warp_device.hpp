// warp_device.hpp — device helpers shared by warp.hip and remap.hip: the
// reference's bicubic weights, derived per pixel instead of read from a table.
#pragma once

#include <hip/hip_runtime.h>

namespace tbdk {
namespace warp_device {

// interpolateCubic (imgwarp.cpp:152-160)
__device__ __forceinline__ void cubic_coeffs(float x, float* c)
{
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// BicubicTab_i[ay*32 + ax] (initInterTab2D, imgwarp.cpp:213-268)
__device__ __forceinline__ void bicubic_tab(int ay, int ax, int* w)
{
    const float scale = 1.f / 32;
    float cy[4], cx[4];
    cubic_coeffs(ay * scale, cy);
    cubic_coeffs(ax * scale, cx);
    int isum = 0;
#pragma unroll
    for (int k1 = 0; k1 < 4; ++k1)
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) {
            int iv = __float2int_rn(cy[k1] * cx[k2] * 32768);  // saturate_cast<short>(float)
            iv = iv < -32768 ? -32768 : (iv > 32767 ? 32767 : iv);
            w[k1 * 4 + k2] = iv;
            isum += iv;
        }
    if (isum != 32768) {  // the correction searches taps (2..3, 2..3), as the reference does
        const int diff = isum - 32768;
        int M = 10, m = 10;
#pragma unroll
        for (int k1 = 2; k1 < 4; ++k1)
#pragma unroll
            for (int k2 = 2; k2 < 4; ++k2) {
                const int t = k1 * 4 + k2;
                if (w[t] < w[m]) m = t;
                else if (w[t] > w[M]) M = t;
            }
        // w[] is indexed by runtime values here: keep it in registers via selects
#pragma unroll
        for (int t = 10; t < 16; ++t) {
            if (diff < 0 && t == M) w[t] -= diff;
            if (diff >= 0 && t == m) w[t] -= diff;
        }
    }
}

}  // namespace warp_device
}  // namespace tbdk
