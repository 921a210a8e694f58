// klt_cn.hip — PyrLK on multi-channel (interleaved cn = 2..4) u8 frames:
// the pyramid levels, their CV_16SC(2cn) Scharr planes and the sparse
// tracker, for gfx950.
//
// The CPU path handles any channel count the same way (video/src/lkpyramid.cpp):
//   * pyrDown_ of an interleaved image filters each channel on its own
//     (imgproc/src/pyramids.cpp:746-790: the border tables hold pixel*cn + c)
//   * calcSharrDeriv (:55-144) runs over rows of cols*cn elements whose
//     horizontal neighbours are cn elements apart; per pixel the plane holds
//     (Ix_c, Iy_c) for c = 0..cn-1
//   * LKTrackerInvoker (:178-695) walks the window as winW*cn elements per row
//     (bilinear neighbours cn elements / 2cn derivative values apart), G and b
//     summed over all of them, minEig normalised by 2*winW*winH, the level-0
//     error by 32*winW*cn*winH.
// As for one channel, the G and b sums are formed exactly (int64 lane partials,
// an exact double wave reduction) and rounded to float once: bit-exact with the
// oracle's ORC_ACCUM_EXACT mode (oracle/klt_oracle.c, cn-generic).
// This is not the TBD path (the sample tracks 8-bit gray frames); the kernels
// are straightforward: one thread per element for the pyramid and the planes,
// one wave per point with the window in LDS for the tracker.
#include "lk_walk.hpp"

namespace tbdk {

using lkdev::reflect101_any;

// level 0: the frame into the padded level, reflect-101 frame of `pad` pixels
__global__ __launch_bounds__(256) void pyr_cn_copy_kernel(const uint8_t* __restrict__ img, int pitch, tbdk_level L,
                                                          int cn)
{
    const int ex = blockIdx.x * 256 + threadIdx.x;  // element of the padded row
    const int yp = blockIdx.y;
    const int wp = L.width + 2 * L.pad;
    if (ex >= wp * cn) return;
    const int xp = ex / cn, c = ex - xp * cn;
    const int x = reflect101_any(xp - L.pad, L.width), y = reflect101_any(yp - L.pad, L.height);
    L.data[(size_t)yp * L.pitch + ex] = img[(size_t)y * pitch + (size_t)x * cn + c];
}

// level l+1 from level l: pyrDown_ (5x5 [1 4 6 4 1]^2, (s + 128) >> 8) of the
// isolated level, evaluated at every element of the padded destination (the
// frame at its reflect-101 interior position)
__global__ __launch_bounds__(256) void pyr_cn_down_kernel(tbdk_level S, tbdk_level D, int cn)
{
    const int ex = blockIdx.x * 256 + threadIdx.x;
    const int yp = blockIdx.y;
    const int wp = D.width + 2 * D.pad;
    if (ex >= wp * cn) return;
    const int xp = ex / cn, c = ex - xp * cn;
    const int x = reflect101_any(xp - D.pad, D.width), y = reflect101_any(yp - D.pad, D.height);
    const uint8_t* src = S.data + (size_t)S.pad * S.pitch + (size_t)S.pad * cn + c;
    int cols[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) cols[i] = reflect101_any(2 * x + i - 2, S.width) * cn;
    int r[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t* s = src + (size_t)reflect101_any(2 * y + j - 2, S.height) * S.pitch;
        r[j] = s[cols[2]] * 6 + (s[cols[1]] + s[cols[3]]) * 4 + s[cols[0]] + s[cols[4]];
    }
    const int v = r[2] * 6 + (r[1] + r[3]) * 4 + r[0] + r[4];
    D.data[(size_t)yp * D.pitch + ex] = (uint8_t)((v + 128) >> 8);
}

// calcSharrDeriv over the interior (the zero frame is written at creation)
__global__ __launch_bounds__(256) void scharr_cn_kernel(tbdk_level L, tbdk_level Dv, int cn)
{
    const int ex = blockIdx.x * 256 + threadIdx.x;  // element x*cn + c of an interior row
    const int y = blockIdx.y;
    const int wn = L.width * cn;
    if (ex >= wn) return;
    const int x = ex / cn, c = ex - x * cn;
    const int h = L.height, w = L.width;
    const uint8_t* base = L.data + (size_t)L.pad * L.pitch + (size_t)L.pad * cn + c;
    const uint8_t* s0 = base + (size_t)(y > 0 ? y - 1 : (h > 1 ? 1 : 0)) * L.pitch;
    const uint8_t* s1 = base + (size_t)y * L.pitch;
    const uint8_t* s2 = base + (size_t)(y < h - 1 ? y + 1 : (h > 1 ? h - 2 : 0)) * L.pitch;
    // the row buffers' borders copy column 1 / w-2 (lkpyramid.cpp:111-116)
    const int xl = (x > 0 ? x - 1 : (w > 1 ? 1 : 0)) * cn, xr = (x < w - 1 ? x + 1 : (w > 1 ? w - 2 : 0)) * cn;
    const int xc = x * cn;
    const int t0l = (int16_t)((s0[xl] + s2[xl]) * 3 + s1[xl] * 10), t0r = (int16_t)((s0[xr] + s2[xr]) * 3 + s1[xr] * 10);
    const int t1l = (int16_t)(s2[xl] - s0[xl]), t1c = (int16_t)(s2[xc] - s0[xc]), t1r = (int16_t)(s2[xr] - s0[xr]);
    int16_t* d = reinterpret_cast<int16_t*>(Dv.data + (size_t)(y + Dv.pad) * Dv.pitch) + (size_t)(Dv.pad * cn + ex) * 2;
    d[0] = (int16_t)(t0r - t0l);
    d[1] = (int16_t)((t1r + t1l) * 3 + t1c * 10);
}

namespace {

using namespace lkdev;

// the window policy of lk_walk: one wave per point; LDS: the window's I (x32)
// and interpolated (Ix, Iy), winW*winH*cn elements each, lanes over them
struct CnWin {
    static constexpr float FLT_SCALE = 1.f / (1 << 20);
    const int lane, cn, cn2, winW, winH, wcn, area;
    int16_t* sP;
    int32_t* sG;

    __device__ __forceinline__ CnWin(const LkArgs& a, uint8_t* smem, int lane_)
        : lane(lane_), cn(a.cn), cn2(2 * cn), winW(a.win_w), winH(a.win_h), wcn(winW * cn), area(wcn * winH)
    {
        sP = reinterpret_cast<int16_t*>(smem);
        sG = reinterpret_cast<int32_t*>(smem + align_up(area * 2, 16));
    }

    __device__ __forceinline__ int win_w() const { return winW; }
    __device__ __forceinline__ int win_h() const { return winH; }
    __device__ __forceinline__ bool gate(float, float, int ix, int iy, const LkLevel& L) const
    {
        return out_of_level(ix, iy, winW, winH, L.w, L.h);
    }
    __device__ __forceinline__ void release() const { __syncthreads(); }

    // ---- I patch (x32), interpolated derivatives, G partial sums (exact)
    __device__ __forceinline__ void setup(const LkLevel& L, int ipx, int ipy, float fa, float fb, float& A11,
                                          float& A12, float& A22)
    {
        int iw00, iw01, iw10, iw11;
        bilinear_weights_int(fa, fb, iw00, iw01, iw10, iw11);
        int64_t a11 = 0, a12 = 0, a22 = 0;
        const uint8_t* ib = L.I + (size_t)(ipy + L.ipad) * L.ipitch + (size_t)(ipx + L.ipad) * cn;
        const int dstep = L.dpitch / 2;
        const int16_t* db = reinterpret_cast<const int16_t*>(L.D + (size_t)(ipy + L.dpad) * L.dpitch) +
                            (size_t)(ipx + L.dpad) * cn2;
        for (int p = lane; p < area; p += 64) {
            const int y = p / wcn, x = p - y * wcn;
            const uint8_t* s = ib + (size_t)y * L.ipitch + x;
            const int ival = descale(s[0] * iw00 + s[cn] * iw01 + s[L.ipitch] * iw10 + s[L.ipitch + cn] * iw11,
                                     W_BITS1 - 5);
            const int16_t* d = db + (size_t)y * dstep + 2 * x;
            const int ix = descale(d[0] * iw00 + d[cn2] * iw01 + d[dstep] * iw10 + d[dstep + cn2] * iw11, W_BITS1);
            const int iy = descale(d[1] * iw00 + d[cn2 + 1] * iw01 + d[dstep + 1] * iw10 + d[dstep + cn2 + 1] * iw11,
                                   W_BITS1);
            sP[p] = (int16_t)ival;
            sG[p] = (int32_t)(((uint32_t)(int16_t)ix & 0xffffu) | ((uint32_t)iy << 16));
            a11 += (int64_t)(int16_t)ix * (int16_t)ix;
            a12 += (int64_t)(int16_t)ix * (int16_t)iy;
            a22 += (int64_t)(int16_t)iy * (int16_t)iy;
        }
        A11 = (float)wave_sum_f64((double)a11) * FLT_SCALE;
        A12 = (float)wave_sum_f64((double)a12) * FLT_SCALE;
        A22 = (float)wave_sum_f64((double)a22) * FLT_SCALE;
        __syncthreads();  // sP / sG complete
    }

    // the window's origin in J.  (inx, iny) is wave-uniform: naming it so keeps
    // the window loops' address arithmetic in scalar registers
    __device__ __forceinline__ const uint8_t* j_origin(const LkLevel& L, int inx, int iny) const
    {
        inx = __builtin_amdgcn_readfirstlane(inx);
        iny = __builtin_amdgcn_readfirstlane(iny);
        return L.J + (size_t)(iny + L.jpad) * L.jpitch + (size_t)(inx + L.jpad) * cn;
    }

    // J(x + fa, y + fb) x 32 - I at window element p
    __device__ __forceinline__ int j_diff(const uint8_t* jb, int jpitch, int p, int iw00, int iw01, int iw10,
                                          int iw11) const
    {
        const int y = p / wcn, x = p - y * wcn;
        const uint8_t* q = jb + (size_t)y * jpitch + x;
        const int jv = descale(q[0] * iw00 + q[cn] * iw01 + q[jpitch] * iw10 + q[jpitch + cn] * iw11, W_BITS1 - 5);
        return jv - sP[p];
    }

    __device__ __forceinline__ void step(const LkLevel& L, int inx, int iny, float fa, float fb, float& fb1,
                                         float& fb2) const
    {
        int iw00, iw01, iw10, iw11;
        bilinear_weights_int(fa, fb, iw00, iw01, iw10, iw11);
        const uint8_t* jb = j_origin(L, inx, iny);
        int64_t b1 = 0, b2 = 0;
        for (int p = lane; p < area; p += 64) {
            const int diff = j_diff(jb, L.jpitch, p, iw00, iw01, iw10, iw11);
            const int32_t g = sG[p];
            b1 += (int64_t)diff * (int16_t)g;
            b2 += (int64_t)diff * (g >> 16);
        }
        fb1 = (float)wave_sum_f64((double)b1) * FLT_SCALE;
        fb2 = (float)wave_sum_f64((double)b2) * FLT_SCALE;
    }

    __device__ __forceinline__ float error(const LkLevel& L, int inx, int iny, float fa, float fb) const
    {
        int iw00, iw01, iw10, iw11;
        bilinear_weights_int(fa, fb, iw00, iw01, iw10, iw11);
        const uint8_t* jb = j_origin(L, inx, iny);
        int64_t e = 0;
        for (int p = lane; p < area; p += 64) {
            const int diff = j_diff(jb, L.jpitch, p, iw00, iw01, iw10, iw11);
            const int ad = diff < 0 ? -diff : diff;
            e += ad;
            sG[p] = ad;  // (the derivatives have had their last use: level 0, after the iteration)
        }
        // the reference adds |diff| in a float in window order (lkpyramid.cpp:677-692):
        // the exact sum while that stays within 2^24, where every partial sum is
        // exact; beyond it each addition rounds, and the same chain is run here
        const double esum = wave_sum_f64((double)e);
        float errval = (float)esum;
        if (esum > 16777216.0) {  // block-uniform
            __syncthreads();
            errval = 0.f;
            for (int p = 0; p < area; ++p) errval += (float)sG[p];
        }
        return errval * 1.f / (float)(32 * winW * cn * winH);
    }
};

}  // namespace

__global__ __launch_bounds__(64) void lk_cn_kernel(LkArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int i = seg_point(a, xcd_swizzle(blockIdx.x, gridDim.x));
    if (i < 0) return;
    CnWin win(a, smem, threadIdx.x);
    lk_walk_point(a, i, threadIdx.x == 0, win);
}

size_t lk_cn_smem_bytes(int win_w, int win_h, int cn)
{
    const size_t area = (size_t)win_w * win_h * cn;
    return align_up((int)(area * 2), 16) + area * 4;
}

hipError_t launch_pyr_cn(const uint8_t* img, int pitch, const tbdk_pyr& pyr, hipStream_t s)
{
    const int cn = pyr.cn;
    for (int l = 0; l < pyr.nlevels; ++l) {
        const tbdk_level& L = pyr.lv[l];
        const dim3 grid(((L.width + 2 * L.pad) * cn + 255) / 256, L.height + 2 * L.pad);
        if (l == 0) hipLaunchKernelGGL(pyr_cn_copy_kernel, grid, dim3(256), 0, s, img, pitch, L, cn);
        else hipLaunchKernelGGL(pyr_cn_down_kernel, grid, dim3(256), 0, s, pyr.lv[l - 1], L, cn);
        if (pyr.dv[l].data)
            hipLaunchKernelGGL(scharr_cn_kernel, dim3((L.width * cn + 255) / 256, L.height), dim3(256), 0, s, L,
                               pyr.dv[l], cn);
    }
    return hipGetLastError();
}

hipError_t launch_lk_cn(const LkArgs& a, hipStream_t s)
{
    const size_t smem = lk_cn_smem_bytes(a.win_w, a.win_h, a.cn);
    // > 64 KiB of LDS (large windows x 4 channels) must be opted into
    static std::atomic<unsigned long long> opted{0};
    if (smem > 64 * 1024) {
        const hipError_t e = lds_opt_in(opted, {reinterpret_cast<const void*>(&lk_cn_kernel)}, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lk_cn_kernel, dim3(a.n), dim3(64), smem, s, a);
    return hipGetLastError();
}

}  // namespace tbdk
