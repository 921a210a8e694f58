// klt_lk_body.inc -- the body of the one-point-per-wave PyrLK kernels
// (klt_lk.hip), included once by each __global__ kernel that shares it.  The
// including kernel provides: BACK (compile-time constant), `a` (LkArgs) and
// `bk` (LkBack; read only when BACK).
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int i = seg_point(a, xcd_swizzle(blockIdx.x, gridDim.x));
    if (i < 0) return;
    const int lane = threadIdx.x;
    const int winW = a.win_w, winH = a.win_h, area = winW * winH;
    const int SW = winW + 3, SH = winH + 3, DW = winW + 1;
    uint8_t* sI = smem;
    int32_t* sD = reinterpret_cast<int32_t*>(smem + align_up(SW * SH, 16));
    int16_t* sP = reinterpret_cast<int16_t*>(reinterpret_cast<uint8_t*>(sD) + align_up(DW * (winH + 1) * 4, 16));
    int32_t* sG = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(sP) + align_up(area * 2, 16));

    const int W_BITS = 14, W_BITS1 = 14;
    const float FLT_SCALE = 1.f / (1 << 20);
    const float halfx = (winW - 1) * 0.5f, halfy = (winH - 1) * 0.5f;
    float p0x = a.prev_pts[2 * i], p0y = a.prev_pts[2 * i + 1];
    const float o0x = p0x, o0y = p0y;  // BACK: the forward pass's start, p0 being its result
    if constexpr (BACK) {
        if (!a.status[i]) {  // lost by the forward pass: takes no part (block-uniform)
            if (lane == 0) {
                if (bk.back_pts) {
                    bk.back_pts[2 * i] = o0x;
                    bk.back_pts[2 * i + 1] = o0y;
                }
                if (bk.fb_err) bk.fb_err[i] = __builtin_inff();
            }
            return;
        }
        p0x = a.next_pts[2 * i];
        p0y = a.next_pts[2 * i + 1];
    }
    float outx = 0.f, outy = 0.f;
    if ((BACK ? 0 : a.flags) & TBDK_OPTFLOW_USE_INITIAL_FLOW) {
        outx = a.next_pts[2 * i];
        outy = a.next_pts[2 * i + 1];
    }
    int status = 1, nit = 0;
    float errv = 0.f;

    // lane -> patch pixel mapping (p = lane + 64k)
    const int qx = 64 % winW, qy = 64 / winW;
    const int lx0 = lane % winW, ly0 = lane / winW;
    const int dq = 64 % DW, dqy = 64 / DW;
    const int dx0 = lane % DW, dy0 = lane / DW;
    const int sq = 64 % SW, sqy = 64 / SW;
    const int sx0 = lane % SW, sy0 = lane / SW;

    for (int level = a.max_level; level >= 0; --level) {
        const LkLevel L = a.lv[level];
        const float sc = (float)(1. / (1 << level));
        float prevx = p0x * sc, prevy = p0y * sc;
        float nextx, nexty;
        if (level == a.max_level) {
            if ((BACK ? 0 : a.flags) & TBDK_OPTFLOW_USE_INITIAL_FLOW) {
                nextx = outx * sc;
                nexty = outy * sc;
            } else {
                nextx = prevx;
                nexty = prevy;
            }
        } else {
            nextx = outx * 2.f;
            nexty = outy * 2.f;
        }
        outx = nextx;
        outy = nexty;

        prevx -= halfx;
        prevy -= halfy;
        const int ipx = (int)floorf(prevx), ipy = (int)floorf(prevy);
        if (ipx < -winW || ipx >= L.w || ipy < -winH || ipy >= L.h) {
            if (level == 0) {
                status = 0;
                errv = 0.f;
            }
            continue;
        }
        float fa = prevx - ipx, fb = prevy - ipy;
        int iw00 = round_even((1.f - fa) * (1.f - fb) * (1 << W_BITS));
        int iw01 = round_even(fa * (1.f - fb) * (1 << W_BITS));
        int iw10 = round_even((1.f - fa) * fb * (1 << W_BITS));
        int iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;

        // ---- stage the (win+3)^2 u8 window of I starting at (ipx-1, ipy-1)
        {
            const uint8_t* base = L.I + (size_t)(ipy - 1 + L.ipad) * L.ipitch + (ipx - 1 + L.ipad);
            int sx = sx0, sy = sy0;
            for (int p = lane; p < SW * SH; p += 64) {
                sI[p] = base[(size_t)sy * L.ipitch + sx];
                sx += sq;
                sy += sqy;
                if (sx >= SW) {
                    sx -= SW;
                    sy += 1;
                }
            }
        }
        __syncthreads();
        // ---- Scharr derivatives on the (win+1)^2 grid; 0 outside the level
        {
            int dx = dx0, dy = dy0;
            for (int p = lane; p < DW * (winH + 1); p += 64) {
                const int X = ipx + dx, Y = ipy + dy;
                int32_t packed = 0;
                if (X >= 0 && X < L.w && Y >= 0 && Y < L.h) {
                    const uint8_t* r0 = sI + dy * SW + dx;  // row Y-1, col X-1
                    const uint8_t* r1 = r0 + SW;
                    const uint8_t* r2 = r1 + SW;
                    const int t0l = (r0[0] + r2[0]) * 3 + r1[0] * 10;
                    const int t0r = (r0[2] + r2[2]) * 3 + r1[2] * 10;
                    const int t1l = r2[0] - r0[0], t1c = r2[1] - r0[1], t1r = r2[2] - r0[2];
                    const int ix = t0r - t0l;
                    const int iy = (t1r + t1l) * 3 + t1c * 10;
                    packed = (int32_t)(((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16));
                }
                sD[p] = packed;
                dx += dq;
                dy += dqy;
                if (dx >= DW) {
                    dx -= DW;
                    dy += 1;
                }
            }
        }
        __syncthreads();
        // ---- I patch (x32), interpolated derivatives, G partial sums
        int a11 = 0, a12 = 0, a22 = 0;
        {
            int px = lx0, py = ly0;
            for (int p = lane; p < area; p += 64) {
                const uint8_t* s = sI + (py + 1) * SW + (px + 1);
                const int ival = descale(s[0] * iw00 + s[1] * iw01 + s[SW] * iw10 + s[SW + 1] * iw11, W_BITS1 - 5);
                const int32_t* d = sD + py * DW + px;
                const int32_t d00 = d[0], d01 = d[1], d10 = d[DW], d11 = d[DW + 1];
                const int ix = descale((int16_t)d00 * iw00 + (int16_t)d01 * iw01 + (int16_t)d10 * iw10 +
                                           (int16_t)d11 * iw11, W_BITS1);
                const int iy = descale((d00 >> 16) * iw00 + (d01 >> 16) * iw01 + (d10 >> 16) * iw10 +
                                           (d11 >> 16) * iw11, W_BITS1);
                sP[p] = (int16_t)ival;
                sG[p] = (int32_t)(((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16));
                a11 += ix * ix;
                a12 += ix * iy;
                a22 += iy * iy;
                px += qx;
                py += qy;
                if (px >= winW) {
                    px -= winW;
                    py += 1;
                }
            }
        }
        const float A11 = (float)wave_sum((double)a11) * FLT_SCALE;
        const float A12 = (float)wave_sum((double)a12) * FLT_SCALE;
        const float A22 = (float)wave_sum((double)a22) * FLT_SCALE;

        float D = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) /
                             (float)(2 * winW * winH);
        if ((BACK ? 0 : a.flags) & TBDK_OPTFLOW_LK_GET_MIN_EIGENVALS) errv = minEig;
        if (minEig < a.min_eig || D < 1.19209290e-07F /*FLT_EPSILON*/) {
            if (level == 0) status = 0;
            __syncthreads();
            continue;
        }
        D = 1.f / D;

        nextx -= halfx;
        nexty -= halfy;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < a.max_count; ++j) {
            const int inx = (int)floorf(nextx), iny = (int)floorf(nexty);
            if (inx < -winW || inx >= L.w || iny < -winH || iny >= L.h) {
                if (level == 0) status = 0;
                break;
            }
            nit++;
            fa = nextx - inx;
            fb = nexty - iny;
            iw00 = round_even((1.f - fa) * (1.f - fb) * (1 << W_BITS));
            iw01 = round_even(fa * (1.f - fb) * (1 << W_BITS));
            iw10 = round_even((1.f - fa) * fb * (1 << W_BITS));
            iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
            const uint8_t* jb = L.J + (size_t)(iny + L.jpad) * L.jpitch + (inx + L.jpad);
            int b1 = 0, b2 = 0;
            int px = lx0, py = ly0;
            for (int p = lane; p < area; p += 64) {
                const uint8_t* q = jb + (size_t)py * L.jpitch + px;
                const int jv = descale(q[0] * iw00 + q[1] * iw01 + q[L.jpitch] * iw10 + q[L.jpitch + 1] * iw11,
                                       W_BITS1 - 5);
                const int diff = jv - sP[p];
                const int32_t g = sG[p];
                b1 += diff * (int16_t)g;
                b2 += diff * (g >> 16);
                px += qx;
                py += qy;
                if (px >= winW) {
                    px -= winW;
                    py += 1;
                }
            }
            const float fb1 = (float)wave_sum((double)b1) * FLT_SCALE;
            const float fb2 = (float)wave_sum((double)b2) * FLT_SCALE;
            const float ddx = (A12 * fb2 - A22 * fb1) * D;
            const float ddy = (A12 * fb1 - A11 * fb2) * D;
            nextx += ddx;
            nexty += ddy;
            outx = nextx + halfx;
            outy = nexty + halfy;
            if ((double)ddx * ddx + (double)ddy * ddy <= a.eps2) break;
            if (j > 0 && (double)fabsf(ddx + pdx) < 0.01 && (double)fabsf(ddy + pdy) < 0.01) {
                outx -= ddx * 0.5f;
                outy -= ddy * 0.5f;
                break;
            }
            pdx = ddx;
            pdy = ddy;
        }

        if (!BACK && level == 0 && status && a.err && ((BACK ? 0 : a.flags) & TBDK_OPTFLOW_LK_GET_MIN_EIGENVALS) == 0) {
            const float npx = outx - halfx, npy = outy - halfy;
            const int inx = (int)floorf(npx), iny = (int)floorf(npy);
            if (inx < -winW || inx >= L.w || iny < -winH || iny >= L.h) {
                status = 0;
            } else {
                const float aa = npx - inx, bb = npy - iny;
                iw00 = round_even((1.f - aa) * (1.f - bb) * (1 << W_BITS));
                iw01 = round_even(aa * (1.f - bb) * (1 << W_BITS));
                iw10 = round_even((1.f - aa) * bb * (1 << W_BITS));
                iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
                const uint8_t* jb = L.J + (size_t)(iny + L.jpad) * L.jpitch + (inx + L.jpad);
                int e = 0;
                int px = lx0, py = ly0;
                for (int p = lane; p < area; p += 64) {
                    const uint8_t* q = jb + (size_t)py * L.jpitch + px;
                    const int jv = descale(q[0] * iw00 + q[1] * iw01 + q[L.jpitch] * iw10 + q[L.jpitch + 1] * iw11,
                                           W_BITS1 - 5);
                    const int diff = jv - sP[p];
                    const int ad = diff < 0 ? -diff : diff;
                    e += ad;
                    sG[p] = ad;  // (the derivatives have had their last use: level 0, after the iteration)
                    px += qx;
                    py += qy;
                    if (px >= winW) {
                        px -= winW;
                        py += 1;
                    }
                }
                // the reference adds |diff| in a float in window order (lkpyramid.cpp:677-692):
                // the exact sum while that stays within 2^24, where every partial sum is
                // exact; beyond it each addition rounds, and the same chain is run here
                const double esum = wave_sum((double)e);
                float errval = (float)esum;
                if (esum > 16777216.0) {  // block-uniform
                    __syncthreads();
                    errval = 0.f;
                    for (int p = 0; p < area; ++p) errval += (float)sG[p];
                }
                errv = errval * 1.f / (float)(32 * winW * winH);
            }
        }
        __syncthreads();  // LDS is rewritten by the next level
    }

    if constexpr (BACK) {
        if (lane == 0) {
            const float dx = fabsf(o0x - outx), dy = fabsf(o0y - outy);
            const float d = fmaxf(dx, dy);
            if (bk.back_pts) {
                bk.back_pts[2 * i] = outx;
                bk.back_pts[2 * i + 1] = outy;
            }
            if (bk.fb_err) bk.fb_err[i] = status ? d : __builtin_inff();
            if (!(status && d < bk.thr)) a.status[i] = 0;
        }
        return;
    }
    if (lane == 0) {
        a.next_pts[2 * i] = outx;
        a.next_pts[2 * i + 1] = outy;
        a.status[i] = (uint8_t)status;
        if (a.err) a.err[i] = errv;
        if (a.iters) a.iters[i] = nit;
    }
