// rigid_transform_driver.cpp — records cv::estimateRigidTransform on point sets
// for tests/golden/rigid_transform_cases.npz (see tools/record_rigid_cases.md).
// Links against a scratch build of the reference's core, imgproc and video
// modules; nothing in the test suite builds or runs it.
//
// stdin : ncases, then per case: n max_iters good_ratio, then n lines "ax ay bx by"
//         (floats printed with 9 significant digits, which round-trip)
// stdout: per case: found m0 m1 m2 m3 m4 m5 (17 significant digits)
#include <cstdio>
#include <vector>

#include <opencv2/core.hpp>
#include <opencv2/video/tracking.hpp>

int main()
{
    int ncases = 0;
    if (std::scanf("%d", &ncases) != 1) return 1;
    for (int c = 0; c < ncases; ++c) {
        int n = 0, max_iters = 0;
        double ratio = 0.0;
        if (std::scanf("%d %d %lf", &n, &max_iters, &ratio) != 3) return 1;
        std::vector<cv::Point2f> a(n), b(n);
        for (int i = 0; i < n; ++i)
            if (std::scanf("%f %f %f %f", &a[i].x, &a[i].y, &b[i].x, &b[i].y) != 4) return 1;
        cv::Mat M;
        try {
            M = cv::estimateRigidTransform(a, b, false, max_iters, ratio, 3);
        } catch (const cv::Exception&) {  // n == 0: checkVector fails; recorded as no transform
            M = cv::Mat();
        }
        if (M.empty()) {
            std::printf("0 0 0 0 0 0 0\n");
        } else {
            const double* m = M.ptr<double>();
            std::printf("1 %.17g %.17g %.17g %.17g %.17g %.17g\n", m[0], m[1], m[2], m[3], m[4], m[5]);
        }
    }
    return 0;
}
