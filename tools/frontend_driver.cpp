// frontend_driver.cpp — records cv::cvtColor and cv::resize(INTER_LINEAR) on raw
// 8-bit images for tests/golden/frontend_cases.npz (see tools/record_frontend_cases.md).
// Links against a scratch build of the reference's core and imgproc modules;
// nothing in the test suite builds or runs it.
//
//   frontend_driver cvt    <in.raw> <w> <h> <cn> <code>     <out.raw>
//   frontend_driver resize <in.raw> <w> <h> <cn> <dw> <dh>  <out.raw>
//
// in.raw / out.raw: tightly packed rows of interleaved u8 pixels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <opencv2/core.hpp>
#include <opencv2/imgproc.hpp>

static bool read_all(const char* path, std::vector<unsigned char>& buf, size_t n)
{
    buf.resize(n);
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(buf.data(), 1, n, f);
    std::fclose(f);
    return got == n;
}

int main(int argc, char** argv)
{
    if (argc < 8) return 2;
    const bool is_resize = std::strcmp(argv[1], "resize") == 0;
    if (is_resize != (argc == 9)) return 2;
    const int w = std::atoi(argv[3]), h = std::atoi(argv[4]), cn = std::atoi(argv[5]);
    std::vector<unsigned char> in;
    if (!read_all(argv[2], in, (size_t)w * h * cn)) return 3;
    cv::Mat src(h, w, CV_8UC(cn), in.data()), dst;
    if (is_resize)
        cv::resize(src, dst, cv::Size(std::atoi(argv[6]), std::atoi(argv[7])), 0, 0, cv::INTER_LINEAR);
    else
        cv::cvtColor(src, dst, std::atoi(argv[6]));
    if (!dst.isContinuous()) dst = dst.clone();
    FILE* f = std::fopen(argv[argc - 1], "wb");
    if (!f) return 4;
    const size_t n = dst.total() * dst.elemSize();
    const bool ok = std::fwrite(dst.data, 1, n, f) == n;
    std::fclose(f);
    return ok ? 0 : 4;
}
