// pnm_reader_check.cpp — opencv_amd/csrc/pnm_reader.hpp alone, host-built with
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_pnm_reader.py).
// Every input lives in a heap block of exactly its length, so a read past the
// buffer is an ASan report; every prefix of every input is parsed as well.
//   pnm_reader_check <scratch dir>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pnm_reader.hpp"

using namespace tbdk;

static int g_fail = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);            \
            ++g_fail;                                                   \
        }                                                               \
    } while (0)

static int parse_exact(const std::string& s, PnmInfo* info)
{
    std::unique_ptr<uint8_t[]> p(new uint8_t[s.size() ? s.size() : 1]);
    std::memcpy(p.get(), s.data(), s.size());
    return pnm_parse(p.get(), s.size(), info);
}

static std::string body(size_t n)
{
    std::string b(n, '\0');
    for (size_t i = 0; i < n; ++i) b[i] = (char)(i * 37 + 11);
    return b;
}

static void write_file(const std::string& path, const std::string& s)
{
    std::FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return;
    std::fwrite(s.data(), 1, s.size(), f);
    std::fclose(f);
}

int main(int argc, char** argv)
{
    PnmInfo pi;
    // valid P5 / P6
    const std::string p5 = "P5\n4 3\n255\n" + body(12);
    CHECK(parse_exact(p5, &pi) == kPnmOk && pi.width == 4 && pi.height == 3 && pi.cn == 1 && pi.offset == 11);
    const std::string p6 = "P6 5 2 255 " + body(30);
    CHECK(parse_exact(p6, &pi) == kPnmOk && pi.width == 5 && pi.height == 2 && pi.cn == 3 && pi.offset == 11);
    CHECK(std::memcmp(p6.data() + pi.offset, body(30).data(), 30) == 0);
    // a body byte that looks like white space or '#' is body
    CHECK(parse_exact("P5\n1 1\n255\n#", &pi) == kPnmOk && pi.offset == 11);
    CHECK(parse_exact("P5\n1 1\n255\n\n", &pi) == kPnmOk && pi.offset == 11);
    // comments anywhere in the header, CR LF line ends, trailing bytes after the body
    const std::string cm = "P6# made by a test\n# second line\n 2 # width\r\n\t3\n#maxval next\n255\n" + body(18) + "tail";
    CHECK(parse_exact(cm, &pi) == kPnmOk && pi.width == 2 && pi.height == 3 && pi.cn == 3);
    CHECK(cm.compare(pi.offset, 18, body(18)) == 0);
    // truncated body (one byte short, and none at all)
    CHECK(parse_exact(p5.substr(0, p5.size() - 1), &pi) == kPnmTruncated);
    CHECK(parse_exact("P6\n5 2\n255\n", &pi) == kPnmTruncated);
    // truncated header
    CHECK(parse_exact("P5\n4 3\n255", &pi) == kPnmBadHeader);  // no separator after maxval
    CHECK(parse_exact("P5\n4 3\n", &pi) == kPnmBadHeader);
    CHECK(parse_exact("P5\n4 # never ends", &pi) == kPnmBadHeader);
    CHECK(parse_exact("P5", &pi) == kPnmBadHeader);
    CHECK(parse_exact("P5\n4 x\n255\n" + body(12), &pi) == kPnmBadHeader);
    CHECK(parse_exact("P5\n-4 3\n255\n" + body(12), &pi) == kPnmBadHeader);
    CHECK(parse_exact("P54 3\n255\n" + body(12), &pi) == kPnmBadHeader);  // magic not separated
    CHECK(parse_exact("P5\n4 3\n255x" + body(12), &pi) == kPnmBadHeader);
    CHECK(parse_exact("P5\n12345678901 3\n255\n", &pi) == kPnmBadHeader);  // overlong number
    // maxval != 255
    CHECK(parse_exact("P5\n4 3\n65535\n" + body(24), &pi) == kPnmBadMaxval);
    CHECK(parse_exact("P5\n4 3\n254\n" + body(12), &pi) == kPnmBadMaxval);
    CHECK(parse_exact("P5\n4 3\n0\n" + body(12), &pi) == kPnmBadMaxval);
    // wrong magic
    CHECK(parse_exact("P4\n4 3\n" + body(3), &pi) == kPnmBadMagic);
    CHECK(parse_exact("P3\n1 1\n255\n1 2 3\n", &pi) == kPnmBadMagic);
    CHECK(parse_exact("\x89PNG\r\n", &pi) == kPnmBadMagic);
    CHECK(parse_exact("P", &pi) == kPnmBadMagic);
    CHECK(parse_exact("", &pi) == kPnmBadMagic);
    CHECK(pnm_parse(nullptr, 0, &pi) == kPnmBadMagic);
    // zero and oversized sizes
    CHECK(parse_exact("P5\n0 3\n255\n", &pi) == kPnmBadSize);
    CHECK(parse_exact("P5\n4 0\n255\n", &pi) == kPnmBadSize);
    CHECK(parse_exact("P6\n40000 1\n255\n", &pi) == kPnmBadSize);
    CHECK(parse_exact("P6\n999999999 999999999\n255\n", &pi) == kPnmBadSize);
    // a large claimed size with a short body: no overflow, no read
    CHECK(parse_exact("P6\n32768 32768\n255\nabc", &pi) == kPnmTruncated);
    // every prefix of the valid inputs: parsed without leaving the buffer, and only the whole is accepted
    for (const std::string* s : {&p5, &p6}) {
        for (size_t n = 0; n < s->size(); ++n) CHECK(parse_exact(s->substr(0, n), &pi) != kPnmOk);
    }
    for (size_t n = 0; n <= cm.size(); ++n) (void)parse_exact(cm.substr(0, n), &pi);
    // a failed parse leaves *info alone
    pi = PnmInfo();
    pi.width = 7;
    CHECK(parse_exact("P5\n4 3\n255\n", &pi) == kPnmTruncated && pi.width == 7);

    // the file forms
    if (argc > 1) {
        const std::string dir = std::string(argv[1]) + "/";
        std::vector<uint8_t> buf;
        write_file(dir + "ok.ppm", p6);
        CHECK(pnm_check_file(dir + "ok.ppm", &pi) == kPnmOk && pi.width == 5 && pi.height == 2 && pi.cn == 3);
        CHECK(pnm_read_file(dir + "ok.ppm", buf, &pi) == kPnmOk && buf.size() == p6.size() && pi.offset == 11);
        write_file(dir + "short.pgm", p5.substr(0, p5.size() - 2));
        CHECK(pnm_check_file(dir + "short.pgm", &pi) == kPnmTruncated);
        CHECK(pnm_read_file(dir + "short.pgm", buf, &pi) == kPnmTruncated);
        write_file(dir + "empty.pgm", "");
        CHECK(pnm_check_file(dir + "empty.pgm", &pi) == kPnmBadMagic);
        CHECK(pnm_read_file(dir + "empty.pgm", buf, &pi) == kPnmBadMagic);
        // a header longer than the checker's first read, and a body far past it
        const std::string big = "P5\n" + std::string(600, ' ') + "40 50\n255\n" + body(2000);
        write_file(dir + "big.pgm", big);
        CHECK(pnm_check_file(dir + "big.pgm", &pi) == kPnmOk && pi.width == 40 && pi.height == 50);
        CHECK(pnm_read_file(dir + "big.pgm", buf, &pi) == kPnmOk);
        CHECK(pnm_check_file(dir + "none.pgm", &pi) == kPnmNoFile);
        CHECK(pnm_read_file(dir + "none.pgm", buf, &pi) == kPnmNoFile);
    }
    if (g_fail) return 1;
    std::printf("pnm reader ok\n");
    return 0;
}
