// pnm_reader.hpp — binary PNM (P5 gray / P6 colour, maxval 255) header parsing
// for the image-sequence driver (tbd_detect.hip).  Host C++ only, no HIP, so
// that it can be checked alone (tests/cpp/pnm_reader_check.cpp).
//
// A header is: magic, width, height, maxval as decimal text separated by
// white space, with '#' comments running to the end of a line anywhere in
// between, then exactly one white-space byte, then width * height * channels
// bytes.  Every read is bounded by the length given.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace tbdk {

enum PnmStatus {
    kPnmOk = 0,
    kPnmBadMagic = -1,   // not "P5" / "P6"
    kPnmBadHeader = -2,  // header cut short or not a number where one must be
    kPnmBadSize = -3,    // zero, or more than kPnmMaxDim
    kPnmBadMaxval = -4,  // only 255 is read
    kPnmTruncated = -5,  // fewer body bytes than width * height * channels
    kPnmNoFile = -6,     // pnm_read_file / pnm_check_file: cannot open or read
};

constexpr int kPnmMaxDim = 1 << 15;

struct PnmInfo {
    int width = 0, height = 0, cn = 0;  // cn: 1 (P5) or 3 (P6, RGB order)
    size_t offset = 0;                  // first body byte
    size_t body() const { return (size_t)width * (size_t)height * (size_t)cn; }
};

namespace pnm_detail {

inline bool is_space(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }

// skips white space and comments; false at the end of the buffer
inline bool skip_blank(const uint8_t* p, size_t len, size_t& i)
{
    while (i < len) {
        if (is_space(p[i])) {
            ++i;
        } else if (p[i] == '#') {
            while (i < len && p[i] != '\n' && p[i] != '\r') ++i;
        } else {
            return true;
        }
    }
    return false;
}

// a decimal number of at most 9 digits, followed by at least one more byte
inline bool read_uint(const uint8_t* p, size_t len, size_t& i, int& out)
{
    if (!skip_blank(p, len, i)) return false;
    int v = 0, nd = 0;
    while (i < len && p[i] >= '0' && p[i] <= '9') {
        if (++nd > 9) return false;
        v = v * 10 + (p[i] - '0');
        ++i;
    }
    if (nd == 0 || i >= len) return false;
    out = v;
    return true;
}

}  // namespace pnm_detail

// the header alone: buf holds at least the header (len bytes are readable)
inline int pnm_parse_header(const uint8_t* buf, size_t len, PnmInfo* info)
{
    using namespace pnm_detail;
    if (!buf || !info || len < 2 || buf[0] != 'P' || (buf[1] != '5' && buf[1] != '6')) return kPnmBadMagic;
    PnmInfo r;
    r.cn = buf[1] == '5' ? 1 : 3;
    size_t i = 2;
    if (i >= len || !(is_space(buf[i]) || buf[i] == '#')) return kPnmBadHeader;
    int maxval = 0;
    if (!read_uint(buf, len, i, r.width) || !read_uint(buf, len, i, r.height) || !read_uint(buf, len, i, maxval))
        return kPnmBadHeader;
    if (!is_space(buf[i])) return kPnmBadHeader;  // read_uint left i < len
    r.offset = i + 1;
    if (r.width <= 0 || r.height <= 0 || r.width > kPnmMaxDim || r.height > kPnmMaxDim) return kPnmBadSize;
    if (maxval != 255) return kPnmBadMaxval;
    *info = r;
    return kPnmOk;
}

// a whole file image in memory: header and body length
inline int pnm_parse(const uint8_t* buf, size_t len, PnmInfo* info)
{
    PnmInfo r;
    const int rc = pnm_parse_header(buf, len, &r);
    if (rc != kPnmOk) return rc;
    if (len - r.offset < r.body()) return kPnmTruncated;  // offset <= len
    *info = r;
    return kPnmOk;
}

// header and size of a file, without reading its body
inline int pnm_check_file(const std::string& path, PnmInfo* info)
{
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return kPnmNoFile;
    uint8_t head[1024];
    const size_t got = std::fread(head, 1, sizeof(head), f);
    long size = -1;
    if (std::fseek(f, 0, SEEK_END) == 0) size = std::ftell(f);
    std::fclose(f);
    if (size < 0) return kPnmNoFile;
    PnmInfo r;
    const int rc = pnm_parse_header(head, got, &r);
    if (rc != kPnmOk) return rc;
    if ((size_t)size < r.offset || (size_t)size - r.offset < r.body()) return kPnmTruncated;
    *info = r;
    return kPnmOk;
}

// the whole file into buf, parsed
inline int pnm_read_file(const std::string& path, std::vector<uint8_t>& buf, PnmInfo* info)
{
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return kPnmNoFile;
    long size = -1;
    if (std::fseek(f, 0, SEEK_END) == 0) size = std::ftell(f);
    if (size < 0 || std::fseek(f, 0, SEEK_SET) != 0) {
        std::fclose(f);
        return kPnmNoFile;
    }
    buf.resize((size_t)size);
    const size_t got = size ? std::fread(buf.data(), 1, (size_t)size, f) : 0;
    std::fclose(f);
    if (got != (size_t)size) return kPnmNoFile;
    return pnm_parse(buf.data(), buf.size(), info);
}

}  // namespace tbdk
