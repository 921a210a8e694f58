// facade_klt_tracker_check.cpp — compiles the C++ facade's KLT point tracker
// (include/tbdk.hpp: tbdk::KltTracker) against libtbdk.so.  Exit code 0 = pass.
//   no GPU : Context throws tbdk::Error(TBDK_ENODEV)
//   GPU    : facade_klt_tracker_check gpu <cfg.bin> <frames.u8> <nframes> <prefix>:
//            a tracker of the configuration (a raw tbdk_klt_tracker_config) stepped
//            over the frames (raw 8-bit rows, width x height each) reads exactly
//            what the Python binding read: <prefix>.ids / .lens (int32), .last /
//            .hist (float32) and .stats (the seven int32 of tbdk_klt_tracker_stats);
//            the same again after reset()
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "tbdk.hpp"

namespace {

template <typename T>
std::vector<T> slurp(const std::string& path)
{
    std::vector<T> v;
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        std::fseek(f, 0, SEEK_END);
        const long n = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        v.resize(n > 0 ? (size_t)n / sizeof(T) : 0);
        if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) v.clear();
        std::fclose(f);
    }
    return v;
}

template <typename T>
bool same(const std::vector<T>& a, const std::vector<T>& b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

}  // namespace

int main(int argc, char** argv)
{
    const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        tbdk::Context ctx(0);
        if (!want_gpu) return 3;  // a context without a GPU must not exist
        if (argc != 6) return 2;
        const std::vector<uint8_t> raw = slurp<uint8_t>(argv[2]);
        if (raw.size() != sizeof(tbdk_klt_tracker_config)) return 2;
        tbdk_klt_tracker_config cfg;
        std::memcpy(&cfg, raw.data(), sizeof(cfg));
        const tbdk_klt_tracker_config def = tbdk::KltTracker::defaultConfig(cfg.width, cfg.height);
        if (def.win != 15 || def.track_len != 10 || def.max_tracks != 8192 || def.width != cfg.width) return 8;
        const int nframes = std::atoi(argv[4]);
        const std::vector<uint8_t> frames = slurp<uint8_t>(argv[3]);
        const size_t fsz = (size_t)cfg.width * cfg.height;
        if (nframes <= 0 || frames.size() != fsz * nframes) return 2;
        const std::string pre = argv[5];
        const std::vector<int32_t> ids = slurp<int32_t>(pre + ".ids"), lens = slurp<int32_t>(pre + ".lens"),
                                   stats = slurp<int32_t>(pre + ".stats");
        const std::vector<float> last = slurp<float>(pre + ".last"), hist = slurp<float>(pre + ".hist");
        if (ids.empty() || stats.size() != 7) return 2;
        uint8_t* d8 = nullptr;
        if (hipMalloc(&d8, frames.size())) return 4;
        (void)hipMemcpy(d8, frames.data(), frames.size(), hipMemcpyHostToDevice);
        tbdk::KltTracker tr(ctx, cfg);
        for (int pass = 0; pass < 2; ++pass) {
            for (int f = 0; f < nframes; ++f) tr.step(tbdk::GpuImage{d8 + fsz * f, cfg.width, cfg.height, cfg.width});
            const tbdk::KltTracker::State s = tr.read();
            std::printf("pass %d: %zu tracks (expected %zu), next id %d\n", pass, s.size(), ids.size(), s.stats.next_id);
            if (!same(s.ids, ids) || !same(s.lens, lens)) return 6;
            if (!same(s.lastPts, last) || !same(s.hist, hist)) return 7;
            if (std::memcmp(&s.stats, stats.data(), sizeof(s.stats)) != 0) return 9;
            tr.reset();
            if (tr.read().size() != 0) return 10;
        }
        return 0;
    } catch (const tbdk::Error& e) {
        std::printf("tbdk::Error: %s\n", e.what());
        return (!want_gpu && e.code() == TBDK_ENODEV) ? 0 : 5;
    }
}
