// The host LZW encoder of the GeoTIFF writer (unet_amd/csrc/tiff_codecs.hip) under AddressSanitizer / UBSan: CPU build only, compiled and
// run by tests/test_tiff_encode_cpu.py.  Random, run-heavy and two-valued buffers of random length are encoded into heap buffers of
// EXACTLY unet_tiff_lzw_cap(n) bytes (so one byte too many is a heap overflow the sanitizer sees), decoded back and compared; then encoded
// into cap - k bytes for an incompressible buffer, where the encoder must return -1 without touching anything behind the buffer.
//   tiff_encode_fuzz <iterations> <seed>    prints: encoded N refused N
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" long long unet_tiff_lzw_cap(long long n);
extern "C" long long unet_tiff_lzw_encode(const unsigned char* src, long long n, unsigned char* dst, long long cap);
extern "C" long long unet_tiff_lzw_decode(const unsigned char* src, long long n, unsigned char* dst, long long cap);

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (uint32_t)(state >> 16); }

static void fill(std::vector<unsigned char>& v, int kind) {
    if (kind == 0) {                                   // random: incompressible, the table fills and Clear goes out mid-strip
        for (auto& b : v) b = (unsigned char)rnd();
    } else if (kind == 1) {                            // runs of random length: long strings
        size_t i = 0;
        while (i < v.size()) {
            const unsigned char c = (unsigned char)(rnd() % 5);
            size_t run = 1 + rnd() % 700;
            while (run-- && i < v.size()) v[i++] = c;
        }
    } else {                                           // two values, mostly alternating
        for (size_t i = 0; i < v.size(); ++i) v[i] = (unsigned char)(((i & 1) ^ (rnd() % 17 == 0)) ? 200 : 3);
    }
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 300;
    if (argc > 2) state ^= (uint64_t)atoll(argv[2]) * 0x2545F4914F6CDD1Dull;
    long encoded = 0, refused = 0;
    for (int it = 0; it < iters; ++it) {
        const int kind = it % 3;
        const uint32_t r = rnd() % 8;
        const size_t n = r == 0 ? rnd() % 40 : r < 6 ? rnd() % 5000 : rnd() % 70000;
        std::vector<unsigned char> src(n);
        fill(src, kind);
        const long long cap = unet_tiff_lzw_cap((long long)n);
        unsigned char* dst = (unsigned char*)malloc((size_t)cap);          // exactly cap bytes: the sanitizer guards byte cap
        const long long got = unet_tiff_lzw_encode(src.data(), (long long)n, dst, cap);
        if (got < 2 || got > cap) { fprintf(stderr, "encode of %zu bytes (kind %d) returned %lld, cap %lld\n", n, kind, got, cap); return 1; }
        unsigned char* back = (unsigned char*)malloc(n ? n : 1);
        const long long m = unet_tiff_lzw_decode(dst, got, back, (long long)n);
        if (m != (long long)n || (n && memcmp(back, src.data(), n) != 0)) { fprintf(stderr, "round trip of %zu bytes (kind %d) failed: %lld\n", n, kind, m); return 1; }
        ++encoded;
        // a destination that is too small: -1, cleanly.  (got - k bytes can never hold the got bytes of the stream)
        for (long long k : {1ll, 2ll, got / 2, got}) {
            const long long small = got - k;
            if (small < 0) continue;
            unsigned char* d2 = (unsigned char*)malloc(small ? (size_t)small : 1);
            const long long g2 = unet_tiff_lzw_encode(src.data(), (long long)n, d2, small);
            free(d2);
            if (g2 != -1) { fprintf(stderr, "encode of %zu bytes into %lld < %lld bytes returned %lld\n", n, small, got, g2); return 1; }
            ++refused;
        }
        free(back);
        free(dst);
    }
    printf("encoded %ld refused %ld\n", encoded, refused);
    return 0;
}
