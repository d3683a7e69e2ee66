// Host-side strip / tile decoders of the GeoTIFF reader (unet_amd/tiffio.py).  The reference opens rasters through GDAL / rasterio
// (create_tiles_unet.py:252-434, data.py:18-28), which read LZW / PackBits / Deflate files transparently; neither is installed here and a real
// 20000 x 20000 scene is usually compressed.  Deflate is zlib (Python's); the two byte-oriented TIFF codecs are restated here because a pure
// Python loop decodes ~1 MB/s.  No device code: plain C++ behind the C ABI.
#include <stdint.h>
#include <string.h>

#include "unet_hip.h"

// TIFF 6.0 section 13: LZW with MSB-first codes of 9..12 bits, ClearCode 256, EndOfInformation 257, "early change" (the code width grows one
// code early).  Returns the number of bytes written to dst, or -1 on a malformed stream / overflow of cap.
// Table entries do not store strings: the string of a new code is, by construction, the bytes just written for the previous code plus the
// byte that follows them in the output -- so an entry is (offset into dst, length) and emitting a code is one forward copy out of the
// output already produced (a forward byte copy also gives the KwKwK case, where the last byte of the string is its own first byte).
extern "C" long long unet_tiff_lzw_decode(const unsigned char* src, long long n, unsigned char* dst, long long cap) {
    if (src == nullptr || dst == nullptr || n < 0 || cap < 0) return -1;
    enum { CLEAR = 256, EOI = 257, MAXC = 4096 };
    long long off[MAXC];             // where in dst the string of a code >= 258 was written when the code was created
    int len[MAXC];
    long long bitpos = 0, out = 0, prev_off = 0;
    const long long nbits = n * 8;
    int width = 9, next = 258, prev = -1, prev_len = 0;
    for (;;) {
        if (bitpos + width > nbits) break;          // a stream may end without EOI
        const long long byte = bitpos >> 3;
        uint32_t acc = ((uint32_t)src[byte] << 16) | ((byte + 1 < n ? (uint32_t)src[byte + 1] : 0u) << 8) | (byte + 2 < n ? (uint32_t)src[byte + 2] : 0u);
        const int code = (int)((acc >> (24 - (int)(bitpos & 7) - width)) & ((1u << width) - 1));
        bitpos += width;
        if (code == EOI) break;
        if (code == CLEAR) { width = 9; next = 258; prev = -1; continue; }
        int cur_len;
        if (code < 256) {
            if (out + 1 > cap) return -1;
            dst[out] = (unsigned char)code;
            cur_len = 1;
        } else {
            if (prev < 0 || code > next || (code == next && next >= MAXC)) return -1;      // a code beyond the table
            long long from;
            if (code == next) { from = prev_off; cur_len = prev_len + 1; }      // KwKwK: the previous string followed by its own first byte
            else { from = off[code]; cur_len = len[code]; }
            if (out + cur_len > cap) return -1;
            const unsigned char* q = dst + from;
            unsigned char* p = dst + out;
            if (from + cur_len <= out && cur_len >= 16) memcpy(p, q, (size_t)cur_len);
            else for (int k = 0; k < cur_len; ++k) p[k] = q[k];                 // forward, byte by byte: source and destination may overlap
        }
        if (prev >= 0 && next < MAXC) {            // new entry = previous string + first byte of this one = dst[prev_off, prev_off + prev_len]
            off[next] = prev_off;
            len[next] = prev_len + 1;
            ++next;
        }
        prev_off = out;
        prev_len = cur_len;
        out += cur_len;
        prev = code;
        if (next + 1 >= (1 << width) && width < 12) ++width;      // early change
    }
    return out;
}

// The encoder of the writer (unet_amd/tiffio.py write_tiff(compress="lzw")); csrc/tiff_encode.hip is the same rule on the device and
// tests/tiff_lzw_ref.py the same rule in Python -- the three produce equal bytes.  Every strip: Clear at 9 bits, next = 258; greedy
// longest match; a pair (prefix, byte) that is not in the table emits prefix, becomes code `next`, and then either next == 4094 emits
// Clear (at 12 bits) and empties the table, or next > 2^width - 1 widens the codes (the early change); at the end the pending prefix, the
// same step once more, EOI, zero padding.  An empty strip is Clear, EOI.  unet_tiff_lzw_cap(n) bytes always suffice: at most one 12-bit
// code per byte, one Clear per 3836 additions, the Clear / EOI frame.
// The dictionary is an open-addressed table of 8192 words, word = key << 12 | code with key = prefix << 8 | byte, all ones = empty.
extern "C" long long unet_tiff_lzw_cap(long long n) { return n < 0 ? -1 : (3 * (n + n / 3836 + 4) + 1) / 2; }

namespace {
struct LzwBits {          // MSB-first packer into dst[0, cap)
    unsigned char* dst;
    long long cap, out;
    uint64_t acc;
    int nbits;
    bool put(int code, int width) {
        acc = (acc << width) | (uint64_t)code;
        nbits += width;
        while (nbits >= 8) {
            if (out >= cap) return false;
            dst[out++] = (unsigned char)(acc >> (nbits - 8));
            nbits -= 8;
        }
        return true;
    }
    bool flush() {
        if (nbits == 0) return true;
        if (out >= cap) return false;
        dst[out++] = (unsigned char)(acc << (8 - nbits));
        nbits = 0;
        return true;
    }
};
}  // namespace

extern "C" long long unet_tiff_lzw_encode(const unsigned char* src, long long n, unsigned char* dst, long long cap) {
    if ((src == nullptr && n > 0) || dst == nullptr || n < 0 || cap < 0) return -1;
    enum { CLEAR = 256, EOI = 257, LAST = 4094, SLOTS = 8192 };
    uint32_t table[SLOTS];
    memset(table, 0xFF, sizeof(table));
    LzwBits b{dst, cap, 0, 0, 0};
    int width = 9, next = 258;
    // after a code has gone out: the table grows by one (at the end of the strip only the counter does); Clear or the early change
    auto step = [&]() -> bool {
        if (++next == LAST) {
            if (!b.put(CLEAR, width)) return false;
            memset(table, 0xFF, sizeof(table));
            next = 258;
            width = 9;
        } else if (next > (1 << width) - 1) {
            ++width;
        }
        return true;
    };
    if (!b.put(CLEAR, 9)) return -1;
    if (n > 0) {
        uint32_t prefix = src[0];
        for (long long i = 1; i < n; ++i) {
            const uint32_t key = (prefix << 8) | src[i];
            uint32_t h = (key * 2654435761u) >> 19;
            uint32_t e;
            while ((e = table[h]) != 0xFFFFFFFFu && (e >> 12) != key) h = (h + 1) & (SLOTS - 1);
            if (e != 0xFFFFFFFFu) { prefix = e & 0xFFFu; continue; }
            if (!b.put((int)prefix, width)) return -1;
            table[h] = (key << 12) | (uint32_t)next;
            if (!step()) return -1;
            prefix = src[i];
        }
        if (!b.put((int)prefix, width) || !step()) return -1;
    }
    if (!b.put(EOI, width) || !b.flush()) return -1;
    return b.out;
}

// PackBits (TIFF 6.0 section 9): n in [0,127]: copy n + 1 literal bytes; n in [-127,-1]: repeat the next byte 1 - n times; -128: no-op
extern "C" long long unet_tiff_packbits_decode(const unsigned char* src, long long n, unsigned char* dst, long long cap) {
    if (src == nullptr || dst == nullptr || n < 0 || cap < 0) return -1;
    long long i = 0, out = 0;
    while (i < n) {
        const int c = (int8_t)src[i++];
        if (c >= 0) {
            const int k = c + 1;
            if (i + k > n || out + k > cap) return -1;
            memcpy(dst + out, src + i, (size_t)k);
            i += k; out += k;
        } else if (c != -128) {
            const int k = 1 - c;
            if (i >= n || out + k > cap) return -1;
            memset(dst + out, src[i++], (size_t)k);
            out += k;
        }
    }
    return out;
}
