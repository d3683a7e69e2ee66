// LZW strips of a GeoTIFF encoded on the device (unet_amd/tiffenc.py): the code stream of unet_tiff_lzw_encode
// (csrc/tiff_codecs.hip), byte for byte.
//   unet_tiff_encode_strips   one wavefront (a workgroup of 64 lanes) per strip -> its slot of the scratch buffer + its size
//   unet_tiff_encode_tiles    the same walk over square tiles: only the staging differs -- the kernel takes it as a parameter
//   unet_tiff_compact_strips  slots -> one contiguous buffer at the exclusive prefix sum of the sizes
// LZW is a chain of dependent dictionary look-ups, so ONE lane of the wave walks the match chain; the 64 lanes together stage the next
// ENC_CHUNK input bytes into LDS (strided rows / planes are read in place, Predictor 2 is taken here: a parallel difference), empty the
// dictionary at every Clear and copy the packed output words of a phase from LDS into the slot with coalesced stores.  The parallelism
// of the launch is across strips.
// The dictionary is the open-addressed table of the host encoder (8192 words in LDS, word = key << 12 | code, key = prefix << 8 | byte,
// all ones = empty, linear probing, at most 3836 entries: load <= 0.47).  LDS per wave: 32 KiB table + 1 KiB input + 2 KiB output =
// 35 KiB, so 4 encoders fit the 160 KiB of a CU (one per SIMD), 1024 on the chip.  No atomics, no tables in global memory.
#include "common.h"

using namespace unet;

namespace {

constexpr int ENC_SLOTS = 8192;
constexpr int ENC_CHUNK = 1024;            // input bytes staged per phase
constexpr int ENC_OUTW = 512;              // output words of a phase: (ENC_CHUNK + 2) codes of 12 bits + 31 carried bits < 2048 bytes
constexpr uint32_t ENC_EMPTY = 0xFFFFFFFFu;
constexpr int LZW_CLEAR = 256, LZW_EOI = 257, LZW_LAST = 4094;

struct EncArgs {
    const void* src;
    long long row_stride, plane_stride, first, slot_bytes;
    int H, W, rows_per_strip, strips_per_plane, predictor;
    unsigned char* scratch;
    uint32_t* sizes;
};

struct TileLevel {                               // one image of a launch over tiles: a level of the pyramid
    const void* src;
    long long row_stride, plane_stride, first_tile;          // first_tile: index of its tile 0 in the launch's tile order
    int H, W, tiles_across, tiles_down;
};

struct TileArgs {
    long long first, slot_bytes;
    int tile, predictor, nlevels;
    unsigned char* scratch;
    uint32_t* sizes;
    TileLevel lv[UNET_TIFF_MAX_LEVELS];
};

// The staging step of the encoder: where block k of the launch lies and what its bytes are.  n bytes in rows of rowbytes; byte(t) is byte
// t of the block (sample differenced against its left neighbour in the block's row under Predictor 2, little-endian).
template <typename T>
struct StripSource {
    using Args = EncArgs;     // strip k = p * strips_per_plane + s: rows_per_strip whole rows of the image (the last strip of a plane fewer)
    const T* img;
    long long row_stride, n;
    uint32_t rowbytes;
    int predictor;
    __device__ StripSource(const EncArgs& a, long long k) {
        const int plane = (int)(k / a.strips_per_plane);
        const int r0 = (int)(k % a.strips_per_plane) * a.rows_per_strip;
        const int rows = min(a.rows_per_strip, a.H - r0);
        rowbytes = (uint32_t)a.W * (uint32_t)sizeof(T);
        n = (long long)rows * rowbytes;
        img = static_cast<const T*>(a.src) + plane * a.plane_stride + r0 * a.row_stride;
        row_stride = a.row_stride;
        predictor = a.predictor;
    }
    __device__ __forceinline__ unsigned char byte(int row0, uint32_t t) const {
        constexpr uint32_t ES = (uint32_t)sizeof(T);
        const uint32_t dr = t / rowbytes, cb = t - dr * rowbytes;
        const uint32_t s = cb / ES, kb = cb % ES;
        const T* rowp = img + (row0 + (long long)dr) * row_stride;
        T v = rowp[s];
        if (predictor == 2 && s > 0) v = (T)(v - rowp[s - 1]);
        return (unsigned char)((uint32_t)v >> (8 * kb));
    }
};

template <typename T>
struct TileSource {           // tile k of a level = (p * tiles_down + j) * tiles_across + i: tile x tile samples from column i * tile of row
    using Args = TileArgs;    // j * tile on; what lies beyond the right or bottom edge of the image is zero, and Predictor 2 runs along the
    const T* img;             // whole padded row (the first padded sample holds 0 - last), as libtiff writes an edge tile.  The launch's
    long long row_stride, n;  // tiles are those of its levels one level after the other.
    uint32_t rowbytes;
    int predictor, rows, cols;          // the part of the tile inside the image
    __device__ TileSource(const TileArgs& a, long long g) {
        int l = 0;
        while (l + 1 < a.nlevels && g >= a.lv[l + 1].first_tile) ++l;
        const TileLevel& L = a.lv[l];
        const long long k = g - L.first_tile;
        const long long per_plane = (long long)L.tiles_across * L.tiles_down;
        const int plane = (int)(k / per_plane);
        const long long rem = k % per_plane;
        const int j = (int)(rem / L.tiles_across), i = (int)(rem % L.tiles_across);
        rows = min(a.tile, L.H - j * a.tile);
        cols = min(a.tile, L.W - i * a.tile);
        rowbytes = (uint32_t)a.tile * (uint32_t)sizeof(T);
        n = (long long)a.tile * rowbytes;
        img = static_cast<const T*>(L.src) + plane * L.plane_stride + (long long)j * a.tile * L.row_stride + (long long)i * a.tile;
        row_stride = L.row_stride;
        predictor = a.predictor;
    }
    __device__ __forceinline__ unsigned char byte(int row0, uint32_t t) const {
        constexpr uint32_t ES = (uint32_t)sizeof(T);
        const uint32_t dr = t / rowbytes, cb = t - dr * rowbytes;
        const uint32_t s = cb / ES, kb = cb % ES;
        const int row = row0 + (int)dr;
        if (row >= rows) return 0;                       // a padded row: zeros, and their differences are zeros
        const T* rowp = img + (long long)row * row_stride;
        T v = (int)s < cols ? rowp[s] : (T)0;
        if (predictor == 2 && s > 0) v = (T)(v - ((int)s - 1 < cols ? rowp[s - 1] : (T)0));
        return (unsigned char)((uint32_t)v >> (8 * kb));
    }
};

// the bit packer of lane 0: MSB-first, whole big-endian words go to outw
struct Packer {
    uint64_t acc;
    int nbits;
    __device__ __forceinline__ void put(uint32_t code, int width, uint32_t* outw, int& outn) {
        acc = (acc << width) | code;
        nbits += width;
        if (nbits >= 32) {
            outw[outn++] = __builtin_bswap32((uint32_t)(acc >> (nbits - 32)));
            nbits -= 32;
        }
    }
};

template <typename T, template <typename> class Source>
__global__ __launch_bounds__(64) void lzw_encode_kernel(typename Source<T>::Args a) {
    __shared__ __attribute__((aligned(16))) uint32_t table[ENC_SLOTS];
    __shared__ __attribute__((aligned(16))) uint32_t stage_w[ENC_CHUNK / 4];
    __shared__ __attribute__((aligned(16))) uint32_t outw[ENC_OUTW];
    unsigned char* stage = reinterpret_cast<unsigned char*>(stage_w);
    const int lane = threadIdx.x;
    const int j = blockIdx.x;
    const Source<T> source(a, a.first + j);
    const uint32_t rowbytes = source.rowbytes;
    const long long n = source.n;
    uint32_t* slot = reinterpret_cast<uint32_t*>(a.scratch + j * a.slot_bytes);
    const long long slot_words = a.slot_bytes >> 2;

    auto clear_table = [&]() {
        uint4* t4 = reinterpret_cast<uint4*>(table);
        for (int i = lane; i < ENC_SLOTS / 4; i += 64) t4[i] = make_uint4(ENC_EMPTY, ENC_EMPTY, ENC_EMPTY, ENC_EMPTY);
    };
    clear_table();

    // lane 0's encoder state
    Packer pk{(uint64_t)LZW_CLEAR, 9};
    uint32_t prefix = 0;
    int width = 9, next = 258;
    long long flushed = 0;          // words already in the slot (wave-uniform)
    bool overflow = false;

    // copies the outn whole words of a phase into the slot; never past the slot
    auto flush = [&](int outn) {
        if (flushed + outn > slot_words) { overflow = true; return; }
        for (int i = lane; i < outn; i += 64) slot[flushed + i] = outw[i];
        flushed += outn;
    };

    for (long long base = 0; base < n; base += ENC_CHUNK) {
        const int chunk = (int)min((long long)ENC_CHUNK, n - base);
        const int row0 = (int)(base / rowbytes);
        const uint32_t col0 = (uint32_t)(base - (long long)row0 * rowbytes);
        for (int b = lane; b < chunk; b += 64) stage[b] = source.byte(row0, col0 + (uint32_t)b);
        __syncthreads();
        int pos = 0;
        while (pos < chunk) {
            int flag = 0, outn = 0;
            if (lane == 0) {
                int i = pos;
                if (base == 0 && i == 0) prefix = stage[i++];
                while (i < chunk) {
                    const uint32_t c = stage[i++];
                    const uint32_t key = (prefix << 8) | c;
                    uint32_t h = (key * 2654435761u) >> 19;
                    uint32_t e;
                    while ((e = table[h]) != ENC_EMPTY && (e >> 12) != key) h = (h + 1) & (ENC_SLOTS - 1);
                    if (e != ENC_EMPTY) { prefix = e & 0xFFFu; continue; }
                    pk.put(prefix, width, outw, outn);
                    table[h] = (key << 12) | (uint32_t)next;
                    prefix = c;
                    if (++next == LZW_LAST) {
                        pk.put(LZW_CLEAR, width, outw, outn);
                        next = 258;
                        width = 9;
                        flag = 1;
                        break;
                    }
                    if (next > (1 << width) - 1) ++width;
                }
                pos = i;
            }
            pos = __builtin_amdgcn_readfirstlane(pos);
            flag = __builtin_amdgcn_readfirstlane(flag);
            outn = __builtin_amdgcn_readfirstlane(outn);
            __syncthreads();
            flush(outn);
            if (flag) clear_table();
            __syncthreads();
        }
    }

    int outn = 0, tail = 0;
    if (lane == 0) {
        pk.put(prefix, width, outw, outn);
        if (++next == LZW_LAST) {
            pk.put(LZW_CLEAR, width, outw, outn);
            width = 9;
        } else if (next > (1 << width) - 1) {
            ++width;
        }
        pk.put(LZW_EOI, width, outw, outn);
        tail = (pk.nbits + 7) >> 3;                      // bytes of the last, zero-padded word
        if (pk.nbits > 0) outw[outn] = __builtin_bswap32((uint32_t)(pk.acc << (32 - pk.nbits)));
    }
    outn = __builtin_amdgcn_readfirstlane(outn);
    tail = __builtin_amdgcn_readfirstlane(tail);
    __syncthreads();
    const long long whole = flushed + outn;
    flush(outn + (tail ? 1 : 0));
    if (lane == 0) a.sizes[j] = overflow ? 0xFFFFFFFFu : (uint32_t)(whole * 4 + tail);
}

__global__ __launch_bounds__(256) void lzw_compact_kernel(const unsigned char* __restrict__ scratch, long long slot_bytes,
                                                          const uint32_t* __restrict__ sizes, const long long* __restrict__ offsets,
                                                          unsigned char* __restrict__ out, long long out_bytes) {
    const int j = blockIdx.x;
    const uint32_t sz = sizes[j];
    const long long off = offsets[j];
    if (sz == 0xFFFFFFFFu || (long long)sz > slot_bytes || off < 0 || off + sz > out_bytes) return;      // (the host raises on such a size)
    const unsigned char* s = scratch + j * slot_bytes;
    unsigned char* d = out + off;
    for (uint32_t i = threadIdx.x; i < sz; i += 256) d[i] = s[i];
}

}  // namespace

extern "C" int unet_tiff_encode_strips(const void* src, int elem_size, int P, int H, int W, long long row_stride, long long plane_stride,
                                       int rows_per_strip, int predictor, long long first, int count, unsigned char* scratch,
                                       long long slot_bytes, uint32_t* sizes, void* stream) {
    UNET_CHECK_ARG(src && scratch && sizes, "tiff_encode_strips: null pointer");
    UNET_CHECK_ARG(elem_size == 1 || elem_size == 2 || elem_size == 4, "tiff_encode_strips: elem_size must be 1, 2 or 4 (got %d)", elem_size);
    UNET_CHECK_ARG(P >= 1 && H >= 1 && W >= 1 && (long long)W * elem_size <= (1ll << 31) - 2 * ENC_CHUNK,
                   "tiff_encode_strips: bad image %d x %d x %d", P, H, W);
    UNET_CHECK_ARG(rows_per_strip >= 1 && rows_per_strip <= H && (long long)rows_per_strip * W * elem_size <= (1ll << 31) - 1,
                   "tiff_encode_strips: rows_per_strip must be in 1..H with a strip below 2^31 bytes (got %d)", rows_per_strip);
    UNET_CHECK_ARG(row_stride >= W && (P == 1 || plane_stride >= 1) && ((uintptr_t)src % elem_size) == 0,
                   "tiff_encode_strips: bad strides (%lld, %lld) or a misaligned source", row_stride, plane_stride);
    UNET_CHECK_ARG(predictor == 1 || predictor == 2, "tiff_encode_strips: predictor must be 1 or 2 (got %d)", predictor);
    const int spp = cdiv(H, rows_per_strip);
    UNET_CHECK_ARG(first >= 0 && count >= 1 && first + count <= (long long)P * spp,
                   "tiff_encode_strips: strips [%lld, %lld) of %lld", first, first + count, (long long)P * spp);
    UNET_CHECK_ARG(slot_bytes % 4 == 0 && slot_bytes >= unet_tiff_lzw_cap((long long)rows_per_strip * W * elem_size) && ((uintptr_t)scratch & 3) == 0,
                   "tiff_encode_strips: slot_bytes %lld must be a multiple of 4, at least the capacity of a strip, in a 4-byte aligned scratch", slot_bytes);
    EncArgs a{src, row_stride, plane_stride, first, slot_bytes, H, W, rows_per_strip, spp, predictor, scratch, sizes};
    const dim3 grid((unsigned)count), block(64);
    if (elem_size == 1) hipLaunchKernelGGL((lzw_encode_kernel<uint8_t, StripSource>), grid, block, 0, (hipStream_t)stream, a);
    else if (elem_size == 2) hipLaunchKernelGGL((lzw_encode_kernel<uint16_t, StripSource>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((lzw_encode_kernel<uint32_t, StripSource>), grid, block, 0, (hipStream_t)stream, a);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_tiff_encode_tile_levels(const unet_tiff_level* levels, int nlevels, int elem_size, int P, int tile, int predictor,
                                            long long first, int count, unsigned char* scratch, long long slot_bytes, uint32_t* sizes,
                                            void* stream) {
    UNET_CHECK_ARG(levels && scratch && sizes, "tiff_encode_tile_levels: null pointer");
    UNET_CHECK_ARG(nlevels >= 1 && nlevels <= UNET_TIFF_MAX_LEVELS, "tiff_encode_tile_levels: 1..%d levels (got %d)", UNET_TIFF_MAX_LEVELS, nlevels);
    UNET_CHECK_ARG(elem_size == 1 || elem_size == 2 || elem_size == 4, "tiff_encode_tile_levels: elem_size must be 1, 2 or 4 (got %d)", elem_size);
    UNET_CHECK_ARG(tile >= 16 && tile <= 1024 && tile % 16 == 0, "tiff_encode_tile_levels: tile must be a multiple of 16 in 16..1024 (got %d)", tile);
    UNET_CHECK_ARG(P >= 1, "tiff_encode_tile_levels: P must be >= 1 (got %d)", P);
    UNET_CHECK_ARG(predictor == 1 || predictor == 2, "tiff_encode_tile_levels: predictor must be 1 or 2 (got %d)", predictor);
    TileArgs a;
    memset(&a, 0, sizeof(a));
    long long total = 0;
    for (int l = 0; l < nlevels; ++l) {
        const unet_tiff_level& L = levels[l];
        UNET_CHECK_ARG(L.src && L.H >= 1 && L.W >= 1 && (long long)L.W * elem_size <= (1ll << 31) - 2 * ENC_CHUNK,
                       "tiff_encode_tile_levels: level %d: null source or bad image %d x %d x %d", l, P, L.H, L.W);
        UNET_CHECK_ARG(L.row_stride >= L.W && (P == 1 || L.plane_stride >= 1) && ((uintptr_t)L.src % elem_size) == 0,
                       "tiff_encode_tile_levels: level %d: bad strides (%lld, %lld) or a misaligned source", l, L.row_stride, L.plane_stride);
        a.lv[l] = TileLevel{L.src, L.row_stride, P > 1 ? L.plane_stride : 0, total, L.H, L.W, cdiv(L.W, tile), cdiv(L.H, tile)};
        total += (long long)P * a.lv[l].tiles_across * a.lv[l].tiles_down;
    }
    UNET_CHECK_ARG(first >= 0 && count >= 1 && first + count <= total, "tiff_encode_tile_levels: tiles [%lld, %lld) of %lld", first, first + count,
                   total);
    UNET_CHECK_ARG(slot_bytes % 4 == 0 && slot_bytes >= unet_tiff_lzw_cap((long long)tile * tile * elem_size) && ((uintptr_t)scratch & 3) == 0,
                   "tiff_encode_tile_levels: slot_bytes %lld must be a multiple of 4, at least the capacity of a tile, in a 4-byte aligned scratch",
                   slot_bytes);
    a.first = first;
    a.slot_bytes = slot_bytes;
    a.tile = tile;
    a.predictor = predictor;
    a.nlevels = nlevels;
    a.scratch = scratch;
    a.sizes = sizes;
    const dim3 grid((unsigned)count), block(64);
    if (elem_size == 1) hipLaunchKernelGGL((lzw_encode_kernel<uint8_t, TileSource>), grid, block, 0, (hipStream_t)stream, a);
    else if (elem_size == 2) hipLaunchKernelGGL((lzw_encode_kernel<uint16_t, TileSource>), grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((lzw_encode_kernel<uint32_t, TileSource>), grid, block, 0, (hipStream_t)stream, a);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}

extern "C" int unet_tiff_encode_tiles(const void* src, int elem_size, int P, int H, int W, long long row_stride, long long plane_stride, int tile,
                                      int predictor, long long first, int count, unsigned char* scratch, long long slot_bytes, uint32_t* sizes,
                                      void* stream) {
    const unet_tiff_level one{src, row_stride, plane_stride, H, W};
    return unet_tiff_encode_tile_levels(&one, 1, elem_size, P, tile, predictor, first, count, scratch, slot_bytes, sizes, stream);
}

extern "C" int unet_tiff_compact_strips(const unsigned char* scratch, long long slot_bytes, const uint32_t* sizes, const long long* offsets,
                                        int count, unsigned char* out, long long out_bytes, void* stream) {
    UNET_CHECK_ARG(scratch && sizes && offsets && out, "tiff_compact_strips: null pointer");
    UNET_CHECK_ARG(slot_bytes >= 4 && count >= 1 && out_bytes >= 0, "tiff_compact_strips: slot_bytes %lld, count %d, out_bytes %lld", slot_bytes, count, out_bytes);
    hipLaunchKernelGGL(lzw_compact_kernel, dim3((unsigned)count), dim3(256), 0, (hipStream_t)stream, scratch, slot_bytes, sizes, offsets, out, out_bytes);
    UNET_CHECK_LAUNCH();
    return UNET_OK;
}
