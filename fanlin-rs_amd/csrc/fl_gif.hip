// fl_gif.hip -- the GIF encoder: one finished GIF89a file from the frames the per-frame pipeline left on the device.
//
// What the reference's encoder writes for frames of at most 256 colours (image 0.25.6 GifEncoder::encode_frames over gif 0.13.1
// Frame::from_rgba_speed): alpha != 0 becomes 255, the palette is the distinct (r, g, b, a) tuples in ascending order, padded
// with zeros to 2, 4 .. 256 entries, the transparent index is that of the LAST pixel with alpha 0, every frame is a full-canvas
// image with a local table, disposal 1, delay 0.  Above 256 colours the reference runs NeuQuant; here the file's overflow flag
// is set, every later kernel returns at once and the caller takes the pixels instead -- or, where the job says so
// (FLGPU_ENCODE_GIF_QUANTIZE), the frame is marked and fl_gifquant.hip gives it a table and indices of the library's own rule.
//
// LZW is serial, so a frame's indices are cut into segments of kGifSegIndices that are coded independently, each from an empty
// table and closed by a clear code: a decoder sees one ordinary stream.  The segments' bit strings are then gathered into the
// frame's sub-blocks (no atomics: every output dword is built by one thread), and the frames are placed behind one another.
#include <algorithm>

#include "fl_gif.h"
#include "fl_wave.h"

namespace fl {

namespace {

constexpr uint32_t kNoColour = 1u;          // never a key: the low byte of a key is 0 or 255
constexpr uint32_t kNoEntry = 0xffffffffu;  // never a dictionary entry: a prefix code stays below 4,095

// r, g, b, a big-endian in a dword, so that dword order is tuple order; alpha normalised to 0 / 255
__device__ __forceinline__ uint32_t key_of_rgba(uint32_t v) { return (__builtin_bswap32(v) & 0xffffff00u) | ((v >> 24) ? 255u : 0u); }
__device__ __forceinline__ uint32_t key_of_la(uint32_t v) { return (v & 255u) * 0x01010100u | ((v >> 8) ? 255u : 0u); } // LumaA8::to_rgba8: l, l, l, a
__device__ __forceinline__ uint32_t key_at(const uint8_t *frame, uint32_t p, uint32_t c)
{
    return c == 4u ? key_of_rgba(reinterpret_cast<const uint32_t *>(frame)[p]) : key_of_la(reinterpret_cast<const uint16_t *>(frame)[p]);
}
__device__ __forceinline__ uint32_t colour_slot(uint32_t key) { return (key * 0x9E3779B1u) >> 22; }

__device__ const uint8_t kFileHead[kGifFileHead] = {'G', 'I', 'F', '8', '9', 'a', 0, 0, 0, 0, 0x70, 0, 0,
                                                    0x21, 0xff, 0x0b, 'N', 'E', 'T', 'S', 'C', 'A', 'P', 'E', '2', '.', '0', 3, 1, 0, 0, 0};

// One workgroup per frame: the set of colours in an LDS hash, their ranks, and with them the frame's head (graphic control
// extension, image descriptor, padded local table, code size byte) and the colour -> index table of gif_index_kernel.
__global__ __launch_bounds__(kGifThreads) void gif_palette_kernel(GifEncJob J)
{
    __shared__ uint32_t s_tab[kGifColourSlots];
    __shared__ uint32_t s_keys[256], s_slot[256], s_sorted[256];
    __shared__ uint32_t s_count, s_n, s_tpos, s_tidx;
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    const uint8_t *frame = J.pixels + (size_t)f * J.pix_pitch;
    for (uint32_t i = tid; i < kGifColourSlots; i += kGifThreads) s_tab[i] = kNoColour;
    if (tid < 256u) s_sorted[tid] = 0u;
    if (tid == 0u) { s_count = 0u; s_n = 0u; s_tpos = 0u; s_tidx = kGifNoTransparent; }
    __syncthreads();
    volatile uint32_t *tab = s_tab;
    volatile uint32_t *count = &s_count;
    uint32_t last = kNoColour, tpos = 0u;
    for (uint32_t p = tid; p < J.px; p += kGifThreads) {
        // (at most 256 + one per thread colours are ever in the table: it cannot fill)
        if (*count > 256u) break;
        const uint32_t key = key_at(frame, p, J.c);
        if (!(key & 255u)) tpos = p + 1u;
        if (key == last) continue;
        last = key;
        uint32_t h = colour_slot(key);
        for (uint32_t probe = 0; probe < kGifColourSlots; ++probe, h = (h + 1u) & (kGifColourSlots - 1u)) {
            uint32_t cur = tab[h];
            if (cur == kNoColour) {
                cur = atomicCAS(&s_tab[h], kNoColour, key);
                if (cur == kNoColour) { atomicAdd(&s_count, 1u); break; }
            }
            if (cur == key) break;
        }
    }
    if (tpos) atomicMax(&s_tpos, tpos);
    __syncthreads();
    const uint32_t n = s_count;
    if (n > 256u) { // NeuQuant's ground: the caller gets the pixels, or -- J.quant -- this frame its table from fl_gifquant.hip
        if (J.quant) {
            uint4 *cells = reinterpret_cast<uint4 *>(J.qcells + (size_t)f * 4u * J.qstride);
            for (uint32_t i = tid; i < J.qstride; i += kGifThreads) cells[i] = make_uint4(0u, 0u, 0u, 0u);
            if (tid == 0u) J.frec[(size_t)f * kGifFrameRec + kGrQuant] = kGqMarked;
        } else if (tid == 0u) {
            J.status[0] = 1u;
        }
        return;
    }
    for (uint32_t i = tid; i < kGifColourSlots; i += kGifThreads) {
        const uint32_t k = s_tab[i];
        J.ckeys[(size_t)f * kGifColourSlots + i] = k;
        if (k != kNoColour) { const uint32_t at = atomicAdd(&s_n, 1u); s_keys[at] = k; s_slot[at] = i; }
    }
    __syncthreads();
    // rank = the number of smaller keys (n <= 256 reads of one LDS word by all lanes at a time)
    if (tid < n) {
        const uint32_t key = s_keys[tid];
        uint32_t rank = 0u;
        for (uint32_t j = 0; j < n; ++j) rank += s_keys[j] < key ? 1u : 0u;
        s_sorted[rank] = key;
        J.cvals[(size_t)f * kGifColourSlots + s_slot[tid]] = rank;
        if (s_tpos && key == key_at(frame, s_tpos - 1u, J.c)) s_tidx = rank;
    }
    __syncthreads();
    const uint32_t tbits = n <= 2u ? 1u : 32u - (uint32_t)__builtin_clz(n - 1u), tsize = 1u << tbits, mcs = tbits < 2u ? 2u : tbits;
    uint8_t *body = J.bodies + (size_t)f * J.body_pitch;
    if (tid < tsize) {
        const uint32_t k = s_sorted[tid]; // (zero beyond the n colours)
        body[18u + 3u * tid] = (uint8_t)(k >> 24); body[19u + 3u * tid] = (uint8_t)(k >> 16); body[20u + 3u * tid] = (uint8_t)(k >> 8);
    }
    if (tid == 0u) {
        const uint32_t t = s_tidx;
        const uint8_t head[18] = {0x21, 0xf9, 4, (uint8_t)(t == kGifNoTransparent ? 0x04 : 0x05), 0, 0, (uint8_t)(t == kGifNoTransparent ? 0u : t), 0,
                                  0x2c, 0, 0, 0, 0, (uint8_t)J.w, (uint8_t)(J.w >> 8), (uint8_t)J.h, (uint8_t)(J.h >> 8), (uint8_t)(0x80u | (tbits - 1u))};
        for (uint32_t i = 0; i < 18u; ++i) body[i] = head[i];
        body[18u + 3u * tsize] = (uint8_t)mcs;
        uint32_t *rec = J.frec + (size_t)f * kGifFrameRec;
        rec[kGrColours] = n; rec[kGrTableBits] = tbits; rec[kGrCodeSize] = mcs; rec[kGrTransparent] = t;
        rec[kGrHeadBytes] = 19u + 3u * tsize; rec[kGrQuant] = 0u;
    }
}

// One index byte per pixel, four pixels a thread: the frame's colour -> index table in LDS, 16-byte reads of Rgba8, dword stores.
// (A frame the quantiser took has its indices from gif_qindex_kernel.)
__global__ __launch_bounds__(kGifThreads) void gif_index_kernel(GifEncJob J)
{
    if (J.status[0] || J.frec[(size_t)blockIdx.y * kGifFrameRec + kGrQuant]) return;
    __shared__ uint32_t s_k[kGifColourSlots];
    __shared__ uint8_t s_v[kGifColourSlots];
    const uint32_t f = blockIdx.y, tid = threadIdx.x;
    for (uint32_t i = tid; i < kGifColourSlots; i += kGifThreads) {
        s_k[i] = J.ckeys[(size_t)f * kGifColourSlots + i];
        s_v[i] = (uint8_t)J.cvals[(size_t)f * kGifColourSlots + i]; // (whatever the words of empty slots hold: never looked at)
    }
    __syncthreads();
    const uint8_t *frame = J.pixels + (size_t)f * J.pix_pitch;
    uint32_t *out = reinterpret_cast<uint32_t *>(J.indices + (size_t)f * J.idx_pitch);
    const uint32_t quads = (J.px + 3u) / 4u;
    for (uint32_t q = blockIdx.x * kGifThreads + tid; q < quads; q += gridDim.x * kGifThreads) {
        uint32_t key[4] = {kNoColour, kNoColour, kNoColour, kNoColour};
        if (J.c == 4u && 4u * q + 4u <= J.px) {
            const uint4 v = reinterpret_cast<const uint4 *>(frame)[q];
            key[0] = key_of_rgba(v.x); key[1] = key_of_rgba(v.y); key[2] = key_of_rgba(v.z); key[3] = key_of_rgba(v.w);
        } else {
            for (uint32_t k = 0; k < 4u; ++k)
                if (4u * q + k < J.px) key[k] = key_at(frame, 4u * q + k, J.c);
        }
        uint32_t word = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (key[k] == kNoColour) continue;
            uint32_t h = colour_slot(key[k]);
            for (uint32_t probe = 0; probe < kGifColourSlots && s_k[h] != key[k]; ++probe) h = (h + 1u) & (kGifColourSlots - 1u);
            word |= (uint32_t)s_v[h] << (8u * k);
        }
        out[q] = word;
    }
}

// One wave per segment: greedy longest match from an empty table.  The chain is serial, so every lane walks it with the same
// values (the indices arrive 64 at a time, one a lane, and are read back lane by lane); lane 0 stores the codes.
__global__ __launch_bounds__(64) void gif_lzw_kernel(GifEncJob J)
{
    if (J.status[0]) return;
    __shared__ uint32_t s_dict[kGifDictSlots]; // prefix code << 20 | byte << 12 | code
    const uint32_t sid = blockIdx.x, f = sid / J.nseg, s = sid - f * J.nseg, lane = threadIdx.x;
    for (uint32_t i = lane; i < kGifDictSlots; i += 64u) s_dict[i] = kNoEntry;
    __syncthreads();
    const uint32_t first = s * kGifSegIndices, count = min(kGifSegIndices, J.px - first);
    const uint8_t *idx = J.indices + (size_t)f * J.idx_pitch + first;
    const uint32_t mcs = J.frec[(size_t)f * kGifFrameRec + kGrCodeSize];
    const uint32_t clear = 1u << mcs, eoi = clear + 1u;
    uint32_t width = mcs + 1u, nxt = clear + 2u;
    uint32_t *out = J.segs + (size_t)sid * kGifSegDwords;
    uint64_t acc = 0;
    uint32_t nbits = 0, nw = 0;
    auto put = [&](uint32_t code) {
        acc |= (uint64_t)code << nbits;
        nbits += width;
        if (nbits >= 32u) {
            if (lane == 0u) out[nw] = (uint32_t)acc;
            ++nw; acc >>= 32; nbits -= 32u;
        }
    };
    if (s == 0u) put(clear); // (the segments behind it follow the clear code that closed the one before)
    uint32_t cur = 0;
    for (uint32_t base = 0; base < count; base += 64u) {
        const uint32_t mine = base + lane < count ? idx[base + lane] : 0u;
        const uint32_t m = min(64u, count - base);
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)j);
            if (base + j == 0u) { cur = k; continue; }
            const uint32_t key = cur << 8 | k;
            uint32_t h = (key * 0x9E3779B1u) >> 20;
            bool found = false;
            for (uint32_t probe = 0; probe < kGifDictSlots; ++probe, h = (h + 1u) & (kGifDictSlots - 1u)) {
                const uint32_t e = s_dict[h];
                if (e == kNoEntry) break;
                if ((e >> 12) == key) { cur = e & 0xfffu; found = true; break; }
            }
            if (found) continue;
            put(cur);
            s_dict[h] = key << 12 | nxt; // (every lane the same word: at most kGifSegIndices - 1 entries, the table is never half full)
            ++nxt;
            if (nxt - 1u == (1u << width) && width < 12u) ++width;
            cur = k;
        }
    }
    put(cur);
    // the decoder adds one more entry behind the last data code: the closing code's width follows that
    if (nxt == (1u << width) && width < 12u) ++width;
    put(s + 1u == J.nseg ? eoi : clear);
    if (lane == 0u) {
        if (nbits) out[nw] = (uint32_t)acc;
        J.seg_bits[sid] = nw * 32u + nbits;
    }
}

// One workgroup per frame: where every segment's bits start in the frame's data, and with their sum the frame's bytes.
__global__ __launch_bounds__(kGifThreads) void gif_scan_kernel(GifEncJob J)
{
    if (J.status[0]) return;
    __shared__ uint32_t s_w[kGifThreads / 64u];
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    uint32_t base = 0;
    for (uint32_t s0 = 0; s0 < J.nseg; s0 += kGifThreads) {
        const uint32_t s = s0 + tid;
        const uint32_t v = s < J.nseg ? J.seg_bits[(size_t)f * J.nseg + s] : 0u;
        uint32_t total;
        const uint32_t ex = wg_scan<kGifThreads>(v, s_w, &total);
        if (s < J.nseg) J.seg_off[(size_t)f * J.nseg + s] = base + ex;
        base += total;
    }
    if (tid == 0u) {
        uint32_t *rec = J.frec + (size_t)f * kGifFrameRec;
        const uint32_t d = (base + 7u) / 8u;
        rec[kGrDataBits] = base;
        rec[kGrBytes] = rec[kGrHeadBytes] + d + (d + 254u) / 255u + 1u;
    }
}

// Every dword of a frame's data is gathered from the segments that cover it, and its bytes go where the sub-block framing
// puts them: data byte k at k + k / 255 + 1 behind the code size byte.  The lanes that own a block's first byte write its
// length, the one that owns the last byte the terminator.
__global__ __launch_bounds__(kGifThreads) void gif_pack_kernel(GifEncJob J)
{
    if (J.status[0]) return;
    const uint32_t f = blockIdx.y;
    const uint32_t *rec = J.frec + (size_t)f * kGifFrameRec;
    const uint32_t bits = rec[kGrDataBits], d = (bits + 7u) / 8u, ndw = (bits + 31u) / 32u;
    uint8_t *data = J.bodies + (size_t)f * J.body_pitch + rec[kGrHeadBytes];
    const uint32_t *off = J.seg_off + (size_t)f * J.nseg, *len = J.seg_bits + (size_t)f * J.nseg;
    for (uint32_t j = blockIdx.x * kGifThreads + threadIdx.x; j < ndw; j += gridDim.x * kGifThreads) {
        const uint32_t pos = 32u * j;
        uint32_t lo = 0, hi = J.nseg - 1u; // the last segment that starts at or in front of pos
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1u) >> 1;
            if (off[mid] <= pos) lo = mid; else hi = mid - 1u;
        }
        uint32_t word = 0u, filled = 0u;
        for (uint32_t s = lo; filled < 32u && s < J.nseg; ++s) {
            const uint32_t o = pos + filled - off[s], avail = len[s] - o, take = min(32u - filled, avail);
            const uint32_t *scr = J.segs + ((size_t)f * J.nseg + s) * kGifSegDwords + (o >> 5);
            uint32_t part = (uint32_t)((scr[0] | (uint64_t)scr[1] << 32) >> (o & 31u));
            if (take < 32u) part &= (1u << take) - 1u;
            word |= part << filled;
            filled += take;
        }
#pragma unroll
        for (uint32_t b = 0; b < 4u; ++b) {
            const uint32_t k = 4u * j + b;
            if (k >= d) break;
            data[k + k / 255u + 1u] = (uint8_t)(word >> (8u * b));
            if (k % 255u == 0u) data[k + k / 255u] = (uint8_t)min(255u, d - k);
            if (k == d - 1u) data[d + (d + 254u) / 255u] = 0u;
        }
    }
}

// The frames behind one another: every workgroup sums the bytes of the frames in front of its own (any number of frames) and
// copies its share; the first one writes the file's head, the last frame's first one the trailer and the file's length.
__global__ __launch_bounds__(kGifThreads) void gif_file_kernel(GifEncJob J)
{
    if (J.status[0]) return;
    __shared__ uint32_t s_w[kGifThreads / 64u];
    const uint32_t f = blockIdx.y, tid = threadIdx.x;
    uint32_t part = 0u;
    for (uint32_t g = tid; g < f; g += kGifThreads) part += J.frec[(size_t)g * kGifFrameRec + kGrBytes];
    part = wave_sum(part);
    if ((tid & 63u) == 0u) s_w[tid >> 6] = part;
    __syncthreads();
    uint32_t at = kGifFileHead;
    for (uint32_t i = 0; i < kGifThreads / 64u; ++i) at += s_w[i];
    const uint32_t bytes = J.frec[(size_t)f * kGifFrameRec + kGrBytes];
    const uint8_t *body = J.bodies + (size_t)f * J.body_pitch;
    for (uint32_t i = blockIdx.x * kGifThreads + tid; i < bytes; i += gridDim.x * kGifThreads) J.file[at + i] = body[i];
    if (blockIdx.x) return;
    if (f == 0u && tid < kGifFileHead)
        J.file[tid] = tid == 6u ? (uint8_t)J.w : tid == 7u ? (uint8_t)(J.w >> 8) : tid == 8u ? (uint8_t)J.h : tid == 9u ? (uint8_t)(J.h >> 8) : kFileHead[tid];
    if (f + 1u == J.frames && tid == 0u) { J.file[at + bytes] = 0x3b; J.status[1] = at + bytes + 1u; }
}

} // namespace

hipError_t launch_gif_encode(const GifEncJob &J, hipStream_t st)
{
    if (!J.frames || !J.px || J.nseg != gif_segments(J.px) || (J.c != 2u && J.c != 4u) || J.frames > 65535u) return hipErrorInvalidValue;
    const uint32_t quads = (J.px + 3u) / 4u;
    const uint32_t max_dw = (uint32_t)((12ull * (J.px + 1ull + J.nseg) + 31u) / 32u);
    auto groups = [](uint64_t items, uint32_t cap) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + kGifThreads - 1) / kGifThreads, 1), cap); };
    if (J.quant && (!gif_quantizable(J.px, J.frames) || J.qstride != gif_quant_stride(J.px) || !J.qcells || !J.qbox)) return hipErrorInvalidValue;
    gif_palette_kernel<<<dim3(J.frames), dim3(kGifThreads), 0, st>>>(J);
    if (J.quant) launch_gif_quantize(J, st);
    gif_index_kernel<<<dim3(groups(quads, 64), J.frames), dim3(kGifThreads), 0, st>>>(J);
    gif_lzw_kernel<<<dim3(J.frames * J.nseg), dim3(64), 0, st>>>(J);
    gif_scan_kernel<<<dim3(J.frames), dim3(kGifThreads), 0, st>>>(J);
    gif_pack_kernel<<<dim3(groups(max_dw, 256), J.frames), dim3(kGifThreads), 0, st>>>(J);
    gif_file_kernel<<<dim3(groups(J.body_pitch / 16u, 64), J.frames), dim3(kGifThreads), 0, st>>>(J);
    return hipGetLastError();
}

} // namespace fl
