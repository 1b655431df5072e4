// fl_gifsrc.cpp -- host half of the GIF decode front end: container walk and LZW (see fl_gifsrc.h).
// Plain C++: no HIP, no library.  Every read is bounds-checked against the file, every write against the frame's w x h and
// the caller's capacity.
#include "fl_gifsrc.h"

#include <string.h>

namespace fl {
namespace {

inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15u; }

// Where the frames of a decode go (null for the walk that only describes the file).
struct Sink {
    uint8_t *blob;
    size_t cap;
    uint32_t frames;       // as the describing walk counted them
    size_t idx_at;         // next frame's index bytes
    size_t pal_at;         // next palette
    uint32_t palettes;
    size_t global_pal;     // the global table without a transparent index, 0 = not stored yet
    size_t last_pal;       // the palette of the frame before, 0 = none
};

struct Frame {
    uint32_t x, y, w, h, disposal, interlaced, min_code;
    int transparent;       // -1 = none
    const uint8_t *table;  // the colour table that applies, 3 bytes an entry
    uint32_t table_size;
    size_t data_pos;       // the first data sub-block's length byte
};

// The frame's sub-blocks (validated by the walk: they end in a zero length inside the file) as a stream of LSB-first codes,
// decoded into out[0 .. npix).  Table entries are (position, length) of a string ALREADY in `out`: entry k is the string of the
// code before it plus one byte, and those bytes lie next to each other in the output, so a code is written by one forward copy.
int lzw_decode(const uint8_t *data, size_t pos, uint32_t min_code, uint8_t *out, size_t npix)
{
    uint32_t off[4096];
    uint16_t len[4096];
    const uint32_t clear = 1u << min_code, eoi = clear + 1u;
    uint32_t next = clear + 2u, width = min_code + 1u;
    uint64_t acc = 0;
    uint32_t nbits = 0, blk_left = 0;
    bool exhausted = false, have_prev = false;
    size_t o = 0, prev_pos = 0;
    uint32_t prev_len = 0;
    while (o < npix) {
        while (nbits <= 56u && !exhausted) {
            if (!blk_left) {
                blk_left = data[pos];
                if (!blk_left) { exhausted = true; break; }
                ++pos;
            }
            acc |= (uint64_t)data[pos++] << nbits;
            nbits += 8u;
            --blk_left;
        }
        if (nbits < width) break; // the data ends without an end code
        const uint32_t code = (uint32_t)acc & ((1u << width) - 1u);
        acc >>= width;
        nbits -= width;
        if (code == clear) { next = clear + 2u; width = min_code + 1u; have_prev = false; continue; }
        if (code == eoi) break;
        size_t src;
        uint32_t L;
        if (code < clear) { out[o] = (uint8_t)code; src = o; L = 1u; }
        else if (code < next) { src = off[code]; L = len[code]; }
        else if (code == next && have_prev) { src = prev_pos; L = prev_len + 1u; } // the string of the code before plus its own first byte
        else return kGifParse;
        const size_t m = L < npix - o ? L : npix - o;
        if (src != o) {
            if (src + m <= o) memcpy(out + o, out + src, m);
            else for (size_t i = 0; i < m; ++i) out[o + i] = out[src + i]; // overlapping: forward, byte by byte
        }
        if (have_prev && next < 4096u) { // (a full table stays as it is, at 12 bits, until a clear code)
            off[next] = (uint32_t)prev_pos;
            len[next] = (uint16_t)(prev_len + 1u);
            ++next;
            if (next == (1u << width) && width < 12u) ++width;
        }
        have_prev = true;
        prev_pos = o;
        prev_len = L;
        o += m;
    }
    return o == npix ? 0 : kGifParse;
}

void build_palette(const Frame &f, uint32_t *pal)
{
    for (uint32_t i = 0; i < 256u; ++i) {
        const uint8_t *e = f.table + 3u * i;
        pal[i] = i < f.table_size ? ((uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | 0xff000000u) : 0u;
    }
    if (f.transparent >= 0) pal[f.transparent] = 0u;
}

int decode_frame(const uint8_t *data, const Frame &f, bool global_table, uint32_t index, Sink &s)
{
    const size_t npix = (size_t)f.w * f.h;
    if (s.idx_at + npix > s.cap) return kGifSmall;
    uint8_t *idx = s.blob + s.idx_at;
    if (int rc = lzw_decode(data, f.data_pos, f.min_code, idx, npix)) return rc;
    uint32_t top = 0;
    for (size_t i = 0; i < npix; ++i) top = idx[i] > top ? idx[i] : top;
    if (top >= f.table_size) return kGifUnsupported;
    // the palette: the global table's plain copy or the frame before's where they are the same, else one more
    uint32_t pal[256];
    build_palette(f, pal);
    size_t at = 0;
    if (s.last_pal && !memcmp(s.blob + s.last_pal, pal, sizeof(pal))) at = s.last_pal;
    else if (s.global_pal && !memcmp(s.blob + s.global_pal, pal, sizeof(pal))) at = s.global_pal;
    else {
        if (s.pal_at + sizeof(pal) > s.cap) return kGifSmall;
        at = s.pal_at;
        memcpy(s.blob + at, pal, sizeof(pal));
        s.pal_at += sizeof(pal);
        s.palettes++;
        if (global_table && f.transparent < 0) s.global_pal = at;
    }
    s.last_pal = at;
    GifFrameRec r;
    r.x = f.x; r.y = f.y; r.w = f.w; r.h = f.h;
    r.disposal = f.disposal; r.interlaced = f.interlaced;
    r.pal_off = (uint32_t)at; r.idx_off = (uint32_t)s.idx_at;
    memcpy(s.blob + sizeof(GifBlobHeader) + (size_t)index * sizeof(GifFrameRec), &r, sizeof(r));
    s.idx_at += npix;
    return 0;
}

// One pass over the container.  Without a sink it fills `info` and goes on to the trailer whatever it meets (supported = 0
// where the decoder does not vouch for the file); with one it decodes every frame and stops at the first it cannot.
int walk(const uint8_t *data, size_t n, GifInfo &info, Sink *sink)
{
    info = GifInfo{};
    if (n < 13 || (memcmp(data, "GIF87a", 6) && memcmp(data, "GIF89a", 6))) return kGifParse;
    info.width = le16(data + 6); info.height = le16(data + 8);
    if (!info.width || !info.height) return kGifParse;
    const uint32_t gsize = (data[10] & 0x80u) ? 2u << (data[10] & 7u) : 0u;
    size_t pos = 13;
    if (n - pos < 3u * gsize) return kGifParse;
    const uint8_t *gtable = data + pos;
    pos += 3u * gsize;
    info.has_global_table = gsize ? 1u : 0u;
    bool supported = true;
    uint32_t disposal = 0;
    int transparent = -1;
    for (;;) {
        if (pos >= n) return kGifParse; // no trailer
        const uint8_t b = data[pos++];
        if (b == 0x3b) break;
        if (b == 0x21) { // an extension: label, sub-blocks; only the graphic control extension (0xf9) says anything here
            if (pos >= n) return kGifParse;
            const uint8_t label = data[pos++];
            for (bool first = true;; first = false) {
                if (pos >= n) return kGifParse;
                const uint32_t sz = data[pos];
                if (n - pos - 1u < sz) return kGifParse;
                if (!sz) { ++pos; break; }
                if (label == 0xf9 && first && sz >= 4u) { // it applies to the next image; of several the last one wins
                    disposal = (data[pos + 1] >> 2) & 7u;
                    transparent = (data[pos + 1] & 1u) ? (int)data[pos + 4] : -1;
                }
                pos += 1u + sz;
            }
            continue;
        }
        if (b != 0x2c) return kGifParse; // an unknown block introducer
        if (n - pos < 9u) return kGifParse;
        Frame f;
        f.x = le16(data + pos); f.y = le16(data + pos + 2); f.w = le16(data + pos + 4); f.h = le16(data + pos + 6);
        const uint8_t packed = data[pos + 8];
        pos += 9;
        f.interlaced = (packed & 0x40u) ? 1u : 0u;
        f.table = gtable; f.table_size = gsize;
        if (packed & 0x80u) {
            f.table_size = 2u << (packed & 7u);
            if (n - pos < 3u * f.table_size) return kGifParse;
            f.table = data + pos;
            pos += 3u * f.table_size;
        }
        if (!f.table_size) return kGifParse; // neither a local nor a global colour table
        if (pos >= n) return kGifParse;
        f.min_code = data[pos++];
        f.data_pos = pos;
        for (;;) { // the data sub-blocks, to their terminator
            if (pos >= n) return kGifParse;
            const uint32_t sz = data[pos];
            if (n - pos - 1u < sz) return kGifParse;
            pos += 1u + sz;
            if (!sz) break;
        }
        f.disposal = disposal; f.transparent = transparent;
        disposal = 0; transparent = -1;
        const uint32_t index = info.frames++;
        if (index >= kGifMaxFrames || !f.w || !f.h || f.x + f.w > info.width || f.y + f.h > info.height || f.min_code < 2u || f.min_code > 8u) {
            supported = false;
            if (sink) return kGifUnsupported;
            continue;
        }
        info.interlaced_frames += f.interlaced;
        info.transparent_frames += f.transparent >= 0 ? 1u : 0u;
        info.disposal_mask |= 1u << f.disposal;
        info.max_code_size = f.min_code > info.max_code_size ? f.min_code : info.max_code_size;
        info.index_bytes += (uint64_t)f.w * f.h;
        if (sink) {
            if (index >= sink->frames) return kGifSmall;
            if (int rc = decode_frame(data, f, f.table == gtable, index, *sink)) return rc;
        }
    }
    info.decoded_bytes = (uint64_t)info.frames * info.width * info.height * 4u;
    if (!info.frames || info.decoded_bytes > kGifMaxDecoded) supported = false;
    info.supported = supported ? 1u : 0u;
    return 0;
}

} // namespace

int gif_parse_info(const uint8_t *data, size_t n, GifInfo &info) { return walk(data, n, info, nullptr); }

size_t gif_blob_capacity(const GifInfo &info)
{
    return sizeof(GifBlobHeader) + (size_t)info.frames * sizeof(GifFrameRec) + align16((size_t)info.index_bytes) + 1024u * ((size_t)info.frames + 1u);
}

int gif_decode_blob(const uint8_t *data, size_t n, uint8_t *blob, size_t cap, GifBlobHeader *hdr)
{
    GifInfo info;
    if (int rc = walk(data, n, info, nullptr)) return rc;
    if (!info.supported) return kGifUnsupported;
    if (cap < gif_blob_capacity(info)) return kGifSmall;
    Sink s{};
    s.blob = blob; s.cap = cap; s.frames = info.frames;
    s.idx_at = sizeof(GifBlobHeader) + (size_t)info.frames * sizeof(GifFrameRec);
    s.pal_at = align16(s.idx_at + (size_t)info.index_bytes);
    const size_t idx_off = s.idx_at, pal_off = s.pal_at;
    memset(blob + idx_off + (size_t)info.index_bytes, 0, pal_off - idx_off - (size_t)info.index_bytes);
    GifInfo again;
    if (int rc = walk(data, n, again, &s)) return rc;
    GifBlobHeader H;
    H.magic = kGifMagic;
    H.width = info.width; H.height = info.height; H.frames = info.frames;
    H.palettes = s.palettes;
    H.pal_off = (uint32_t)pal_off; H.idx_off = (uint32_t)idx_off;
    H.total_bytes = (uint32_t)s.pal_at;
    memcpy(blob, &H, sizeof(H));
    if (hdr) *hdr = H;
    return 0;
}

} // namespace fl
