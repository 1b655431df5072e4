// fl_pngsrc.cpp -- host half of the PNG decode front end: container, CRC-32, inflate, Adler-32 (see fl_pngsrc.h).
// Plain C++: no HIP, no zlib.  Every read is bounds-checked against the file, every write against the size IHDR implies.
#include "fl_pngsrc.h"

#include <string.h>

#include <memory>
#include <vector>

#include "fl_inflate_core.h"

namespace fl {
namespace {

inline uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
constexpr uint32_t fourcc(char a, char b, char c, char d) { return (uint32_t)(uint8_t)a << 24 | (uint32_t)(uint8_t)b << 16 | (uint32_t)(uint8_t)c << 8 | (uint8_t)d; }
constexpr uint32_t kIHDR = fourcc('I', 'H', 'D', 'R'), kPLTE = fourcc('P', 'L', 'T', 'E'), kTRNS = fourcc('t', 'R', 'N', 'S'),
                   kIDAT = fourcc('I', 'D', 'A', 'T'), kIEND = fourcc('I', 'E', 'N', 'D');
const uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};

// CRC-32 (ISO 3309, as PNG uses it), eight bytes per step
struct CrcTables {
    uint32_t t[8][256];
    CrcTables()
    {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int s = 1; s < 8; ++s) t[s][i] = t[0][t[s - 1][i] & 255u] ^ (t[s - 1][i] >> 8);
    }
};

uint32_t crc32(const uint8_t *p, size_t n)
{
    static const CrcTables T;
    uint32_t c = 0xffffffffu;
    while (n >= 8) {
        uint32_t a, b;
        memcpy(&a, p, 4);
        memcpy(&b, p + 4, 4);
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
        a = __builtin_bswap32(a); b = __builtin_bswap32(b);
#endif
        a ^= c;
        c = T.t[7][a & 255u] ^ T.t[6][(a >> 8) & 255u] ^ T.t[5][(a >> 16) & 255u] ^ T.t[4][a >> 24] ^
            T.t[3][b & 255u] ^ T.t[2][(b >> 8) & 255u] ^ T.t[1][(b >> 16) & 255u] ^ T.t[0][b >> 24];
        p += 8; n -= 8;
    }
    while (n--) c = T.t[0][(c ^ *p++) & 255u] ^ (c >> 8);
    return c ^ 0xffffffffu;
}

uint32_t adler32(const uint8_t *p, size_t n)
{
    uint32_t a = 1, b = 0;
    while (n) {
        size_t k = n < 5552 ? n : 5552; // the longest run for which b cannot overflow 32 bits
        n -= k;
        while (k >= 8) {
            a += p[0]; b += a; a += p[1]; b += a; a += p[2]; b += a; a += p[3]; b += a;
            a += p[4]; b += a; a += p[5]; b += a; a += p[6]; b += a; a += p[7]; b += a;
            p += 8; k -= 8;
        }
        while (k--) { a += *p++; b += a; }
        a %= 65521u; b %= 65521u;
    }
    return b << 16 | a;
}

// One chunk at data[pos]: 0 = ok (pos advanced behind its CRC), kPngParse = it does not fit the file.
struct Chunk { uint32_t type; const uint8_t *p; uint32_t len; };
int next_chunk(const uint8_t *data, size_t n, size_t &pos, Chunk &c)
{
    if (pos > n || n - pos < 12) return kPngParse;
    const uint32_t len = be32(data + pos);
    if (len > 0x7fffffffu || (size_t)len > n - pos - 12) return kPngParse;
    c.type = be32(data + pos + 4);
    c.p = data + pos + 8;
    c.len = len;
    pos += 12 + (size_t)len;
    return 0;
}
bool chunk_crc_ok(const Chunk &c) { return crc32(c.p - 4, (size_t)c.len + 4) == be32(c.p + c.len); }

// What the walk over the chunks collects besides PngInfo.
struct Container {
    PngInfo info;
    const uint8_t *plte = nullptr;
    const uint8_t *trns = nullptr;
    uint32_t trns_len = 0;
    size_t first_idat = 0; // file offset of the first IDAT chunk
};

// verify = false: lengths and layout only (a caller that sizes its buffers first and lets png_decode_scanlines check the CRCs, once)
// adam7 = true: an interlaced file of depth <= 8 is supported, bounded on its seven passes' scanlines
int walk(const uint8_t *data, size_t n, Container &C, bool verify, bool adam7)
{
    auto crc_ok = [verify](const Chunk &c) { return !verify || chunk_crc_ok(c); };
    PngInfo &I = C.info;
    I = PngInfo();
    if (!data || n < 8 || memcmp(data, kSignature, 8) != 0) return kPngParse;
    size_t pos = 8;
    Chunk c;
    if (next_chunk(data, n, pos, c) || c.type != kIHDR || c.len != 13 || !crc_ok(c)) return kPngParse;
    I.width = be32(c.p); I.height = be32(c.p + 4);
    I.bit_depth = c.p[8]; I.color_type = c.p[9];
    if (I.width == 0 || I.height == 0 || I.width > 0x7fffffffu || I.height > 0x7fffffffu) return kPngParse;
    if (c.p[10] != 0 || c.p[11] != 0 || c.p[12] > 1) return kPngParse; // compression, filter method, interlace
    I.interlaced = c.p[12];
    uint32_t samples = 0;
    const uint32_t d = I.bit_depth;
    switch (I.color_type) {
    case 0: samples = 1; if (d != 1 && d != 2 && d != 4 && d != 8 && d != 16) return kPngParse; break;
    case 2: samples = 3; if (d != 8 && d != 16) return kPngParse; break;
    case 3: samples = 1; if (d != 1 && d != 2 && d != 4 && d != 8) return kPngParse; break;
    case 4: samples = 2; if (d != 8 && d != 16) return kPngParse; break;
    case 6: samples = 4; if (d != 8 && d != 16) return kPngParse; break;
    default: return kPngParse;
    }
    bool seen_idat = false, seen_iend = false, idat_ended = false;
    while (!seen_iend) {
        const size_t at = pos;
        if (next_chunk(data, n, pos, c)) return kPngParse; // truncated: no IEND
        if (seen_idat && c.type != kIDAT) idat_ended = true;
        switch (c.type) {
        case kIHDR:
            return kPngParse;
        case kPLTE:
            if (!crc_ok(c) || c.len == 0 || c.len % 3u != 0 || c.len > 768u || seen_idat) return kPngParse;
            if (!C.plte) { C.plte = c.p; I.plte_entries = c.len / 3u; }
            break;
        case kTRNS:
            if (!crc_ok(c) || seen_idat) return kPngParse;
            if (I.color_type == 0 && c.len != 2) return kPngParse;
            if (I.color_type == 2 && c.len != 6) return kPngParse;
            if (I.color_type == 3 && (c.len > 256u || !C.plte)) return kPngParse; // (tRNS in front of PLTE: the png crate refuses it too)
            // (grey-alpha and RGBA pictures carry their own alpha: a tRNS there means nothing)
            if (I.color_type == 0 || I.color_type == 2 || I.color_type == 3) { C.trns = c.p; C.trns_len = c.len; I.has_trns = 1; }
            break;
        case kIDAT:
            if (!crc_ok(c) || idat_ended) return kPngParse; // IDAT chunks are consecutive (the png crate refuses others)
            if (!seen_idat) C.first_idat = at;
            seen_idat = true;
            I.idat_bytes += c.len;
            break;
        case kIEND:
            if (!crc_ok(c)) return kPngParse;
            seen_iend = true;
            break;
        default:
            // ancillary chunks (gAMA, sRGB, iCCP, eXIf, text, ...) are skipped uninterpreted; an unknown CRITICAL chunk
            // (upper-case first letter) is something a decoder must not ignore
            if (!(c.type & 0x20000000u)) return kPngParse;
            break;
        }
    }
    if (!seen_idat) return kPngParse;
    if (I.color_type == 3 && !C.plte) return kPngParse;
    const uint64_t row_bits = (uint64_t)I.width * samples * d;
    const uint64_t row_bytes = (row_bits + 7u) / 8u;
    I.bpp = samples * d >= 8u ? samples * d / 8u : 1u;
    I.pixel_bits = samples * d;
    uint32_t channels = 0;
    switch (I.color_type) {
    case 0: channels = I.has_trns ? 2u : 1u; break;
    case 2: channels = I.has_trns ? 4u : 3u; break;
    case 3: channels = I.has_trns ? 4u : 3u; break;
    case 4: channels = 2u; break;
    case 6: channels = 4u; break;
    }
    I.supported = d <= 8 && (!I.interlaced || adam7);
    const uint64_t scan = I.interlaced ? adam7_scan_bytes(I.width, I.height, I.pixel_bits) : (uint64_t)I.height * (1u + row_bytes);
    const uint64_t decoded = (uint64_t)I.width * I.height * channels;
    if (scan >= kPngMaxDecoded || decoded >= kPngMaxDecoded) I.supported = 0;
    I.row_bytes = row_bytes <= 0xffffffffu ? (uint32_t)row_bytes : 0u;
    I.channels = I.supported ? channels : 0u;
    // A deflate stream expands by at most 1032 : 1 (a length-258 match costs two bits at best), so a file whose IDAT
    // payload is shorter than that has too few bytes for the picture its header announces: nothing is reserved on the
    // say-so of a few hostile bytes.
    if (I.supported && scan > (I.idat_bytes + 1u) * 1032u) return kPngParse;
    return 0;
}

// ---- inflate ---------------------------------------------------------------------------------------------------------------------

// The compressed stream is the concatenation of the IDAT payloads: bytes are pulled from the file chunk by chunk (the
// walk above has verified lengths and CRCs), so nothing is copied and nothing allocated.
struct BitReader {
    const uint8_t *data; size_t n, pos; // pos: file offset of the next chunk header
    const uint8_t *cur = nullptr, *end = nullptr;
    uint64_t buf = 0;
    uint32_t cnt = 0;
    bool next_segment()
    {
        Chunk c;
        while (pos < n) {
            if (next_chunk(data, n, pos, c)) return false;
            if (c.type == kIEND) { pos = n; return false; }
            if (c.type == kIDAT && c.len) { cur = c.p; end = c.p + c.len; return true; }
        }
        return false;
    }
    inline void refill()
    {
        while (cnt <= 56) {
            if (cur == end && !next_segment()) return;
            if (end - cur >= 8) { // the common case in one load; the bits above cnt are those of the bytes that follow, so a later refill ORs the same bits again
                uint64_t v;
                memcpy(&v, cur, 8);
#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ == __ORDER_BIG_ENDIAN__
                v = __builtin_bswap64(v);
#endif
                buf |= v << cnt;
                const uint32_t k = (63u - cnt) >> 3;
                cur += k; cnt += 8u * k;
                return;
            }
            buf |= (uint64_t)*cur++ << cnt;
            cnt += 8;
        }
    }
    // true if `k` (<= 32) bits are available
    inline bool need(uint32_t k) { if (cnt < k) refill(); return cnt >= k; }
    inline uint32_t peek(uint32_t k) const { return (uint32_t)(buf & ((1ull << k) - 1u)); }
    inline void drop(uint32_t k) { buf >>= k; cnt -= k; }
    inline uint32_t take(uint32_t k) { const uint32_t v = peek(k); drop(k); return v; }
};

constexpr uint32_t kFastBits = 10;
struct Huffman {
    uint16_t fast[1u << kFastBits]; // (symbol << 4) | length, 0 = a longer code (or none)
    uint16_t count[16];
    uint16_t symbol[288];
    uint32_t max_len;
};

// Canonical code from lengths (RFC 1951 3.2.2).  false: over-subscribed, or incomplete with more than one code.
bool build(Huffman &h, const uint8_t *len, uint32_t nsym)
{
    memset(h.count, 0, sizeof(h.count));
    for (uint32_t s = 0; s < nsym; ++s) h.count[len[s]]++;
    memset(h.fast, 0, sizeof(h.fast));
    h.max_len = 0;
    if (h.count[0] == nsym) return true; // no codes at all: decoding any symbol fails
    int left = 1;
    for (uint32_t l = 1; l < 16; ++l) {
        left <<= 1;
        left -= h.count[l];
        if (left < 0) return false;
        if (h.count[l]) h.max_len = l;
    }
    if (left > 0 && nsym - h.count[0] != 1) return false;
    uint16_t offs[16];
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; ++l) offs[l + 1] = offs[l] + h.count[l];
    for (uint32_t s = 0; s < nsym; ++s) if (len[s]) h.symbol[offs[len[s]]++] = (uint16_t)s;
    // fast table: every code of up to kFastBits bits, bit-reversed (codes are packed starting from their top bit)
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= kFastBits; ++l) {
        for (uint32_t k = 0; k < h.count[l]; ++k, ++code, ++idx) {
            uint32_t rev = 0;
            for (uint32_t b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1 - b);
            const uint16_t e = (uint16_t)(h.symbol[idx] << 4 | l);
            for (uint32_t v = rev; v < (1u << kFastBits); v += 1u << l) h.fast[v] = e;
        }
        code <<= 1;
    }
    return true;
}

// One symbol: >= 0, or -1 (invalid code / out of input).
inline int decode(BitReader &br, const Huffman &h)
{
    if (br.cnt < 15) br.refill();
    const uint16_t e = h.fast[br.peek(kFastBits)];
    if (e) {
        const uint32_t l = e & 15u;
        if (l > br.cnt) return -1;
        br.drop(l);
        return e >> 4;
    }
    // longer codes, bit by bit
    int code = 0, first = 0, index = 0;
    uint64_t bits = br.buf;
    for (uint32_t l = 1; l <= h.max_len; ++l) {
        if (l > br.cnt) return -1;
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int count = h.count[l];
        if (code - count < first) { br.drop(l); return h.symbol[index + (code - first)]; }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

struct FixedTables {
    Huffman lit, dist;
    FixedTables()
    {
        uint8_t l[288];
        for (int s = 0; s < 144; ++s) l[s] = 8;
        for (int s = 144; s < 256; ++s) l[s] = 9;
        for (int s = 256; s < 280; ++s) l[s] = 7;
        for (int s = 280; s < 288; ++s) l[s] = 8;
        build(lit, l, 288);
        for (int s = 0; s < 32; ++s) l[s] = 5; // (codes 30 and 31 exist in the fixed code and are invalid in a stream)
        build(dist, l, 32);
    }
};

int codes(BitReader &br, const Huffman &lit, const Huffman &dist, uint8_t *out, size_t cap, size_t &pos)
{
    for (;;) {
        int sym = decode(br, lit);
        if (sym < 0) return kPngParse;
        if (sym < 256) {
            if (pos >= cap) return kPngUnsupported; // more scanline data than IHDR implies
            out[pos++] = (uint8_t)sym;
            continue;
        }
        if (sym == 256) return 0;
        sym -= 257;
        if (sym >= 29) return kPngParse;
        if (!br.need(kLenExtra[sym])) return kPngParse;
        const uint32_t len = kLenBase[sym] + br.take(kLenExtra[sym]);
        const int ds = decode(br, dist);
        if (ds < 0 || ds >= 30) return kPngParse;
        if (!br.need(kDistExtra[ds])) return kPngParse;
        const size_t d = (size_t)kDistBase[ds] + br.take(kDistExtra[ds]);
        if (d > pos) return kPngParse; // before the start of the stream
        if (len > cap - pos) return kPngUnsupported;
        const uint8_t *from = out + pos - d;
        uint8_t *to = out + pos;
        if (d >= len) memcpy(to, from, len);
        else for (uint32_t k = 0; k < len; ++k) to[k] = from[k]; // overlapping: the run repeats
        pos += len;
    }
}

int inflate(BitReader &br, uint8_t *out, size_t cap, size_t *produced)
{
    static const FixedTables fixed;
    size_t pos = 0;
    *produced = 0;
    // zlib header (RFC 1950): deflate, window <= 32 KB, check bits, no preset dictionary
    if (!br.need(16)) return kPngParse;
    const uint32_t cmf = br.take(8), flg = br.take(8);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return kPngParse;
    Huffman lit, dist;
    for (bool last = false; !last;) {
        if (!br.need(3)) return kPngParse;
        last = br.take(1) != 0;
        const uint32_t type = br.take(2);
        if (type == 0) {
            br.drop(br.cnt & 7u);
            if (!br.need(32)) return kPngParse;
            const uint32_t len = br.take(16), nlen = br.take(16);
            if ((len ^ nlen) != 0xffffu) return kPngParse;
            if (len > cap - pos) return kPngUnsupported;
            uint32_t left = len;
            while (left && br.cnt >= 8) { out[pos++] = (uint8_t)br.take(8); --left; } // bytes already in the bit buffer
            br.buf = br.cnt ? br.buf & ((1ull << br.cnt) - 1u) : 0; // (what refill() read ahead is skipped below)
            while (left) {
                if (br.cur == br.end && !br.next_segment()) return kPngParse;
                const size_t k = (size_t)(br.end - br.cur) < left ? (size_t)(br.end - br.cur) : left;
                memcpy(out + pos, br.cur, k);
                br.cur += k; pos += k; left -= (uint32_t)k;
            }
        } else if (type == 1) {
            const int rc = codes(br, fixed.lit, fixed.dist, out, cap, pos);
            if (rc) return rc;
        } else if (type == 2) {
            if (!br.need(14)) return kPngParse;
            const uint32_t nlen = br.take(5) + 257, ndist = br.take(5) + 1, ncode = br.take(4) + 4;
            if (nlen > 286 || ndist > 30) return kPngParse;
            static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint8_t lengths[320];
            memset(lengths, 0, sizeof(lengths));
            for (uint32_t k = 0; k < ncode; ++k) {
                if (!br.need(3)) return kPngParse;
                lengths[order[k]] = (uint8_t)br.take(3);
            }
            if (!build(lit, lengths, 19)) return kPngParse; // (lit doubles as the code-length code)
            uint32_t idx = 0;
            while (idx < nlen + ndist) {
                const int sym = decode(br, lit);
                if (sym < 0) return kPngParse;
                if (sym < 16) { lengths[idx++] = (uint8_t)sym; continue; }
                uint32_t rep, val = 0;
                if (sym == 16) {
                    if (idx == 0 || !br.need(2)) return kPngParse;
                    val = lengths[idx - 1];
                    rep = 3 + br.take(2);
                } else if (sym == 17) {
                    if (!br.need(3)) return kPngParse;
                    rep = 3 + br.take(3);
                } else {
                    if (!br.need(7)) return kPngParse;
                    rep = 11 + br.take(7);
                }
                if (idx + rep > nlen + ndist) return kPngParse;
                while (rep--) lengths[idx++] = (uint8_t)val;
            }
            if (lengths[256] == 0) return kPngParse; // no end-of-block code
            uint8_t dl[32];
            memcpy(dl, lengths + nlen, ndist);
            if (!build(lit, lengths, nlen) || !build(dist, dl, ndist)) return kPngParse;
            const int rc = codes(br, lit, dist, out, cap, pos);
            if (rc) return rc;
        } else {
            return kPngParse;
        }
    }
    *produced = pos;
    br.drop(br.cnt & 7u);
    if (!br.need(32)) return kPngParse; // the check value is missing
    uint32_t want = 0;
    for (int k = 0; k < 4; ++k) want = want << 8 | br.take(8);
    if (want != adler32(out, pos)) return kPngParse;
    return 0;
}

// the blob header of the picture `C` describes
void fill_header(const Container &C, uint32_t magic, size_t total_bytes, PngBlobHeader *hdr)
{
    const PngInfo &I = C.info;
    memset(hdr, 0, sizeof(*hdr));
    hdr->magic = magic;
    hdr->width = I.width; hdr->height = I.height;
    hdr->color_type = I.color_type; hdr->bit_depth = I.bit_depth;
    hdr->channels = I.channels; hdr->bpp = I.bpp; hdr->row_bytes = I.row_bytes;
    hdr->has_trns = I.has_trns;
    hdr->interlaced = I.interlaced;
    // (an interlaced picture's rows are never its pixels: the de-interlace kernel puts them together)
    hdr->direct = (I.bit_depth == 8 && I.color_type != 3 && !I.has_trns && !I.interlaced) ? 1u : 0u;
    hdr->scan_off = (uint32_t)sizeof(PngBlobHeader);
    hdr->total_bytes = (uint32_t)total_bytes;
    // the key is compared on the raw sample (its low byte: samples have at most 8 bits here)
    if (I.has_trns && I.color_type == 0) hdr->key[0] = C.trns[1];
    if (I.has_trns && I.color_type == 2) { hdr->key[0] = C.trns[1]; hdr->key[1] = C.trns[3]; hdr->key[2] = C.trns[5]; }
    for (uint32_t k = 0; k < 256; ++k) {
        uint32_t e = 0xff000000u; // beyond PLTE: opaque black
        if (I.color_type == 3) {
            if (k < I.plte_entries) e |= (uint32_t)C.plte[3 * k] | (uint32_t)C.plte[3 * k + 1] << 8 | (uint32_t)C.plte[3 * k + 2] << 16;
            if (I.has_trns && k < C.trns_len) e = (e & 0x00ffffffu) | (uint32_t)C.trns[k] << 24;
        }
        hdr->palette[k] = e;
    }
}

} // namespace

int png_parse_info(const uint8_t *data, size_t n, PngInfo &info, bool verify_crc, bool adam7)
{
    Container C;
    const int rc = walk(data, n, C, verify_crc, adam7);
    info = C.info;
    return rc;
}

int png_decode_scanlines(const uint8_t *data, size_t n, uint8_t *scan, size_t cap, PngBlobHeader *hdr, bool adam7)
{
    Container C;
    int rc = walk(data, n, C, true, adam7);
    if (rc) return rc;
    const PngInfo &I = C.info;
    if (!I.supported) return kPngUnsupported;
    const size_t want = png_scan_bytes(I);
    if (!scan || cap < want) return kPngSmall;
    BitReader br{data, n, C.first_idat};
    size_t produced = 0;
    rc = inflate(br, scan, want, &produced);
    if (rc) return rc;
    if (produced != want) return kPngParse; // too few bytes for the picture
    // the kernel never sees another filter type than 0..4: every row's filter byte, for an interlaced file every pass row's
    for (uint32_t p = 0; p < (I.interlaced ? kAdam7Passes : 1u); ++p) {
        const Adam7Pass P = I.interlaced ? adam7_pass(I.width, I.height, I.pixel_bits, p) : Adam7Pass{I.width, I.height, I.row_bytes, 0, 0};
        if (!P.w || !P.h) continue;
        const size_t stride = 1u + (size_t)P.row_bytes;
        for (uint32_t y = 0; y < P.h; ++y)
            if (scan[(size_t)P.scan_off + (size_t)y * stride] > 4u) return kPngParse;
    }
    if (hdr) fill_header(C, kPngMagic, sizeof(PngBlobHeader) + want, hdr);
    return 0;
}

// ---- sources whose deflate stream the device inflates ----------------------------------------------------------------------------

int png_stage_compressed(const uint8_t *data, size_t n, uint8_t *blob, size_t cap, PngBlobHeader *hdr, bool adam7)
{
    Container C;
    const int rc = walk(data, n, C, true, adam7);
    if (rc) return rc;
    const PngInfo &I = C.info;
    if (!I.supported) return kPngUnsupported;
    const size_t total = png_stage_bytes(I);
    if (!blob || !hdr || cap < total || total > 0xffffffffu) return kPngSmall;
    fill_header(C, kPngzMagic, total, hdr);
    memcpy(blob, hdr, sizeof(*hdr));
    uint8_t *to = blob + sizeof(PngBlobHeader);
    size_t pos = C.first_idat, left = (size_t)I.idat_bytes;
    Chunk c;
    while (left && next_chunk(data, n, pos, c) == 0 && c.type == kIDAT) { // (consecutive, and their lengths sum to idat_bytes: the walk has seen to both)
        if (c.len > left) return kPngParse;
        memcpy(to, c.p, c.len);
        to += c.len; left -= c.len;
    }
    if (left) return kPngParse;
    memset(to, 0, kPngzPad);
    return 0;
}

int png_inflate_model(const uint8_t *staged, size_t staged_bytes, uint8_t *out, size_t cap, uint32_t stats[8])
{
    uint32_t none[8];
    if (!stats) stats = none;
    memset(stats, 0, 8 * sizeof(uint32_t));
    PngBlobHeader H;
    if (!staged || staged_bytes < sizeof(H) + kPngzPad) return kPngParse;
    memcpy(&H, staged, sizeof(H));
    if (H.magic != kPngzMagic || H.total_bytes != staged_bytes) return kPngParse;
    const uint32_t payload = (uint32_t)(staged_bytes - sizeof(H) - kPngzPad);
    const size_t want = png_header_scan_bytes(H);
    if (want >= kPngMaxDecoded) return kPngParse;
    if (!out || cap < want) return kPngSmall;
    const uint32_t expected = (uint32_t)want;
    // the kernel's view of the payload: whole words, zero bits past them
    const uint64_t nwords = ((uint64_t)payload + kPngzPad) / 4u, total_bits = (uint64_t)payload * 8u;
    std::vector<uint32_t> words((size_t)nwords);
    memcpy(words.data(), staged + sizeof(H), (size_t)nwords * 4u);
    const uint8_t *bytes = staged + sizeof(H);
    // the kernel's LDS, array by array
    std::vector<uint32_t> window(kInfWindowWords), state(kInfSubs + 1u), seen(kInfSubs), cnt(kInfSubs), ntok(kInfSubs), in(kInfSubs), pos(kInfSubs), off(kInfSubs);
    std::vector<uint8_t> lengths(320), fin(kInfSubs);
    std::unique_ptr<InfTable> fixed_lit(new InfTable), fixed_dist(new InfTable), lit(new InfTable), dist(new InfTable), cl(new InfTable);

    if (payload < 2u) return kPngParse;
    {
        const uint32_t cmf = bytes[0], flg = bytes[1];
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return kPngParse;
    }
    inf_fixed_tables(*fixed_lit, *fixed_dist, lengths.data());
    uint64_t P = 16;
    uint32_t obase = 0, exact_total = 0;
    for (bool last = false; !last;) {
        if (total_bits - P < 3u) return kPngParse;
        stats[0]++;
        const uint64_t hw = P >> 5;
        const uint32_t hb = (uint32_t)P & 31u;
        for (uint32_t k = 0; k < kInfHeaderWords; ++k) window[k] = hw + k < nwords ? words[(size_t)(hw + k)] : 0u;
        const uint64_t hv = inf_peek(window.data(), kInfHeaderWords, hb);
        last = (hv & 1u) != 0;
        const uint32_t type = (uint32_t)(hv >> 1) & 3u;
        if (type == 3u) return kPngParse;
        if (type == 0u) {
            const uint64_t at = (P + 3u + 7u) >> 3;
            if (at + 4u > payload) return kPngParse;
            const uint32_t len = bytes[at] | (uint32_t)bytes[at + 1] << 8, nlen = bytes[at + 2] | (uint32_t)bytes[at + 3] << 8;
            if ((len ^ nlen) != 0xffffu) return kPngParse;
            if (len > payload - at - 4u) return kPngParse;
            if (len > expected - obase) return kPngParse;
            memcpy(out + obase, bytes + at + 4u, len);
            obase += len;
            P = (at + 4u + len) * 8u;
            continue;
        }
        const InfTable *L = fixed_lit.get(), *D = fixed_dist.get();
        if (type == 2u) {
            const uint64_t rem = total_bits - (hw << 5);
            const uint32_t q = inf_dynamic_header(window.data(), kInfHeaderWords, hb + 3u, rem > (1u << 28) ? 1u << 28 : (uint32_t)rem, *cl, *lit, *dist, lengths.data());
            if (!q) return kPngParse;
            P = (hw << 5) + q;
            L = lit.get(); D = dist.get();
        } else {
            P += 3u;
        }
        for (bool in_block = true; in_block;) {
            stats[1]++;
            const uint64_t wb = P >> 5;
            const uint32_t base = (uint32_t)P & 31u;
            for (uint32_t k = 0; k < kInfWindowWords; ++k) window[k] = wb + k < nwords ? words[(size_t)(wb + k)] : 0u;
            const uint64_t rem = total_bits - (wb << 5);
            const uint32_t limit = rem > (1u << 28) ? 1u << 28 : (uint32_t)rem;
            for (uint32_t t = 0; t < kInfSubs; ++t) { state[t] = base + t * kInfSubBits; seen[t] = kInfNever; cnt[t] = ntok[t] = 0; }
            // 1. synchronisation: every "thread" reads its state, then every thread whose state changed walks again
            bool settled = false;
            uint32_t rounds = 0;
            for (uint32_t round = 0; round < kInfSubs + 2u; ++round) {
                for (uint32_t t = 0; t < kInfSubs; ++t) in[t] = state[t];
                bool changed = false;
                for (uint32_t t = 0; t < kInfSubs; ++t) {
                    if (in[t] == seen[t]) continue;
                    seen[t] = in[t];
                    uint32_t st = kInfDead;
                    cnt[t] = ntok[t] = 0;
                    if (!(in[t] & kInfFlags)) {
                        st = inf_walk(*L, *D, window.data(), kInfWindowWords, in[t], base + (t + 1u) * kInfSubBits, limit, cnt[t], ntok[t]);
                        stats[4] += ntok[t];
                    }
                    state[t + 1u] = st;
                    changed = true;
                }
                if (!changed) { settled = true; break; }
                ++rounds;
            }
            if (!settled) return kPngParse;
            stats[2] += rounds;
            if (rounds > stats[6]) stats[6] = rounds;
            // 2. the block's end, the output offsets
            uint32_t e = kInfNever, total = 0;
            for (uint32_t t = 0; t < kInfSubs && e == kInfNever; ++t) if (state[t + 1u] & (kInfEob | kInfInvalid)) e = t;
            if (e != kInfNever && (state[e + 1u] & kInfInvalid)) return kPngParse;
            uint32_t exact = 0;
            for (uint32_t t = 0; t < kInfSubs; ++t) { off[t] = total; total += cnt[t]; exact += ntok[t]; }
            stats[5] = stats[4] - (exact_total += exact); // (stats[4] counts every walk: what is left once the exact tokens are taken off was decoded again)
            if (total > expected - obase) return kPngParse;
            // 3. write and resolve
            for (uint32_t t = 0; t < kInfSubs; ++t) { pos[t] = seen[t]; off[t] += obase; fin[t] = (seen[t] & kInfFlags) != 0; }
            uint32_t done = obase, rr = 0;
            for (;; ++rr) {
                if (rr > kInfStripBits + 1u) return kPngParse;
                uint32_t next = kInfNever;
                for (uint32_t t = 0; t < kInfSubs; ++t) {
                    if (fin[t]) continue;
                    const int r = inf_resolve(*L, *D, window.data(), kInfWindowWords, pos[t], base + (t + 1u) * kInfSubBits, off[t], done, out, expected);
                    if (r == kInfFail) return kPngParse;
                    if (r == kInfPending) { if (off[t] < next) next = off[t]; }
                    else fin[t] = 1;
                }
                if (next == kInfNever) break;
                done = next;
            }
            stats[3] += rr + 1u;
            if (rr + 1u > stats[7]) stats[7] = rr + 1u;
            obase += total;
            if (e != kInfNever) { P = (wb << 5) + (state[e + 1u] & ~kInfFlags); in_block = false; }
            else P = (wb << 5) + state[kInfSubs];
        }
    }
    if (obase != expected) return kPngParse;
    const uint64_t at = (P + 7u) >> 3;
    if (at + 4u > payload) return kPngParse;
    const uint32_t check = (uint32_t)bytes[at] << 24 | (uint32_t)bytes[at + 1] << 16 | (uint32_t)bytes[at + 2] << 8 | bytes[at + 3];
    uint64_t s1 = 0, s2 = 0;
    for (uint32_t j = 0; j < expected; j += 16u) {
        const uint32_t k = expected - j < 16u ? expected - j : 16u;
        inf_adler_piece(s1, s2, out + j, k, (expected - j) % kAdlerMod);
        s1 %= kAdlerMod; s2 %= kAdlerMod;
    }
    if (inf_adler_finish(s1, s2, expected) != check) return kPngParse;
    for (uint32_t p = 0; p < (H.interlaced ? kAdam7Passes : 1u); ++p) {
        const Adam7Pass A = H.interlaced ? adam7_pass(H.width, H.height, png_pixel_bits(H), p) : Adam7Pass{H.width, H.height, H.row_bytes, 0, 0};
        if (!A.w || !A.h) continue;
        const size_t stride = 1u + (size_t)A.row_bytes;
        for (uint32_t y = 0; y < A.h; ++y)
            if (out[(size_t)A.scan_off + (size_t)y * stride] > 4u) return kPngParse;
    }
    return 0;
}

} // namespace fl
