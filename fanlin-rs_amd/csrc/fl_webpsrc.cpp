// fl_webpsrc.cpp -- host half of the lossless WebP decode front end: RIFF container, VP8L headers, prefix codes, LZ77 with the
// short-distance map, colour cache, meta prefix codes, and the sub-images of the transforms (each an entropy-coded image of
// its own).  See fl_webpsrc.h.  Plain C++: no HIP, no allocation in the decode path (the caller's buffer holds the blob in
// front and the work area -- entropy image and code tables -- at its end).
#include "fl_webpsrc.h"

#include <string.h>

#include <vector>

namespace fl {

namespace {

inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15u; }

// ---- bit reader: LSB first; bits past the end read as zero and set eos() once one of them has been consumed ----------------
struct Bits {
    const uint8_t *p;
    size_t n, pos = 0;
    uint64_t val = 0;
    int have = 0, fake = 0; // bits in val; how many of them lie past the end of the data
    Bits(const uint8_t *d, size_t len) : p(d), n(len) {}
    inline void fill()
    {
        if (have > 32) return;
        if (pos + 4 <= n) {
            uint32_t w;
            memcpy(&w, p + pos, 4);
            val |= (uint64_t)w << have; have += 32; pos += 4;
            return;
        }
        while (have <= 56) {
            if (pos < n) val |= (uint64_t)p[pos++] << have; else if (fake < 4096) fake += 8; else break;
            have += 8;
        }
    }
    inline void drop(int k) { val >>= k; have -= k; }
    inline uint32_t get(int k) // k <= 24
    {
        fill();
        const uint32_t v = (uint32_t)val & ((1u << k) - 1u);
        drop(k);
        return v;
    }
    inline bool eos() const { return have < fake; }
};

// ---- prefix codes ----------------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxAlphabet = 256 + 24 + (1u << 11);
constexpr uint8_t kClOrder[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};

#ifndef FL_WEBP_FAST_BITS
#define FL_WEBP_FAST_BITS 10
#endif
constexpr uint32_t kFastBits = FL_WEBP_FAST_BITS, kFastSize = 1u << kFastBits;

struct Code {
    uint16_t count[16]; // symbols per code length
    uint16_t *syms;     // the used symbols, sorted by (length, symbol)
    uint16_t *fast;     // kFastSize entries: length << 12 | symbol for codes of up to kFastBits bits, 0 = a longer one; may be null
    uint16_t nsyms, single; // nsyms == 1: `single` is the symbol, and reading it consumes no bits
};
struct Group { Code c[5]; };

// Two-ended arena over the caller's buffer: the blob grows from the front, the work area from the back.
struct Arena {
    uint8_t *base, *front, *back;
    void *take_back(size_t bytes)
    {
        bytes = (bytes + 7u) & ~(size_t)7u;
        if ((size_t)(back - front) < bytes) return nullptr;
        back -= bytes;
        return back;
    }
    void *take_front(size_t bytes)
    {
        bytes = align16(bytes);
        if ((size_t)(back - front) < bytes) return nullptr;
        void *p = front;
        front += bytes;
        return p;
    }
};

// lengths[0 .. n) -> a Code in the work area.  kWebpParse for an over-subscribed or incomplete code; one used symbol is
// complete by definition, whatever its length.
int build_code(const uint8_t *lengths, uint32_t n, Arena &A, Code &c, bool want_fast)
{
    memset(c.count, 0, sizeof(c.count));
    uint32_t used = 0;
    for (uint32_t s = 0; s < n; ++s) { c.count[lengths[s]]++; used += lengths[s] != 0; }
    c.count[0] = 0;
    if (!used) return kWebpParse;
    c.nsyms = (uint16_t)used;
    c.fast = nullptr;
    c.syms = static_cast<uint16_t *>(A.take_back(used * sizeof(uint16_t)));
    if (!c.syms) return kWebpUnsupported;
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + c.count[l]);
    for (uint32_t s = 0; s < n; ++s) if (lengths[s]) c.syms[offs[lengths[s]]++] = (uint16_t)s;
    c.single = c.syms[0];
    if (used == 1) return 0;
    int left = 1;
    for (int l = 1; l <= 15; ++l) {
        left <<= 1;
        left -= c.count[l];
        if (left < 0) return kWebpParse;
    }
    if (left != 0) return kWebpParse;
    if (!want_fast) return 0;
    c.fast = static_cast<uint16_t *>(A.take_back(kFastSize * sizeof(uint16_t)));
    if (!c.fast) return 0; // (the work area is full: this code is read bit by bit)
    memset(c.fast, 0, kFastSize * sizeof(uint16_t));
    uint32_t code = 0, idx = 0;
    for (uint32_t l = 1; l <= kFastBits; ++l) {
        for (uint32_t k = 0; k < c.count[l]; ++k, ++code, ++idx) {
            uint32_t rev = 0;
            for (uint32_t b = 0; b < l; ++b) rev |= ((code >> b) & 1u) << (l - 1u - b);
            for (uint32_t r = rev; r < kFastSize; r += 1u << l) c.fast[r] = (uint16_t)(l << 12 | c.syms[idx]);
        }
        code <<= 1;
    }
    return 0;
}

inline int read_sym(Bits &b, const Code &c)
{
    if (c.nsyms == 1) return c.single;
    b.fill();
    if (c.fast) {
        const uint32_t e = c.fast[b.val & (kFastSize - 1u)];
        if (e) { b.drop((int)(e >> 12)); return (int)(e & 0xfffu); }
    }
    uint32_t v = (uint32_t)b.val;
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)(v & 1u);
        v >>= 1;
        const int cnt = c.count[l];
        if (code - cnt < first) { b.drop(l); return c.syms[index + (code - first)]; }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

int read_code(Bits &b, uint32_t alphabet, Arena &A, Code &c, bool want_fast)
{
    uint8_t lengths[kMaxAlphabet];
    memset(lengths, 0, alphabet);
    if (b.get(1)) { // simple: one or two symbols of length 1
        const uint32_t two = b.get(1);
        const uint32_t s0 = b.get(b.get(1) ? 8 : 1);
        lengths[s0] = 1; // (every alphabet has at least 40 symbols; 8-bit symbols beyond a 40-symbol alphabet are refused below)
        uint32_t s1 = 0;
        if (two) { s1 = b.get(8); if (s1 < alphabet) lengths[s1] = 1; }
        if (s0 >= alphabet || s1 >= alphabet) return kWebpParse;
    } else {
        uint8_t cl[19];
        memset(cl, 0, sizeof(cl));
        const uint32_t ncl = b.get(4) + 4u;
        for (uint32_t k = 0; k < ncl; ++k) cl[kClOrder[k]] = (uint8_t)b.get(3);
        Arena T = A; // the code-length code lives only as long as this function
        Code clc;
        int rc = build_code(cl, 19, T, clc, false);
        if (rc) return rc;
        uint32_t max_symbol = alphabet;
        if (b.get(1)) {
            const int nb = 2 + 2 * (int)b.get(3);
            max_symbol = 2u + b.get(nb);
            if (max_symbol > alphabet) return kWebpParse;
        }
        uint32_t s = 0, prev = 8;
        while (s < alphabet) {
            if (max_symbol-- == 0) break;
            const int l = read_sym(b, clc);
            if (l < 0 || b.eos()) return kWebpParse;
            if (l < 16) { lengths[s++] = (uint8_t)l; if (l) prev = (uint32_t)l; continue; }
            const uint32_t rep = l == 16 ? 3u + b.get(2) : l == 17 ? 3u + b.get(3) : 11u + b.get(7);
            if (s + rep > alphabet) return kWebpParse;
            memset(lengths + s, l == 16 ? (int)prev : 0, rep);
            s += rep;
        }
    }
    if (b.eos()) return kWebpParse;
    return build_code(lengths, alphabet, A, c, want_fast);
}

// ---- the short-distance map -------------------------------------------------------------------------------------------------
constexpr uint8_t kCodeToPlane[120] = {
    0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a,
    0x25, 0x2b, 0x48, 0x04, 0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03,
    0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d, 0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e,
    0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e, 0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f,
    0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e, 0x00, 0x74, 0x7c, 0x41,
    0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};

inline uint32_t plane_distance(uint32_t xsize, uint32_t code)
{
    if (code > 120u) return code - 120u;
    const uint32_t e = kCodeToPlane[code - 1u];
    const int64_t d = (int64_t)(e >> 4) * xsize + (8 - (int)(e & 15u));
    return d >= 1 ? (uint32_t)d : 1u; // a distance that lands before the picture's start of row: 1
}

// length / distance prefix symbol -> value, with its extra bits
inline uint32_t read_lz_value(Bits &b, uint32_t sym)
{
    if (sym < 4u) return sym + 1u;
    const uint32_t extra = (sym - 2u) >> 1;
    const uint32_t offset = (2u + (sym & 1u)) << extra;
    return offset + b.get((int)extra) + 1u;
}

struct Decoder {
    Bits b;
    Arena A;
    bool header_only = false; // deep info: stop in front of the main image's pixels
    uint32_t cache_bits0 = 0, groups0 = 0;
    Decoder(const uint8_t *d, size_t n) : b(d, n) {}

    // an entropy-coded image of w x h dwords into out; level0 = the main image (meta prefix codes allowed)
    int image(uint32_t w, uint32_t h, bool level0, uint32_t *out)
    {
        uint32_t cache_bits = 0;
        if (b.get(1)) {
            cache_bits = b.get(4);
            if (cache_bits < 1u || cache_bits > 11u) return kWebpParse;
        }
        const uint32_t *entropy = nullptr;
        uint32_t ebits = 0, ew = 0, ngroups = 1;
        uint8_t *const back_on_entry = A.back;
        if (level0 && b.get(1)) {
            ebits = b.get(3) + 2u;
            ew = webp_subsample(w, ebits);
            const uint32_t eh = webp_subsample(h, ebits);
            uint32_t *e = static_cast<uint32_t *>(A.take_back((size_t)ew * eh * 4u));
            if (!e) return kWebpUnsupported;
            const int rc = image(ew, eh, false, e);
            if (rc) return rc;
            uint32_t mx = 0;
            for (size_t i = 0; i < (size_t)ew * eh; ++i) { e[i] = (e[i] >> 8) & 0xffffu; mx = e[i] > mx ? e[i] : mx; }
            ngroups = mx + 1u;
            entropy = e;
        }
        if (b.eos()) return kWebpParse;
        Group *groups = static_cast<Group *>(A.take_back((size_t)ngroups * sizeof(Group)));
        if (!groups) return kWebpUnsupported;
        const uint32_t alpha0 = 256u + 24u + (cache_bits ? 1u << cache_bits : 0u);
        for (uint32_t g = 0; g < ngroups; ++g) {
            const uint32_t sizes[5] = {alpha0, 256u, 256u, 256u, 40u};
            for (int k = 0; k < 5; ++k) {
                const int rc = read_code(b, sizes[k], A, groups[g].c[k], true);
                if (rc) return rc;
            }
        }
        if (level0) { cache_bits0 = cache_bits; groups0 = ngroups; }
        if (level0 && header_only) return 0;
        const int rc = pixels(w, h, out, cache_bits, groups, entropy, ebits, ew);
        if (!level0) A.back = back_on_entry; // a sub-image's tables are done with
        return rc;
    }

    int pixels(uint32_t w, uint32_t h, uint32_t *out, uint32_t cache_bits, const Group *groups, const uint32_t *entropy, uint32_t ebits, uint32_t ew)
    {
        uint32_t cache[1u << 11];
        if (cache_bits) memset(cache, 0, sizeof(uint32_t) << cache_bits);
        const int cshift = 32 - (int)cache_bits;
        const size_t end = (size_t)w * h;
        const uint32_t mask = entropy ? (1u << ebits) - 1u : ~0u;
        const uint32_t cache_limit = 280u + (cache_bits ? 1u << cache_bits : 0u);
        size_t pos = 0;
        uint32_t col = 0, row = 0;
        const Group *G = groups;
        while (pos < end) {
            if (entropy && (col & mask) == 0u) G = groups + entropy[(size_t)(row >> ebits) * ew + (col >> ebits)];
            const int s = read_sym(b, G->c[0]);
            if (s < 0) return kWebpParse;
            if (s < 256 || (uint32_t)s >= 280u) {
                uint32_t px;
                if (s < 256) {
                    const int r = read_sym(b, G->c[1]), bl = read_sym(b, G->c[2]), a = read_sym(b, G->c[3]);
                    if ((r | bl | a) < 0) return kWebpParse;
                    px = (uint32_t)a << 24 | (uint32_t)r << 16 | (uint32_t)s << 8 | (uint32_t)bl;
                } else {
                    if (!cache_bits || (uint32_t)s >= cache_limit) return kWebpParse; // a cache index without a cache
                    px = cache[s - 280];
                }
                if (b.eos()) return kWebpParse;
                out[pos++] = px;
                if (cache_bits) cache[(px * 0x1e35a7bdu) >> cshift] = px;
                if (++col == w) { col = 0; ++row; }
                continue;
            }
            const uint32_t len = read_lz_value(b, (uint32_t)s - 256u);
            const int ds = read_sym(b, G->c[4]);
            if (ds < 0) return kWebpParse;
            const uint32_t dist = plane_distance(w, read_lz_value(b, (uint32_t)ds));
            if (b.eos()) return kWebpParse;
            if (dist > pos || len > end - pos) return kWebpParse; // before pixel 0; past the last pixel
            for (uint32_t k = 0; k < len; ++k) {
                const uint32_t px = out[pos - dist];
                out[pos++] = px;
                if (cache_bits) cache[(px * 0x1e35a7bdu) >> cshift] = px;
            }
            col += len;
            while (col >= w) { col -= w; ++row; }
            if (entropy && pos < end && (col & mask)) G = groups + entropy[(size_t)(row >> ebits) * ew + (col >> ebits)];
        }
        return 0;
    }
};

// transforms + main image of one VP8L payload into the arena; H is filled as the stream is read
int decode_stream(const WebpInfo &info, Decoder &D, WebpBlobHeader &H, bool headerless = false)
{
    Bits &b = D.b;
    if (!headerless) { b.get(8); b.get(14); b.get(14); b.get(1); b.get(3); } // signature, sizes, alpha, version: webp_parse_info has read them
    memset(&H, 0, sizeof(H));
    H.magic = kWebpMagic;
    H.width = info.width; H.height = info.height; H.channels = info.channels;
    uint32_t xsize = info.width, seen = 0;
    while (b.get(1)) {
        const uint32_t t = b.get(2);
        if (seen & (1u << t)) return kWebpParse; // each kind at most once
        seen |= 1u << t;
        const uint32_t k = H.ntransforms++;
        H.ttype[k] = t;
        H.twidth[k] = xsize;
        if (t == kWtPredictor || t == kWtCrossColor) {
            const uint32_t bits = b.get(3) + 2u;
            const uint32_t bw = webp_subsample(xsize, bits), bh = webp_subsample(info.height, bits);
            uint32_t *img = static_cast<uint32_t *>(D.A.take_front((size_t)bw * bh * 4u));
            if (!img) return kWebpSmall;
            H.tbits[k] = bits;
            H.toff[k] = (uint32_t)(reinterpret_cast<uint8_t *>(img) - D.A.base);
            const int rc = D.image(bw, bh, false, img);
            if (rc) return rc;
        } else if (t == kWtColorIndexing) {
            const uint32_t ncol = b.get(8) + 1u;
            uint32_t *pal = static_cast<uint32_t *>(D.A.take_front(256u * 4u));
            if (!pal) return kWebpSmall;
            memset(pal, 0, 256u * 4u);
            H.tbits[k] = ncol;
            H.toff[k] = (uint32_t)(reinterpret_cast<uint8_t *>(pal) - D.A.base);
            const int rc = D.image(ncol, 1, false, pal);
            if (rc) return rc;
            for (uint32_t i = 1; i < ncol; ++i) { // delta-coded, per byte
                const uint32_t p = pal[i - 1], c = pal[i];
                pal[i] = (((c & 0xff00ff00u) + (p & 0xff00ff00u)) & 0xff00ff00u) | (((c & 0x00ff00ffu) + (p & 0x00ff00ffu)) & 0x00ff00ffu);
            }
            xsize = webp_subsample(xsize, webp_index_shift(ncol));
        }
        if (b.eos()) return kWebpParse;
    }
    H.xsize = xsize;
    H.res_off = (uint32_t)(D.A.front - D.A.base);
    H.total_bytes = H.res_off + xsize * info.height * 4u;
    uint32_t *res = nullptr;
    if (!D.header_only) {
        res = static_cast<uint32_t *>(D.A.take_front((size_t)xsize * info.height * 4u));
        if (!res) return kWebpSmall;
    }
    const int rc = D.image(xsize, info.height, true, res);
    if (rc) return rc;
    return b.eos() ? kWebpParse : 0;
}

size_t work_bytes(const WebpInfo &info, size_t file_bytes)
{
    // entropy image, and the code tables: a group of five codes takes 280 bytes, its used symbols two bytes each, a first-level
    // table 2 KiB a code while there is room; a file cannot describe more symbols than it has bits
    return (size_t)webp_subsample(info.width, 2) * webp_subsample(info.height, 2) * 4u + ((size_t)256 << 10) + 2u * file_bytes;
}

// The deep header walk: transform headers and the main image's code groups, without the main image's pixels.  The sub-images in front
// of them have to be entropy-decoded, into a work area of this call's own, bounded like the decode's.
int walk_headers(const WebpInfo &info, const uint8_t *stream, size_t len, size_t file_bytes, bool headerless, WebpBlobHeader &H, uint32_t &cache_bits, uint32_t &groups)
{
    const size_t sub = align16((size_t)webp_subsample(info.width, 2) * webp_subsample(info.height, 2) * 4u);
    std::vector<uint8_t> work(sizeof(WebpBlobHeader) + 2u * sub + 1024u + work_bytes(info, file_bytes) + 64u);
    Decoder D(stream, len);
    D.header_only = true;
    uint8_t *base = work.data() + ((16u - (reinterpret_cast<uintptr_t>(work.data()) & 15u)) & 15u);
    D.A = Arena{base, base + sizeof(WebpBlobHeader), work.data() + work.size()};
    D.A.back -= reinterpret_cast<uintptr_t>(D.A.back) & 7u;
    const int rc = decode_stream(info, D, H, headerless);
    cache_bits = D.cache_bits0; groups = D.groups0;
    return rc;
}

} // namespace

size_t webp_blob_capacity(const WebpInfo &info, size_t file_bytes)
{
    const size_t sub = align16((size_t)webp_subsample(info.width, 2) * webp_subsample(info.height, 2) * 4u);
    return sizeof(WebpBlobHeader) + 2u * sub + 1024u + align16((size_t)info.width * info.height * 4u) + work_bytes(info, file_bytes) + 64u;
}

int webp_parse_info(const uint8_t *d, size_t n, WebpInfo &info, bool deep)
{
    info = WebpInfo{};
    if (!d || n < 20 || memcmp(d, "RIFF", 4) || memcmp(d + 8, "WEBP", 4)) return kWebpParse;
    if ((uint64_t)le32(d + 4) + 8u != n || (n & 1u)) return kWebpParse; // the RIFF size is the file's
    size_t pos = 12;
    bool first = true, lossy = false, have_image = false;
    uint32_t canvas_w = 0, canvas_h = 0;
    while (pos < n) {
        if (n - pos < 8) return kWebpParse;
        const uint8_t *tag = d + pos;
        const uint32_t len = le32(d + pos + 4);
        if (len > n - pos - 8) return kWebpParse;
        if ((len & 1u) && (size_t)len + 1u > n - pos - 8) return kWebpParse; // the padding byte of an odd chunk
        const uint8_t *p = d + pos + 8;
        if (first && !memcmp(tag, "VP8X", 4)) {
            if (len < 10) return kWebpParse;
            info.extended = 1;
            info.has_alpha = (p[0] >> 4) & 1u;
            info.animated = (p[0] >> 1) & 1u;
            canvas_w = 1u + ((uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16);
            canvas_h = 1u + ((uint32_t)p[7] | (uint32_t)p[8] << 8 | (uint32_t)p[9] << 16);
        } else if (!memcmp(tag, "ANIM", 4) || !memcmp(tag, "ANMF", 4)) {
            if (!info.extended) return kWebpParse;
            info.animated = 1;
        } else if (!memcmp(tag, "VP8L", 4)) {
            if (!first && !info.extended) return kWebpParse;
            if (!have_image) {
                have_image = true;
                if (len < 5 || p[0] != 0x2f) return kWebpParse;
                const uint32_t v = le32(p + 1);
                if ((v >> 29) != 0u) return kWebpParse; // version
                info.lossless = 1;
                info.width = (v & 0x3fffu) + 1u;
                info.height = ((v >> 14) & 0x3fffu) + 1u;
                if (!info.extended) info.has_alpha = (v >> 28) & 1u;
                info.vp8l_off = pos + 8; info.vp8l_len = len;
            }
        } else if (!memcmp(tag, "VP8 ", 4)) {
            if (!first && !info.extended) return kWebpParse;
            if (!have_image) {
                have_image = lossy = true;
                if (len >= 10 && p[3] == 0x9d && p[4] == 0x01 && p[5] == 0x2a) {
                    info.width = ((uint32_t)p[6] | (uint32_t)p[7] << 8) & 0x3fffu;
                    info.height = ((uint32_t)p[8] | (uint32_t)p[9] << 8) & 0x3fffu;
                }
            }
        } else if (!memcmp(tag, "EXIF", 4)) {
            if (info.extended && !info.exif_len) { info.exif_off = pos + 8; info.exif_len = len; }
        } else if (first) return kWebpParse; // a file starts with VP8, VP8L or VP8X
        // (ALPH, ICCP, "XMP " and unknown chunks are skipped)
        first = false;
        pos += 8u + (size_t)len + (len & 1u);
    }
    if (info.animated) { info.width = canvas_w; info.height = canvas_h; return 0; }
    if (!have_image) return kWebpParse;
    if (lossy) return 0;
    if (info.extended && (canvas_w != info.width || canvas_h != info.height)) return kWebpParse;
    if ((uint64_t)info.width * info.height * 4u >= kWebpMaxDecoded) return 0;
    info.channels = info.has_alpha ? 4u : 3u;
    info.supported = 1;
    if (!deep) return 0;
    // transform headers and the main image's code groups: their sub-images have to be entropy-decoded to get past them
    WebpBlobHeader H;
    uint32_t cache_bits = 0, groups = 0;
    const int rc = walk_headers(info, d + info.vp8l_off, info.vp8l_len, n, false, H, cache_bits, groups);
    if (rc == kWebpUnsupported) { info.supported = 0; info.channels = 0; return 0; }
    if (rc) return kWebpParse;
    for (uint32_t k = 0; k < H.ntransforms; ++k) info.transforms |= 1u << H.ttype[k];
    info.color_cache_bits = cache_bits;
    info.prefix_groups = groups;
    info.blob_bytes = H.total_bytes;
    return 0;
}

// The VP8L-coded plane of a lossy picture's ALPH chunk: the stream without its five header bytes, the frame's sizes, the values in
// the green channel.  The blob is a lossless picture's (four output channels: the device writes R, G, B, A and green is taken).
static WebpInfo alpha_info(uint32_t width, uint32_t height)
{
    WebpInfo info;
    info.width = width; info.height = height; info.channels = 4; info.has_alpha = 1; info.lossless = 1; info.supported = 1;
    return info;
}

size_t webp_alpha_blob_capacity(uint32_t width, uint32_t height, size_t stream_bytes) { return webp_blob_capacity(alpha_info(width, height), stream_bytes); }

int webp_decode_alpha_residuals(const uint8_t *d, size_t n, uint32_t width, uint32_t height, uint8_t *blob, size_t cap, WebpBlobHeader *hdr)
{
    const WebpInfo info = alpha_info(width, height);
    if (!d || !width || !height || (uint64_t)width * height * 4u >= kWebpMaxDecoded) return kWebpParse;
    if (!blob || (reinterpret_cast<uintptr_t>(blob) & 15u) || cap < sizeof(WebpBlobHeader) + 64u) return kWebpSmall;
    Decoder D(d, n);
    D.A = Arena{blob, blob + sizeof(WebpBlobHeader), blob + (cap & ~(size_t)7u)};
    WebpBlobHeader H;
    const int rc = decode_stream(info, D, H, true);
    if (rc) return rc;
    memcpy(blob, &H, sizeof(H));
    if (hdr) *hdr = H;
    return 0;
}

int webp_alpha_blob_bytes(const uint8_t *d, size_t n, uint32_t width, uint32_t height, uint32_t *bytes)
{
    // as the deep parse of a lossless file: the transforms' sub-images are decoded into a work area of this call's own, the plane is not
    const WebpInfo info = alpha_info(width, height);
    if (!d || !width || !height || (uint64_t)width * height * 4u >= kWebpMaxDecoded) return kWebpParse;
    WebpBlobHeader H;
    uint32_t cache_bits = 0, groups = 0;
    const int rc = walk_headers(info, d, n, n, true, H, cache_bits, groups);
    if (rc) return rc;
    *bytes = H.total_bytes;
    return 0;
}

int webp_decode_residuals(const uint8_t *d, size_t n, uint8_t *blob, size_t cap, WebpBlobHeader *hdr)
{
    WebpInfo info;
    const int prc = webp_parse_info(d, n, info, false);
    if (prc) return prc;
    if (!info.supported) return kWebpUnsupported;
    if (!blob || (reinterpret_cast<uintptr_t>(blob) & 15u) || cap < sizeof(WebpBlobHeader) + 64u) return kWebpSmall;
    Decoder D(d + info.vp8l_off, info.vp8l_len);
    D.A = Arena{blob, blob + sizeof(WebpBlobHeader), blob + (cap & ~(size_t)7u)};
    WebpBlobHeader H;
    const int rc = decode_stream(info, D, H);
    if (rc) return rc;
    memcpy(blob, &H, sizeof(H));
    if (hdr) *hdr = H;
    return 0;
}

} // namespace fl
