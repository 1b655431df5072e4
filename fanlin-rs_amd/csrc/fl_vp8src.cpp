// fl_vp8src.cpp -- host half of the lossy WebP decode front end: RIFF container, VP8 frame tag and first partition (segments,
// filter, partitions, quantisers, probability updates, per macroblock segment id / skip flag / modes), token partitions into
// levels.  See fl_vp8src.h.  Plain C++: no HIP, no allocation (the caller's buffer holds the blob; the contexts of one
// macroblock row live on the stack, bounded by the 14-bit width).  Streams end as libwebp's reader ends them: bits past a
// partition's last byte read as zero, and a macroblock (row of modes) that needed one of them is kVp8Parse.
#include "fl_vp8src.h"

#include <string.h>

#include "fl_vp8_core.h"
#include "fl_vp8_dtables.h"
#include "fl_webpsrc.h"

namespace fl {

namespace {

inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le24(const uint8_t *p) { return le16(p) | (uint32_t)p[2] << 16; }
inline uint32_t le32(const uint8_t *p) { return le24(p) | (uint32_t)p[3] << 24; }
inline size_t align16(size_t v) { return (v + 15u) & ~(size_t)15u; }
inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// ---- boolean decoder (section 7), a byte at a time; `range` holds the range minus one -------------------------------------------
struct BoolDec {
    const uint8_t *p = nullptr, *end = nullptr;
    uint64_t value = 0;
    uint32_t range = 254;
    int bits = -8;
    bool eof = false;
    void init(const uint8_t *d, size_t n) { p = d; end = d + n; value = 0; range = 254; bits = -8; eof = false; load(); }
    inline void load()
    {
        if (p < end) { value = (value << 8) | *p++; bits += 8; }
        else if (!eof) { value <<= 8; bits += 8; eof = true; } // the first byte past the end: zeros, and the stream has ended
        else bits = 0;
    }
    inline int get(uint32_t prob)
    {
        if (bits < 0) load();
        const uint32_t split = (range * prob) >> 8, v = (uint32_t)(value >> bits);
        int bit;
        uint32_t r;
        if (v > split) { r = range - split; value -= (uint64_t)(split + 1u) << bits; bit = 1; }
        else { r = split + 1u; bit = 0; }
        const int shift = __builtin_clz(r) - 24;
        bits -= shift;
        range = (r << shift) - 1u;
        return bit;
    }
    inline uint32_t literal(int n) { uint32_t v = 0; while (n-- > 0) v |= (uint32_t)get(128) << n; return v; }
    inline int signed_literal(int n) { const int v = (int)literal(n); return get(128) ? -v : v; }
};

constexpr uint32_t kMaxMbw = (kVp8MaxSide + 15u) / 16u;

struct Frame {
    uint32_t width = 0, height = 0, mbw = 0, mbh = 0;
    bool use_segment = false, update_map = false;
    int quant[4] = {0, 0, 0, 0}, fstrength[4] = {0, 0, 0, 0};
    uint8_t segp[3] = {255, 255, 255};
    bool simple = false;
    int level = 0, sharpness = 0;
    uint32_t nparts = 1;
    int base_q = 0, dq[5] = {0, 0, 0, 0, 0}; // y1 dc, y2 dc, y2 ac, uv dc, uv ac
    bool use_skip = false;
    uint32_t skip_p = 0;
    uint8_t prob[4 * 8 * 3 * 11];
    BoolDec br, part[8];
};

// frame tag, start code, sizes, and the first partition up to the first macroblock
int parse_frame(const uint8_t *d, size_t n, Frame &F, Vp8Info &info)
{
    if (n < 10) return kVp8Parse;
    const uint32_t tag = le24(d);
    const uint32_t key = !(tag & 1u), version = (tag >> 1) & 7u, show = (tag >> 4) & 1u, part0 = tag >> 5;
    if (!key || !show || version > 3u) return kVp8Parse; // what WebPDecode refuses: an inter frame, a hidden one, an unknown profile
    if (d[3] != 0x9d || d[4] != 0x01 || d[5] != 0x2a) return kVp8Parse;
    F.width = le16(d + 6) & 0x3fffu; F.height = le16(d + 8) & 0x3fffu; // (the scale bits are ignored)
    if (!F.width || !F.height) return kVp8Parse;
    F.mbw = (F.width + 15u) >> 4; F.mbh = (F.height + 15u) >> 4;
    info.width = F.width; info.height = F.height; info.version = version;
    if (part0 > n - 10) return kVp8Parse;
    BoolDec &br = F.br;
    br.init(d + 10, part0);
    if (br.literal(1)) info.refused = "the colour-space bit of the frame header";
    if (br.literal(1)) info.refused = "the clamping bit of the frame header";
    // segment header
    F.use_segment = br.literal(1);
    if (F.use_segment) {
        F.update_map = br.literal(1);
        if (br.literal(1)) {
            if (!br.literal(1)) info.refused = "segment quantiser / filter values in delta mode";
            for (int s = 0; s < 4; ++s) F.quant[s] = br.literal(1) ? br.signed_literal(7) : 0;
            for (int s = 0; s < 4; ++s) F.fstrength[s] = br.literal(1) ? br.signed_literal(6) : 0;
        }
        if (F.update_map) for (int s = 0; s < 3; ++s) F.segp[s] = br.literal(1) ? (uint8_t)br.literal(8) : 255u;
    }
    if (br.eof) return kVp8Parse;
    // filter header
    F.simple = br.literal(1);
    F.level = (int)br.literal(6);
    F.sharpness = (int)br.literal(3);
    if (br.literal(1) && br.literal(1)) { // loop_filter_adj_enable, and the deltas are sent
        for (int i = 0; i < 8; ++i) if (br.literal(1) && br.signed_literal(6) != 0) info.refused = i < 4 ? "a non-zero ref_lf_delta" : "a non-zero mode_lf_delta";
    }
    if (br.eof) return kVp8Parse;
    // partitions: the sizes of all but the last follow partition 0; a size that reaches past the file is cut (as libwebp cuts
    // it: such a partition then ends early), a last partition without a byte is refused
    F.nparts = 1u << br.literal(2);
    {
        const uint8_t *sz = d + 10 + part0, *end = d + n;
        size_t left = (size_t)(end - sz);
        if (left < 3u * (F.nparts - 1u)) return kVp8Parse;
        const uint8_t *start = sz + 3u * (F.nparts - 1u);
        left -= 3u * (F.nparts - 1u);
        for (uint32_t k = 0; k + 1u < F.nparts; ++k, sz += 3) {
            size_t psize = le24(sz);
            if (psize > left) psize = left;
            F.part[k].init(start, psize);
            start += psize; left -= psize;
        }
        if (start >= end) return kVp8Parse;
        F.part[F.nparts - 1u].init(start, left);
    }
    // quantiser indices
    F.base_q = (int)br.literal(7);
    for (int i = 0; i < 5; ++i) F.dq[i] = br.literal(1) ? br.signed_literal(4) : 0;
    br.literal(1); // refresh_entropy_probs: nothing follows a key frame
    memcpy(F.prob, kVp8CoefProb, sizeof(F.prob));
    for (uint32_t i = 0; i < sizeof(F.prob); ++i)
        if (br.get(kVp8CoefUpdateProb[i])) { F.prob[i] = (uint8_t)br.literal(8); info.coef_prob_updates++; }
    F.use_skip = br.literal(1);
    if (F.use_skip) F.skip_p = br.literal(8);
    if (br.eof) return kVp8Parse;
    info.segmentation = F.use_segment; info.update_map = F.update_map;
    info.filter_simple = F.simple; info.filter_level = (uint32_t)F.level; info.sharpness = (uint32_t)F.sharpness;
    info.partitions = F.nparts;
    const int nseg = F.use_segment && F.update_map ? 4 : 1; // (without a map every macroblock is in segment 0)
    for (int s = 0; s < nseg; ++s) {
        bool newq = true, newf = true;
        for (int t = 0; t < s; ++t) { newq &= F.quant[t] != F.quant[s]; newf &= F.fstrength[t] != F.fstrength[s]; }
        info.segment_quantizers += newq; info.segment_filter_levels += newf;
    }
    return 0;
}

inline int seg_q(const Frame &F, int s) { return F.use_segment ? F.quant[s] : F.base_q; }

void dequant_steps(const Frame &F, int s, uint16_t *o)
{
    const int q = seg_q(F, s);
    o[0] = kVp8DcStep[clampi(q + F.dq[0], 0, 127)];
    o[1] = kVp8AcStep[clampi(q, 0, 127)];
    o[2] = (uint16_t)(kVp8DcStep[clampi(q + F.dq[1], 0, 127)] * 2u);
    const uint32_t y2ac = ((uint32_t)kVp8AcStep[clampi(q + F.dq[2], 0, 127)] * 101581u) >> 16;
    o[3] = (uint16_t)(y2ac < 8u ? 8u : y2ac);
    o[4] = kVp8DcStep[clampi(q + F.dq[3], 0, 117)];
    o[5] = kVp8AcStep[clampi(q + F.dq[4], 0, 127)];
    o[6] = o[7] = 0;
}

// filter parameters of a segment's macroblocks: limit (0 = not filtered), interior limit, hev threshold
void filter_strength(const Frame &F, int s, uint8_t *o)
{
    int level = F.use_segment ? F.fstrength[s] : F.level;
    level = clampi(level, 0, 63);
    o[0] = o[1] = o[2] = 0;
    if (F.level == 0 || level == 0) return; // (a frame at level 0 is not filtered at all, whatever its segments say)
    vp8_filter_strength(level, F.sharpness, o);
}

// the tokens of one block into lev[0 .. 16) (coding order, zeroed by the caller); returns the position behind the last non-zero level
int read_block(BoolDec &br, const uint8_t *tab, int type, int ctx, int n, int16_t *lev, uint32_t &cat6)
{
    const uint8_t *p = vp8_prob(tab, type, n, ctx);
    for (; n < 16; ++n) {
        if (!br.get(p[0])) return n;
        while (!br.get(p[1])) {
            p = vp8_prob(tab, type, ++n, 0);
            if (n == 16) return 16;
        }
        int v;
        if (!br.get(p[2])) { v = 1; p = vp8_prob(tab, type, n + 1, 1); }
        else {
            if (!br.get(p[3])) v = !br.get(p[4]) ? 2 : 3 + br.get(p[5]);
            else if (!br.get(p[6])) {
                if (!br.get(p[7])) v = 5 + br.get(159);
                else { v = 7 + 2 * br.get(165); v += br.get(145); }
            } else {
                const int b1 = br.get(p[8]), b0 = br.get(p[9 + b1]), cat = 2 + 2 * b1 + b0;
                v = 0;
                for (int k = 0; k < (int)kVp8CatBits[cat]; ++k) v += v + br.get(kVp8CatProb[cat][k]);
                v += (int)kVp8CatBase[cat];
                cat6 += cat == 5;
            }
            p = vp8_prob(tab, type, n + 1, 2);
        }
        lev[n] = (int16_t)(br.get(128) ? -v : v);
    }
    return 16;
}

inline int ctx_mode(int ymode) { return ymode == VP8_DC ? VP8_B_DC : ymode == VP8_V ? VP8_B_VE : ymode == VP8_H ? VP8_B_HE : VP8_B_TM; }

// Every macroblock: modes from the first partition, levels from the token partitions.  recs / levels == nullptr: count only.
int walk(Frame &F, Vp8Info &info, Vp8MbRecord *recs, int16_t *levels, size_t levels_cap, uint32_t *nlevels)
{
    uint8_t top_modes[kMaxMbw * 4u], top_nz[kMaxMbw][9];
    memset(top_modes, VP8_B_DC, (size_t)F.mbw * 4u);
    memset(top_nz, 0, (size_t)F.mbw * 9u);
    uint16_t dq[4][8];
    uint8_t fs[4][3];
    for (int s = 0; s < 4; ++s) { dequant_steps(F, s, dq[s]); filter_strength(F, s, fs[s]); }
    uint32_t nlev = 0;
    for (uint32_t mby = 0; mby < F.mbh; ++mby) {
        uint8_t left_modes[4] = {VP8_B_DC, VP8_B_DC, VP8_B_DC, VP8_B_DC}, left_nz[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        BoolDec &tb = F.part[mby & (F.nparts - 1u)];
        for (uint32_t mbx = 0; mbx < F.mbw; ++mbx) {
            BoolDec &br = F.br;
            Vp8MbRecord R;
            memset(&R, 0, sizeof(R));
            R.lev = nlev;
            if (F.update_map) R.segment = (uint8_t)(!br.get(F.segp[0]) ? br.get(F.segp[1]) : 2 + br.get(F.segp[2]));
            const int skip = F.use_skip ? br.get(F.skip_p) : 0;
            uint8_t *tm = top_modes + mbx * 4u;
            if (br.get(kVp8YModeProb[0])) {
                R.ymode = (uint8_t)(br.get(kVp8YModeProb[1]) ? (br.get(kVp8YModeProb[3]) ? VP8_TM : VP8_H) : (br.get(kVp8YModeProb[2]) ? VP8_V : VP8_DC));
                memset(tm, ctx_mode(R.ymode), 4);
                memset(left_modes, ctx_mode(R.ymode), 4);
                info.ymodes_mask |= 1u << R.ymode;
            } else {
                R.ymode = (uint8_t)kVp8BPred;
                for (int y = 0; y < 4; ++y) {
                    int m = left_modes[y];
                    for (int x = 0; x < 4; ++x) {
                        const uint8_t *p = kVp8BModeProb + ((size_t)tm[x] * 10u + (size_t)m) * 9u;
                        m = !br.get(p[0]) ? VP8_B_DC : !br.get(p[1]) ? VP8_B_TM : !br.get(p[2]) ? VP8_B_VE
                            : !br.get(p[3]) ? (!br.get(p[4]) ? VP8_B_HE : !br.get(p[5]) ? VP8_B_RD : VP8_B_VR)
                                            : (!br.get(p[6]) ? VP8_B_LD : !br.get(p[7]) ? VP8_B_VL : !br.get(p[8]) ? VP8_B_HD : VP8_B_HU);
                        tm[x] = (uint8_t)m;
                        const int b = 4 * y + x;
                        R.bmodes[b >> 1] |= (uint8_t)(m << (4 * (b & 1)));
                        info.bmodes_mask |= 1u << m;
                    }
                    left_modes[y] = (uint8_t)m;
                }
                info.bpred_macroblocks++;
            }
            R.uvmode = (uint8_t)(!br.get(kVp8UvModeProb[0]) ? VP8_DC : !br.get(kVp8UvModeProb[1]) ? VP8_V : br.get(kVp8UvModeProb[2]) ? VP8_TM : VP8_H);
            info.uvmodes_mask |= 1u << R.uvmode;
            if (br.eof) return kVp8Parse;
            // ---- tokens ----
            const bool i4 = R.ymode == kVp8BPred;
            uint8_t *tnz = top_nz[mbx];
            bool coded = false;
            if (!skip) {
                const uint16_t *q = dq[R.segment];
                int16_t lev[25][16];
                memset(lev, 0, sizeof(lev));
                int cnt[25];
                int first = 0, type = 3;
                bool dc_nz[16];
                for (int b = 0; b < 16; ++b) dc_nz[b] = false;
                cnt[24] = 0;
                if (!i4) {
                    const int nz = read_block(tb, F.prob, 1, tnz[8] + left_nz[8], 0, lev[24], info.cat6_tokens);
                    tnz[8] = left_nz[8] = nz > 0;
                    cnt[24] = nz;
                    first = 1; type = 0;
                    if (nz > 0) { // which luma blocks get a DC from the Y2 block: the filter's inner-edge rule needs to know
                        int in[16], dc[16];
                        for (int k = 0; k < 16; ++k) in[kVp8Zigzag[k]] = (int16_t)(lev[24][k] * (int)q[k ? 3 : 2]);
                        vp8_iwht(in, dc);
                        for (int b = 0; b < 16; ++b) dc_nz[b] = (int16_t)dc[b] != 0;
                    }
                }
                for (int b = 0; b < 16; ++b) {
                    const int x = b & 3, y = b >> 2;
                    const int nz = read_block(tb, F.prob, type, tnz[x] + left_nz[y], first, lev[b], info.cat6_tokens);
                    tnz[x] = left_nz[y] = nz > first;
                    cnt[b] = nz > first ? nz : 0;
                    coded |= nz > first || dc_nz[b];
                }
                for (int b = 16; b < 24; ++b) {
                    const int x = 4 + ((b - 16) >> 2) * 2 + (b & 1), y = 4 + ((b - 16) >> 2) * 2 + ((b >> 1) & 1);
                    const int nz = read_block(tb, F.prob, 2, tnz[x] + left_nz[y], 0, lev[b], info.cat6_tokens);
                    tnz[x] = left_nz[y] = nz > 0;
                    cnt[b] = nz;
                    coded |= nz > 0;
                }
                if (tb.eof) return kVp8Parse;
                for (int b = 0; b < 25; ++b) {
                    R.cnt[b] = (uint8_t)cnt[b];
                    if (levels) {
                        if (levels_cap - nlev < (size_t)cnt[b]) return kVp8Small;
                        memcpy(levels + nlev, lev[b], (size_t)cnt[b] * sizeof(int16_t));
                    }
                    nlev += (uint32_t)cnt[b];
                }
            } else {
                memset(tnz, 0, 8); memset(left_nz, 0, 8);
                if (!i4) tnz[8] = left_nz[8] = 0;
                info.skipped_macroblocks++;
                info.skipped_bpred_macroblocks += i4;
            }
            R.inner = i4 || coded;
            R.f_limit = fs[R.segment][0]; R.f_ilevel = fs[R.segment][1]; R.hev_thresh = fs[R.segment][2];
            if (recs) recs[(size_t)mby * F.mbw + mbx] = R;
        }
    }
    info.macroblocks = F.mbw * F.mbh;
    *nlevels = nlev;
    return 0;
}

size_t blob_fixed_bytes(const Vp8Info &info)
{
    const size_t mbs = (size_t)((info.width + 15u) >> 4) * ((info.height + 15u) >> 4);
    return sizeof(Vp8BlobHeader) + mbs * sizeof(Vp8MbRecord);
}

} // namespace

size_t vp8_blob_capacity(const Vp8Info &info)
{
    const size_t mbs = (size_t)((info.width + 15u) >> 4) * ((info.height + 15u) >> 4);
    const size_t alpha = !info.alph_len ? 0u : info.alpha_compression ? webp_alpha_blob_capacity(info.width, info.height, info.alph_len) : align16((size_t)info.width * info.height);
    return blob_fixed_bytes(info) + align16(mbs * kVp8MbLevels * sizeof(int16_t)) + align16(alpha) + 64u;
}

int vp8_parse_info(const uint8_t *d, size_t n, Vp8Info &info, bool deep)
{
    info = Vp8Info{};
    if (!d || n < 20 || memcmp(d, "RIFF", 4) || memcmp(d + 8, "WEBP", 4)) return kVp8Parse;
    if ((uint64_t)le32(d + 4) + 8u != n || (n & 1u)) return kVp8Parse; // the RIFF size is the file's
    size_t pos = 12, alph_off = 0, alph_len = 0;
    bool first = true, have_image = false;
    uint32_t canvas_w = 0, canvas_h = 0;
    while (pos < n) { // the walk of fl_webpsrc.cpp, with the chunks a lossy picture consists of
        if (n - pos < 8) return kVp8Parse;
        const uint8_t *tag = d + pos;
        const uint32_t len = le32(d + pos + 4);
        if (len > n - pos - 8) return kVp8Parse;
        if ((len & 1u) && (size_t)len + 1u > n - pos - 8) return kVp8Parse; // the padding byte of an odd chunk
        const uint8_t *p = d + pos + 8;
        if (first && !memcmp(tag, "VP8X", 4)) {
            if (len < 10) return kVp8Parse;
            info.extended = 1;
            info.has_alpha = (p[0] >> 4) & 1u;
            info.animated = (p[0] >> 1) & 1u;
            canvas_w = 1u + le24(p + 4);
            canvas_h = 1u + le24(p + 7);
        } else if (!memcmp(tag, "ANIM", 4) || !memcmp(tag, "ANMF", 4)) {
            if (!info.extended) return kVp8Parse;
            info.animated = 1;
        } else if (!memcmp(tag, "VP8 ", 4)) {
            if (!first && !info.extended) return kVp8Parse;
            if (!have_image) { have_image = true; info.vp8_off = pos + 8; info.vp8_len = len; }
        } else if (!memcmp(tag, "VP8L", 4)) {
            if (!first && !info.extended) return kVp8Parse;
            if (!have_image) return kVp8Parse; // a lossless picture: not this decoder's file
        } else if (!memcmp(tag, "ALPH", 4)) {
            if (info.extended && !have_image && !alph_len) { alph_off = pos + 8; alph_len = len; }
        } else if (!memcmp(tag, "EXIF", 4)) {
            if (info.extended && !info.exif_len) { info.exif_off = pos + 8; info.exif_len = len; }
        } else if (first) return kVp8Parse; // a file starts with VP8, VP8L or VP8X
        first = false;
        pos += 8u + (size_t)len + (len & 1u);
    }
    if (info.animated) { info.width = canvas_w; info.height = canvas_h; info.refused = "animation"; return 0; }
    if (!have_image) return kVp8Parse;
    Frame F;
    if (int rc = parse_frame(d + info.vp8_off, info.vp8_len, F, info)) return rc;
    if (info.extended && (canvas_w != info.width || canvas_h != info.height)) return kVp8Parse;
    if (info.has_alpha && alph_len) {
        if (alph_len < 1) return kVp8Parse;
        const uint32_t b = d[alph_off];
        info.alpha_compression = b & 3u; info.alpha_filter = (b >> 2) & 3u;
        // what libwebp takes: raw or lossless-coded, pre-processing 0 or 1 (nothing for a decoder to do), the reserved field 0 or 1
        if (info.alpha_compression > 1u || ((b >> 4) & 3u) > 1u || (b >> 6) > 1u) return kVp8Parse;
        info.alph_off = alph_off; info.alph_len = alph_len;
        if (!info.alpha_compression && alph_len - 1u < (uint64_t)info.width * info.height) return kVp8Parse; // a raw plane shorter than the picture
    }
    if ((uint64_t)info.width * info.height * 4u >= kVp8MaxDecoded) info.refused = "a decoded picture of 2^31 bytes and more";
    if (info.refused) return 0;
    info.channels = info.has_alpha ? 4u : 3u;
    info.supported = 1;
    if (!deep) return 0;
    uint32_t nlev = 0;
    if (int rc = walk(F, info, nullptr, nullptr, 0, &nlev)) return rc;
    size_t alpha = info.alph_len ? align16((size_t)info.width * info.height) : 0u;
    if (info.alph_len && info.alpha_compression) {
        uint32_t bytes = 0;
        if (int rc = webp_alpha_blob_bytes(d + info.alph_off + 1u, info.alph_len - 1u, info.width, info.height, &bytes)) return rc; // (the same codes)
        alpha = align16(bytes);
    }
    info.blob_bytes = (uint32_t)(blob_fixed_bytes(info) + align16((size_t)nlev * sizeof(int16_t)) + alpha);
    return 0;
}

int vp8_decode_levels(const uint8_t *d, size_t n, uint8_t *blob, size_t cap, Vp8BlobHeader *hdr)
{
    Vp8Info info;
    if (int rc = vp8_parse_info(d, n, info, false)) return rc;
    if (!info.supported) return kVp8Unsupported;
    if (!blob || (reinterpret_cast<uintptr_t>(blob) & 15u) || cap < blob_fixed_bytes(info) + 64u) return kVp8Small;
    Frame F;
    Vp8Info scratch;
    if (int rc = parse_frame(d + info.vp8_off, info.vp8_len, F, scratch)) return rc;
    Vp8BlobHeader H;
    memset(&H, 0, sizeof(H));
    H.magic = kVp8BlobMagic;
    H.width = info.width; H.height = info.height; H.channels = info.channels;
    H.mbw = F.mbw; H.mbh = F.mbh;
    H.filter_type = F.level == 0 ? 0u : F.simple ? 1u : 2u;
    for (int s = 0; s < 4; ++s) dequant_steps(F, s, H.dq[s]);
    H.rec_off = sizeof(Vp8BlobHeader);
    H.lev_off = (uint32_t)blob_fixed_bytes(info);
    // behind the levels: the raw plane, or the lossless decoder's blob with its work area (fl_webpsrc.h)
    const bool coded = info.alph_len && info.alpha_compression;
    size_t alpha_bytes = !info.alph_len ? 0u : coded ? align16(webp_alpha_blob_capacity(info.width, info.height, info.alph_len)) : align16((size_t)info.width * info.height);
    if (cap - H.lev_off < alpha_bytes) return kVp8Small;
    const size_t lev_cap = ((cap - H.lev_off - alpha_bytes) & ~(size_t)15u) / sizeof(int16_t);
    uint32_t nlev = 0;
    if (int rc = walk(F, scratch, reinterpret_cast<Vp8MbRecord *>(blob + H.rec_off), reinterpret_cast<int16_t *>(blob + H.lev_off), lev_cap, &nlev)) return rc;
    H.nlevels = nlev;
    const size_t lev_bytes = align16((size_t)nlev * sizeof(int16_t));
    memset(blob + H.lev_off + (size_t)nlev * sizeof(int16_t), 0, lev_bytes - (size_t)nlev * sizeof(int16_t));
    H.alpha_off = (uint32_t)(H.lev_off + lev_bytes);
    if (coded) {
        WebpBlobHeader W;
        if (int rc = webp_decode_alpha_residuals(d + info.alph_off + 1u, info.alph_len - 1u, info.width, info.height, blob + H.alpha_off, cap - H.alpha_off, &W)) return rc; // (the same codes)
        H.alpha = 2; H.alpha_filter = info.alpha_filter;
        alpha_bytes = align16(W.total_bytes);
        memset(blob + H.alpha_off + W.total_bytes, 0, alpha_bytes - W.total_bytes);
    } else if (info.alph_len) {
        H.alpha = 1; H.alpha_filter = info.alpha_filter;
        const size_t px = (size_t)info.width * info.height;
        memcpy(blob + H.alpha_off, d + info.alph_off + 1u, px);
        memset(blob + H.alpha_off + px, 0, alpha_bytes - px);
    }
    H.total_bytes = (uint32_t)(H.alpha_off + alpha_bytes);
    memcpy(blob, &H, sizeof(H));
    if (hdr) *hdr = H;
    return 0;
}

} // namespace fl
