// fl_jpeg_dev.h -- the device code the JPEG encoder's translation units share: fl_jpeg.hip (jpeg_dct_quant_kernel, jpeg_pack_kernel),
// fl_jpeg_opt.hip (the kernels of FLGPU_FEO_JPEG_OPTIMIZE, which run the same transform, coder and packer with the picture's own
// tables) and fl_jpeg_420.hip (FLGPU_FEO_JPEG_420: its own transform and coder, this file's packer with another unit order).  The
// options are translation units of their own so that the module the two plain kernels are compiled in holds exactly what it held
// before the options existed: their instruction streams are pinned (profiles/pr_jpeg_optimize.txt, profiles/pr_jpeg_420.txt).
// fl_jpeg.hip describes the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fl_jpeg.h"
#include "fl_jpeg_tables.h"
#include "fl_pixel.h"
#include "fl_types.h"

namespace fl {

namespace {

// ---------------------------------------------------------------- constant tables --

// transform.rs constants (CONST_BITS = 13)
constexpr int32_t F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633, F_1_501 = 12299,
                  F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

struct Mat8 { int32_t a[8][8]; };

// The 1-D butterfly of transform.rs::fdct without its rounding constants and shifts: out[k] is linear in in[].
constexpr void fdct_linear(const int32_t in[8], int32_t out[8])
{
    int32_t t0 = in[0] + in[7], t1 = in[1] + in[6], t2 = in[2] + in[5], t3 = in[3] + in[4];
    const int32_t t10 = t0 + t3, t11 = t1 + t2;
    int32_t t12 = t0 - t3, t13 = t1 - t2;
    t0 = in[0] - in[7]; t1 = in[1] - in[6]; t2 = in[2] - in[5]; t3 = in[3] - in[4];
    out[0] = t10 + t11;
    out[4] = t10 - t11;
    int32_t z1 = (t12 + t13) * F_0_541;
    out[2] = z1 + t12 * F_0_765;
    out[6] = z1 - t13 * F_1_847;
    t12 = t0 + t2;
    t13 = t1 + t3;
    z1 = (t12 + t13) * F_1_175;
    t12 = t12 * (-F_0_390) + z1;
    t13 = t13 * (-F_1_961) + z1;
    z1 = (t0 + t3) * (-F_0_899);
    out[1] = t0 * F_1_501 + z1 + t12;
    out[7] = t3 * F_0_298 + z1 + t13;
    z1 = (t1 + t2) * (-F_2_562);
    out[3] = t1 * F_3_072 + z1 + t13;
    out[5] = t2 * F_2_053 + z1 + t12;
}

constexpr Mat8 make_fdct_matrix()
{
    Mat8 m{};
    for (int j = 0; j < 8; ++j) {
        int32_t e[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        e[j] = 1;
        fdct_linear(e, o);
        for (int k = 0; k < 8; ++k) m.a[k][j] = o[k];
    }
    return m;
}

__constant__ Mat8 kFdct = make_fdct_matrix();

constexpr bool fdct_matrix_fits_i16()
{
    const Mat8 m = make_fdct_matrix();
    for (int k = 0; k < 8; ++k)
        for (int j = 0; j < 8; ++j)
            if (m.a[k][j] > 32767 || m.a[k][j] < -32768) return false;
    return true;
}
static_assert(fdct_matrix_fits_i16(), "the passes use v_dot2_i32_i16: matrix entries must be 16-bit");

typedef short i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ i16x2 as_i16x2(uint32_t v) { return __builtin_bit_cast(i16x2, v); }
__device__ __forceinline__ uint32_t pack_i16(int32_t lo, int32_t hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }
// 8-term dot product of packed 16-bit operands, exact in 32 bits (v_dot2_i32_i16: two multiply-adds per instruction)
__device__ __forceinline__ int32_t dot8_i16(const uint32_t m[4], const uint4 v)
{
    int32_t p = __builtin_amdgcn_sdot2(as_i16x2(m[0]), as_i16x2(v.x), 0, false);
    p = __builtin_amdgcn_sdot2(as_i16x2(m[1]), as_i16x2(v.y), p, false);
    p = __builtin_amdgcn_sdot2(as_i16x2(m[2]), as_i16x2(v.z), p, false);
    return __builtin_amdgcn_sdot2(as_i16x2(m[3]), as_i16x2(v.w), p, false);
}

// zig-zag position -> natural index (encoder.rs UNZIGZAG): the transform gives lane k the sample and coefficient of natural
// index kNatural[k], so that its quantised result is zig-zag coefficient k without an exchange
struct NaturalOrder { uint8_t n[64]; };
constexpr NaturalOrder make_natural()
{
    NaturalOrder t{};
    for (int k = 0; k < 64; ++k) t.n[k] = kUnzigzag[k];
    return t;
}
__constant__ NaturalOrder kNatural = make_natural();

// Annex K Huffman tables (fl_jpeg_tables.h) expanded to (length << 16 | code) at compile time -- encoder.rs build_huff_lut
struct HuffLut { uint32_t e[256]; };

constexpr HuffLut make_lut(const HuffSpec &s)
{
    HuffLut t{};
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < s.len[l - 1]; ++i, ++k) t.e[s.val[k]] = ((uint32_t)l << 16) | code++;
        code <<= 1;
    }
    return t;
}

struct HuffAll { HuffLut ac[2], dc[2]; };
constexpr HuffAll make_all() { return HuffAll{{make_lut(kAcLuma), make_lut(kAcChroma)}, {make_lut(kDcLuma), make_lut(kDcChroma)}}; }
__constant__ HuffAll kHuff = make_all();

// ---------------------------------------------------------------- wave helpers --

template <int N>
__device__ __forceinline__ uint32_t dpp_row_shr(uint32_t v)
{
    // lane i receives lane i - N of its row of 16; lanes without a source get 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + N, 0xf, 0xf, false);
}

// Inclusive prefix sum over the 64 lanes in six DPP adds: four steps inside the rows of 16, then the row totals travel by
// row_bcast:15 (rows 1 and 3 take the last lane of the row before) and row_bcast:31 (rows 2 and 3 take lane 31).
// (VALU latency only; ds_bpermute based shuffles cost an LDS round trip per step, v_readlane + v_cndmask per row six more
// vector instructions -- this kernel runs at 97 % VALU issue, profiles/r03_jpeg_pmc.txt, so instructions are its time.)
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane)
{
    (void)lane;
    v += dpp_row_shr<1>(v);
    v += dpp_row_shr<2>(v);
    v += dpp_row_shr<4>(v);
    v += dpp_row_shr<8>(v);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15 row_mask:0xa
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast:31 row_mask:0xc
    return v;
}

// LDS traffic that stays inside one wave needs no hardware barrier (a wave's DS instructions execute in order);
// this only stops the compiler from moving accesses across the point.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

constexpr uint32_t kPackThreads = 512; // jpeg_pack_kernel: one workgroup per picture; its phases are chains of short dependent steps
constexpr uint32_t kPackWaves = kPackThreads / 64;

// exclusive scan across the threads of the pack workgroup; *total = sum.  s_w: kPackWaves words of LDS.
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t *s_w, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_scan(v, lane);
    __syncthreads(); // s_w may still be read from the previous call
    if (lane == 63u) s_w[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPackWaves; ++i) { const uint32_t t = s_w[i]; if (i < wave) base += t; sum += t; }
    *total = sum;
    return base + inc - v;
}

__device__ __forceinline__ uint32_t coef_size(int32_t v) // encode_coefficient: bits of |v|
{
    const uint32_t mag = (uint32_t)(v < 0 ? -v : v);
    return mag ? 32u - (uint32_t)__clz(mag) : 0u;
}

// ---------------------------------------------------------------- kernel 1: colour + FDCT + quantise + AC Huffman coding --

// Blocks per wave: 16 (lanes 16 k + b code component k of block b) or 32 (lanes b / 32 + b: block b's Y / Cb + Cr units).
// 32 uses every lane in the coding phase but needs 13.5 KB of LDS per wave (2.5 waves per SIMD); 16 needs half of that and took
// 307 us against 394 us per 1024 pictures (profiles/pr_jpeg_unit_coder.txt).  `make EXTRA="-DFL_JPEG_BPW=32 ..."` for the A/B.
#ifndef FL_JPEG_BPW
#define FL_JPEG_BPW 16
#define FL_JPEG_WPG 2
#define FL_JPEG_PREFETCH 3
#endif
constexpr uint32_t kBlocksPerWave = FL_JPEG_BPW;
constexpr uint32_t kWavesPerWg = FL_JPEG_WPG;
constexpr uint32_t kPrefetch = FL_JPEG_PREFETCH;       // blocks whose pixels are loaded ahead
static_assert(kBlocksPerWave == 32u || kBlocksPerWave == 16u, "the coding phase's lane mapping");
constexpr uint32_t kJpegThreads = 64u * kWavesPerWg;
constexpr uint32_t kBlocksPerWg = kWavesPerWg * kBlocksPerWave;
constexpr uint32_t kUnitsPerWave = 3u * kBlocksPerWave;

// The longest AC code of a unit: 63 non-zero coefficients, each a (run, size) code of at most 16 bits and at most 10 value bits
// (|AC| <= 1023 for 8-bit samples), no end-of-block code behind coefficient 63.  Fewer coefficients are shorter: a ZRL (10-11
// bits) stands for 16 zero positions and an end-of-block code (2-4 bits) only follows a zero coefficient 63.
static_assert(63u * (16u + 10u) <= kAcWordsPerUnit * 32u, "a unit's AC code must fit its acbits slot");

// Per wave: the quantised coefficients of kBlocksPerWave blocks (zig-zag order, DC first) and their non-zero AC masks, written
// by the transform phase and read by the coding phase; the transform's two exchange buffers for the three components.
struct WaveLds {
    int16_t coef[kUnitsPerWave][64];
    uint64_t nz[kUnitsPerWave];                          // bit k: zig-zag coefficient k (k >= 1) is not zero
    __attribute__((aligned(16))) int16_t smp[3][64];     // samples, natural order
    __attribute__((aligned(16))) int16_t p1[3][64];      // pass-1 results, transposed
};

// own: the picture's tables, as jpeg_opt_tables_kernel left them (kJpegOptAcLut); nullptr: Annex K's
__device__ __forceinline__ void stage_ac_luts(uint32_t *s_ac, const uint32_t *own = nullptr)
{
    if (own) for (uint32_t i = threadIdx.x; i < 512u; i += kJpegThreads) s_ac[i] = own[i];
    else for (uint32_t i = threadIdx.x; i < 512u; i += kJpegThreads) s_ac[i] = kHuff.ac[i >> 8].e[i & 255u];
    __syncthreads();
}

// kRgba: every letterboxed picture, 4 channels at a 4-byte aligned address: one dword per pixel and no branch, so that the loads
// of the blocks ahead stay in flight (behind the channel-count branches of load_rgba the compiler waits for every load at once)
template <bool kRgba>
__device__ __forceinline__ uint32_t block_pixel(const JpegJob &jb, uint32_t brow, uint32_t bcol, uint32_t r, uint32_t c)
{
    // copy_blocks_ycbcr / pixel_at_or_near: pixels past the right / bottom edge repeat the last column / row
    uint32_t px = bcol * 8u + c, py = brow * 8u + r;
    px = px < jb.w ? px : jb.w - 1u;
    py = py < jb.h ? py : jb.h - 1u;
    // (a global, not a flat, load: a flat load also counts against the LDS waits, so each of them would wait for the pixels too;
    // the caller drops the alpha byte when it takes the value, which keeps the load in flight until then)
    if constexpr (kRgba) return ((const __attribute__((address_space(1))) uint32_t *)jb.src)[(size_t)py * jb.w + px];
    uint32_t pr, pg, pb, pa;
    load_rgba(jb.src + ((size_t)py * jb.w + px) * jb.c, jb.c, pr, pg, pb, pa);
    return pr | (pg << 8) | (pb << 16);
}

// Forward DCT + quantisation of the three components of one block, interleaved so that the LDS round trips of one component
// overlap the arithmetic of the others.  Lane k holds the sample at natural index (r, c) = kNatural[k] and returns the
// quantised coefficient of that index, i.e. zig-zag coefficient k.
__device__ __forceinline__ void dct_quant_block(const uint32_t (&smp)[3], uint32_t nat, uint32_t r, uint32_t c, const uint32_t (&m1)[4],
                                                const uint32_t (&m2)[4], uint4 k1, const uint32_t (&q)[3], const uint32_t (&magic)[3],
                                                WaveLds &w, int32_t (&qv)[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) w.smp[k][nat] = (int16_t)smp[k];
    wave_lds_sync();
    // Pass 1 (rows): lane (r, c) produces horizontal frequency c of row r
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int32_t p = dot8_i16(m1, *reinterpret_cast<const uint4 *>(w.smp[k] + r * 8)); // one 16-byte read: the row's 8 samples
        // transform.rs: c = 0: (p - 8 * 128) << PASS1_BITS (level shift folded in), c = 4: p << PASS1_BITS, else (p + 2^10) >> 11
        // (CONST_BITS - PASS1_BITS).  One form for all lanes, (p << s1 + a1) >> 11 with per-lane s1 = 13 or 0 (the sums of columns 0
        // and 4 are below 2^12, so nothing is shifted out): no lane-dependent branches.
        const int32_t v1 = ((p << k1.x) + (int32_t)k1.y) >> 11;
        w.p1[k][c * 8 + r] = (int16_t)v1;                 // |v1| <= 255 * 8 * 4; transposed: the column pass reads 8 consecutive values
    }
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // Pass 2 (columns): lane (r, c) produces vertical frequency r of column c: rows 0 and 4 (p2 + 2) >> 2, else (p2 + 2^14) >> 15
        const int32_t p2 = dot8_i16(m2, *reinterpret_cast<const uint4 *>(w.p1[k] + c * 8));
        const int32_t d = (p2 + (int32_t)k1.z) >> k1.w;
        // encode_rgb "Quantization": ((d / 8) as f32 / f32::from(q)).round() as i32.  |d / 8| <= 2048 and q <= 255,
        // so the f32 quotient cannot round onto or across a half (nearest miss: 1 / (2q) >= 2^-9 away, f32 error
        // <= 2^-14): it equals the exact round-half-away  sign(n) * floor((2|n| + q) / 2q), taken with the
        // per-coefficient reciprocal ceil(2^32 / 2q) from the table block (exact for 2|n| + q < 2^13).
        // i32 division truncates toward zero: |d / 8| = |d| >> 3, and the sign of a non-zero quotient is d's.
        const int32_t sg = d >> 31;
        const uint32_t an = (uint32_t)((d ^ sg) - sg) >> 3;
        const uint32_t rq = __umulhi(2u * an + q[k], magic[k]);
        qv[k] = ((int32_t)rq ^ sg) - sg;
    }
}

typedef __attribute__((address_space(1))) uint32_t global_u32; // (global, not flat, stores: they do not count against the LDS waits)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));     // a JpegUnit as one 16-byte access: x = meta, y z w = ac[0..2]
typedef __attribute__((address_space(1))) u32x4 global_u32x4;
static_assert(sizeof(JpegUnit) == sizeof(u32x4) && kUnitAcWords == 3u, "a unit's record is one 16-byte access");

// Appends the `len` (<= 26) low bits of `code` to a lane's unit, most significant bit first: the first kUnitAcWords full 32-bit
// words stay in registers (they go out with the unit's record), the later ones go to out[wi], the unit's acbits slot.
struct UnitBits {
    uint64_t acc;   // the low `pend` bits are pending (pend < 32 between calls)
    uint32_t pend, total, wi;
    global_u32 *out;
    uint32_t w0, w1, w2;
    __device__ __forceinline__ void word(uint32_t v)
    {
        w0 = wi == 0u ? v : w0;
        w1 = wi == 1u ? v : w1;
        w2 = wi == 2u ? v : w2;
        if (wi >= kUnitAcWords) out[wi] = v;
        ++wi;
    }
    __device__ __forceinline__ void put(uint32_t code, uint32_t len)
    {
        acc = (acc << len) | code;
        pend += len;
        total += len;
        if (pend >= 32u) { pend -= 32u; word((uint32_t)(acc >> pend)); }
    }
};

// The transform phase of jpeg_dct_quant_kernel: blocks first .. first + count - 1 into the wave's LDS.
template <bool kRgba>
__device__ __forceinline__ void transform_blocks(const JpegJob &jb, const uint32_t *__restrict__ arena, uint32_t first, uint32_t count,
                                                 uint32_t lane, WaveLds &w)
{
    const uint32_t nat = kNatural.n[lane], r = nat >> 3, c = nat & 7u;
    uint32_t m1[4], m2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m1[j] = pack_i16(kFdct.a[c][2 * j], kFdct.a[c][2 * j + 1]);
        m2[j] = pack_i16(kFdct.a[r][2 * j], kFdct.a[r][2 * j + 1]);
    }
    const uint8_t *qt = reinterpret_cast<const uint8_t *>(arena + jb.tab_off) + 624;
    const uint32_t *mg = reinterpret_cast<const uint32_t *>(qt + 128);
    const uint32_t q[3] = {qt[nat], qt[64 + nat], qt[64 + nat]};
    const uint32_t magic[3] = {mg[nat], mg[64 + nat], mg[64 + nat]};
    // per-lane shift / rounding constants of the two passes (see dct_quant_block)
    const uint4 k1 = {(c == 0u || c == 4u) ? 13u : 0u, c == 0u ? (uint32_t)(-(8 * 128) * 8192) : (c == 4u ? 0u : 1u << 10),
                      (r == 0u || r == 4u) ? 2u : 1u << 14, (r == 0u || r == 4u) ? 2u : 15u};
    uint32_t brow = first / jb.bx, bcol = first - brow * jb.bx; // (one division per wave; the walk below steps them)
    // the pixels of the next kPrefetch blocks are in flight while a block is transformed (block_pixel clamps to the picture,
    // so the loads past the wave's last block need no condition -- a condition would make the compiler wait for all of them)
    uint32_t ahead[kPrefetch];
#pragma unroll
    for (uint32_t j = 0; j < kPrefetch; ++j) {
        ahead[j] = block_pixel<kRgba>(jb, brow, bcol, r, c);
        if (++bcol == jb.bx) { bcol = 0; ++brow; }
    }
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t rgb = kRgba ? ahead[0] & 0xffffffu : ahead[0];
#pragma unroll
        for (uint32_t j = 0; j + 1u < kPrefetch; ++j) ahead[j] = ahead[j + 1u];
        ahead[kPrefetch - 1u] = block_pixel<kRgba>(jb, brow, bcol, r, c);
        if (++bcol == jb.bx) { bcol = 0; ++brow; }
        uint32_t smp[3];
        jfif_px(rgb, smp[0], smp[1], smp[2]);
        // a block of one colour (the fill frame of a letterboxed picture: 75 of the 950 blocks of config 1, 31 % of config 0's)
        const bool flat = __ballot(rgb != (uint32_t)__builtin_amdgcn_readfirstlane((int)rgb)) == 0ull;
        if (flat) {
            // Both passes of the transform are linear up to their final shifts and every row of the matrix but the first sums to zero:
            // a constant block s has pass-1 column 0 = 4 (8 s - 1024) in every row, nothing else, and pass 2 turns that into
            // d[0] = (32 (8 s - 1024) + 2) >> 2 = 64 (s - 128); all other d are (0 + rounding) >> shift = 0.  The DC term goes through
            // the quantiser of dct_quant_block (lane 0 holds natural index 0), the AC masks are empty.
            if (lane == 0u) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int32_t d = 64 * ((int32_t)smp[k] - 128);
                    const int32_t sg = d >> 31;
                    const uint32_t an = (uint32_t)((d ^ sg) - sg) >> 3;
                    const uint32_t rq = __umulhi(2u * an + q[k], magic[k]);
                    w.coef[i * 3u + k][0] = (int16_t)(((int32_t)rq ^ sg) - sg);
                    w.nz[i * 3u + k] = 0ull;
                }
            }
            continue;
        }
        int32_t qv[3];
        dct_quant_block(smp, nat, r, c, m1, m2, k1, q, magic, w, qv);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            w.coef[i * 3u + k][lane] = (int16_t)qv[k];
            const uint64_t nz = __ballot(qv[k] != 0) & ~1ull;
            if (lane == 0u) w.nz[i * 3u + k] = nz;
        }
    }
}

// Two phases per wave.  Transform: one block after the other, the 64 lanes are the 64 samples / coefficients of a block
// (dct_quant_block); each unit's quantised coefficients go to LDS in zig-zag order, with a ballot of their non-zero AC terms.
// A block of one colour skips the transform.  Coding: every lane codes whole units by itself (BitWriter::write_block without
// the DC term) -- lane 16 k + b component k of block b (see kBlocksPerWave) -- walking the set bits of the
// unit's mask: one code word per step, however many coefficients its neighbours' units hold.  Out: the unit's record (quantised
// DC, AC bit count, AC bits from bit 0, the last word padded with zeros); AC words 3 and up go to the unit's acbits slot.
// kOwn (jpeg_opt_code_kernel, FLGPU_FEO_JPEG_OPTIMIZE): the AC code tables are the picture's own, from its record in `opt`.
template <bool kOwn>
__device__ __forceinline__ void jpeg_code_units(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena, uint32_t job_base,
                                                const uint32_t *__restrict__ opt)
{
    __shared__ WaveLds s_w[kWavesPerWg];
    __shared__ uint32_t s_ac[512];                       // AC code tables (luma, chroma)
    const JpegJob jb = jobs[job_base + blockIdx.y];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t nblocks = jb.bx * jb.by;
    if (blockIdx.x * kBlocksPerWg >= nblocks) return;    // whole workgroup idle (uniform)
    if constexpr (kOwn) stage_ac_luts(s_ac, opt + jb.opt_off + kJpegOptAcLut);
    else stage_ac_luts(s_ac);
    const uint32_t first = blockIdx.x * kBlocksPerWg + wave * kBlocksPerWave;
    if (first >= nblocks) return;                        // wave-uniform; from here on waves never synchronise with each other
    const uint32_t count = min(kBlocksPerWave, nblocks - first);
    WaveLds &w = s_w[wave];

    // ---- transform phase ----
    if (jb.c == 4u && (reinterpret_cast<uintptr_t>(jb.src) & 3u) == 0u) transform_blocks<true>(jb, arena, first, count, lane, w);
    else transform_blocks<false>(jb, arena, first, count, lane, w);
    wave_lds_sync();

    // ---- coding phase: one lane per unit ----
    uint32_t b, u, u_end;
    bool chroma;
    if constexpr (kBlocksPerWave == 32u) { // lane b: block b's Y unit; lane 32 + b: its Cb, then its Cr unit
        b = lane & 31u;
        chroma = lane >= 32u;
        u = b * 3u + (chroma ? 1u : 0u);
        u_end = b * 3u + (chroma ? 3u : 1u);
    } else {                               // lane 16 k + b: component k of block b (lanes 48-63 idle)
        b = lane & 15u;
        chroma = lane >= 16u;
        u = b * 3u + (lane >> 4);
        u_end = lane >= 48u ? u : u + 1u;
    }
    if (b >= count) return;
    const uint32_t *tab = s_ac + (chroma ? 256u : 0u);
    const uint32_t eob = tab[0], zrl = tab[0xF0];
    for (; u < u_end; ++u) {
        const uint32_t unit = first * 3u + u;
        const int16_t *cf = w.coef[u];
        uint64_t m = w.nz[u];
        UnitBits ub{0ull, 0u, 0u, 0u, (global_u32 *)jb.acbits + (size_t)unit * kAcWordsPerUnit, 0u, 0u, 0u};
        uint32_t prev = 0;
        // the next coefficient is read one step ahead, so that a step waits for one LDS round trip (the table entry), not two
        uint32_t pos = (uint32_t)__builtin_ctzll(m | (1ull << 63));
        int32_t v = cf[pos];
        while (m) {
            const uint32_t cpos = pos;
            const int32_t cv = v;
            m &= m - 1ull;
            pos = (uint32_t)__builtin_ctzll(m | (1ull << 63));
            v = cf[pos];
            uint32_t run = cpos - prev - 1u;
            prev = cpos;
            while (run > 15u) { ub.put(zrl & 0xffffu, zrl >> 16); run -= 16u; } // "while zero_run > 15 { huffman_encode(0xF0) }"
            const uint32_t mag = (uint32_t)(cv < 0 ? -cv : cv);
            const uint32_t size = 32u - (uint32_t)__clz(mag);                 // encode_coefficient (cv is not zero)
            const uint32_t value = (uint32_t)(cv + (cv >> 31)) & ((1u << size) - 1u); // negative: (v - 1) & mask
            const uint32_t e = tab[(run << 4) | size];
            ub.put(((e & 0xffffu) << size) | value, (e >> 16) + size);          // <= 16 + 10 bits
        }
        if (prev != 63u) ub.put(eob & 0xffffu, eob >> 16);
        if (ub.pend) ub.word((uint32_t)(ub.acc << (32u - ub.pend)));                    // the last word, padded with zeros
        // the unit's record in one 16-byte store, behind the loop where the wave's lanes have met again: the records of a wave's
        // 48 units are 768 consecutive bytes
        const u32x4 rec = {((uint32_t)(uint16_t)cf[0]) | (ub.total << 16), ub.w0, ub.w1, ub.w2}; // quantised DC, AC bit count
        ((global_u32x4 *)jb.units)[unit] = rec;
    }
}

// ---------------------------------------------------------------- kernel 2: offsets, assembly, stuffing, framing --

constexpr uint32_t kDcCodes = 12; // DC size categories 0..11 (the difference of two quantised DC terms of 8-bit samples)

constexpr uint32_t kWinWords = 8192; // LDS window of the bit stream: 32 KB = 262,144 bits

// ORs the 32-bit word `val`, whose most significant bit sits at stream bit g, into the window [wbase, wbase + kWinWords)
__device__ __forceinline__ void win_or(uint32_t *win, uint32_t wbase, uint64_t g, uint32_t val)
{
    const uint64_t W = g >> 5;
    const uint32_t sh = (uint32_t)g & 31u;
    const uint32_t hi = val >> sh, lo = sh ? val << (32u - sh) : 0u;
    if (hi && W >= wbase && W < (uint64_t)wbase + kWinWords) atomicOr(&win[W - wbase], hi);
    if (lo && W + 1 >= wbase && W + 1 < (uint64_t)wbase + kWinWords) atomicOr(&win[W + 1 - wbase], lo);
}

// The scan's unit order.  k420 = false: three units per block, Y Cb Cr, each after the same component's unit of the block before (u - 3).
// k420 (FLGPU_FEO_JPEG_420, fl_jpeg_420.hip): six per 16 x 16 MCU, Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr; Y(0,0) follows the MCU before's
// Y(1,1) (u - 3), the other Y units the one before (u - 1), Cb and Cr their own of the MCU before (u - 6).  In both orders a unit
// with fewer than unit_dc_back units in front of it is its component's first: its predecessor's DC term is 0.
template <bool k420> __device__ __forceinline__ bool unit_is_chroma(uint32_t u) { return k420 ? (u % 6u) >= 4u : (u % 3u) != 0u; }
template <bool k420> __device__ __forceinline__ uint32_t unit_dc_back(uint32_t u)
{
    if constexpr (!k420) return 3u;
    const uint32_t slot = u % 6u;
    return slot == 0u ? 3u : slot < 4u ? 1u : 6u;
}

// s_dc: the two DC code tables (luma, chroma), kDcCodes entries each, staged in LDS -- a table entry is then an LDS read behind
// the unit's record, not a third dependent global load
template <bool k420 = false>
__device__ __forceinline__ uint32_t dc_code(const uint32_t *s_dc, uint32_t u, uint32_t meta, uint32_t prev_meta, uint32_t *len)
{
    // differential DC against the same component's previous block (encode_rgb: y_dcprev / cb_dcprev / cr_dcprev); prev_meta is
    // the meta word of unit u - unit_dc_back(u), or 0 for a picture's first block
    const int32_t dc = (int16_t)(meta & 0xffffu), prev = (int16_t)(prev_meta & 0xffffu);
    const int32_t diff = dc - prev;
    const uint32_t size = coef_size(diff);
    const uint32_t value = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << size) - 1u);
    const uint32_t e = s_dc[(unit_is_chroma<k420>(u) ? kDcCodes : 0u) + size];
    *len = (e >> 16) + size;                                   // <= 9 + 11 or 11 + 11 bits
    return (((e & 0xffffu) << size) | value) << (32u - *len);  // left-aligned
}

// What the pack kernel reads per unit: its record and the meta word of the same component's previous block, requested together.
// The loads carry no condition (a unit index past the end reads the last unit, a first block's predecessor reads unit 0): behind
// a branch the compiler cannot count the loads in flight and waits for all of them, the ones just requested included.  What
// such a load returned is dropped when the value is taken (take_pack_unit).
struct PackUnit { u32x4 rec; uint32_t prev; };
template <bool k420 = false>
__device__ __forceinline__ PackUnit load_pack_unit(const JpegJob &jb, uint32_t u, uint32_t u_end)
{
    const global_u32x4 *recs = (const global_u32x4 *)jb.units;
    const uint32_t uc = min(u, u_end - 1u);                    // (u_end >= 3: a picture has at least one block)
    PackUnit p;
    p.rec = recs[uc];
    const uint32_t back = unit_dc_back<k420>(uc);              // (clamped, never wrapped: a first unit reads unit 0)
    p.prev = ((const global_u32 *)(recs + (max(uc, back) - back)))[0];
    return p;
}
template <bool k420 = false>
__device__ __forceinline__ PackUnit take_pack_unit(PackUnit p, uint32_t u, uint32_t u_end)
{
    if (u >= u_end) p.rec = u32x4{0u, 0u, 0u, 0u};             // no unit: no bits
    if (u < unit_dc_back<k420>(u) || u >= u_end) p.prev = 0u;
    return p;
}

// Rounds of the first pass whose records are requested ahead of the round that uses them.  One round ahead took 32.4 us per
// 1024 pictures of 300 x 200, all six rounds of such a picture (2,850 units) 35.6 us: 73 registers instead of 58 leave room for
// three workgroups per CU, not four (profiles/pr_jpeg_unit_records.txt).  `make EXTRA=-DFL_JPEG_PACK_DEPTH=6` for the A/B.
#ifndef FL_JPEG_PACK_DEPTH
#define FL_JPEG_PACK_DEPTH 1
#endif
constexpr uint32_t kPackDepth = FL_JPEG_PACK_DEPTH;

// A kernel template, not a kernel around a shared body: inlined into a wrapper, the compiler orders the operands of three additions
// differently from the kernel this was before the option existed; as a template, <false> is that kernel instruction for instruction.
// kOwn (jpeg_pack_kernel<true>, FLGPU_FEO_JPEG_OPTIMIZE; `opt` is unused without it): the DC code tables, the header and its length are the picture's own, from its
// record in `opt` (where the decision fell against them the record holds Annex K's, and the file is jpeg_pack_kernel's byte for byte).
// k420 (fl_jpeg_420.hip): the unit order of FLGPU_FEO_JPEG_420 -- which code table a unit takes and where its DC predecessor sits; bx, by count MCUs.
template <bool kOwn, bool k420 = false>
__global__ __launch_bounds__(kPackThreads) void jpeg_pack_kernel(const JpegJob *__restrict__ jobs, const uint32_t *__restrict__ arena,
                                                                 uint32_t job_base, const uint32_t *__restrict__ opt)
{
    __shared__ uint32_t s_win[kWinWords];
    __shared__ uint32_t s_w[kPackWaves], s_carry, s_lo, s_hi, s_dc[2u * kDcCodes];
    const JpegJob jb = jobs[job_base + blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint32_t nunits = jb.bx * jb.by * (k420 ? 6u : 3u);
    constexpr uint32_t T = kPackThreads;

    // ---- bit offset of every block: DC code size (needs the previous block) + AC size, exclusive scan -- and, in the same pass,
    // the block's code goes into the first window of the stream (win_or drops what lies beyond it): a unit's record holds its
    // meta word and the AC words nearly every unit ends with, so a picture whose stream fits one window (every 300 x 200 picture)
    // costs one load per unit, and that load is requested a round ahead ----
    // the records of the first kPackDepth rounds are on their way while the window is cleared
    PackUnit ahead[kPackDepth];
#pragma unroll
    for (uint32_t j = 0; j < kPackDepth; ++j) ahead[j] = load_pack_unit<k420>(jb, j * T + tid, nunits);
    for (uint32_t i = tid; i < kWinWords; i += T) s_win[i] = 0u;
    const uint32_t *own = kOwn ? opt + jb.opt_off : nullptr;
    if constexpr (kOwn) { if (tid < 2u * kDcCodes) s_dc[tid] = own[kJpegOptDcLut + tid]; }
    else if (tid < 2u * kDcCodes) s_dc[tid] = kHuff.dc[tid / kDcCodes].e[tid % kDcCodes];
    if (tid == 0u) s_carry = 0u;
    __syncthreads();
    for (uint32_t base0 = 0; base0 < nunits; base0 += kPackDepth * T) {
#pragma unroll
        for (uint32_t j = 0; j < kPackDepth; ++j) {
            const uint32_t base = base0 + j * T;
            if (base >= nunits) break;                   // (uniform)
            const uint32_t u = base + tid;
            // round r + kPackDepth's records are requested before round r's scan: a round waits for a load that is already
            // under way, not for a fresh round trip behind the two barriers
            const PackUnit next = load_pack_unit<k420>(jb, u + kPackDepth * T, nunits);
            const PackUnit cur = take_pack_unit<k420>(ahead[j], u, nunits);
            ahead[j] = next;
            const uint32_t m = cur.rec.x;                // (0 beyond the last unit: no bits)
            const uint32_t nw = ((m >> 16) + 31u) >> 5;
            uint32_t len = 0, dl = 0, dcw = 0;
            if (u < nunits) {
                dcw = dc_code<k420>(s_dc, u, m, cur.prev, &dl);
                len = dl + (m >> 16);
            }
            uint32_t chunk;
            const uint32_t ex = wg_exclusive_scan(len, s_w, &chunk);
            const uint32_t carry = s_carry;
            if (u < nunits) {
                const uint32_t off = carry + ex;
                ((global_u32 *)jb.unit_off)[u] = off;          // (global, not flat: see global_u32)
                win_or(s_win, 0u, off, dcw);
                // (a record's unused words are zero and win_or places no zero word: no test of nw for the first three)
                win_or(s_win, 0u, (uint64_t)off + dl, cur.rec.y);
                win_or(s_win, 0u, (uint64_t)off + dl + 32u, cur.rec.z);
                win_or(s_win, 0u, (uint64_t)off + dl + 64u, cur.rec.w);
                for (uint32_t w = kUnitAcWords; w < nw; ++w)
                    win_or(s_win, 0u, (uint64_t)off + dl + 32u * w, ((const global_u32 *)jb.acbits)[(size_t)u * kAcWordsPerUnit + w]);
            }
            __syncthreads();
            if (tid == 0u) s_carry = carry + chunk;
            __syncthreads();
        }
    }
    const uint32_t total_bits = s_carry;
    if (tid == 0u) jb.unit_off[nunits] = total_bits;
    __threadfence_block();
    __syncthreads();
    const uint32_t nbytes = (total_bits + 7u) >> 3, limit = jb.dst_cap;
    // everything in front of the scan data
    const uint8_t *hdr = reinterpret_cast<const uint8_t *>(kOwn ? own + kJpegOptHeader : arena + jb.tab_off);
    const uint32_t hdr_bytes = kOwn ? own[kJpegOptHdrLen] : kJpegHeaderBytes;
    for (uint32_t i = tid; i < hdr_bytes; i += T) if (i < limit) jb.dst[i] = hdr[i];

    uint32_t ff_before = 0; // stuffed bytes emitted by earlier windows (same value in every thread)
    for (uint32_t wbase = 0; wbase * 32ull < total_bits; wbase += kWinWords) {
        const uint64_t wb = (uint64_t)wbase * 32u, we = wb + (uint64_t)kWinWords * 32u;
        if (wbase != 0u) { // (the first window was filled by the pass above)
            for (uint32_t i = tid; i < kWinWords; i += T) s_win[i] = 0u;
            // blocks that touch this window: offsets are ascending, so two binary searches bound them
            if (tid == 0u) {
                uint32_t lo = 0, hi = nunits;            // first u with unit_off[u + 1] > wb
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (jb.unit_off[mid + 1u] > wb) hi = mid; else lo = mid + 1u; }
                s_lo = lo;
                uint32_t lo2 = lo, hi2 = nunits;         // first u with unit_off[u] >= we
                while (lo2 < hi2) { const uint32_t mid = (lo2 + hi2) >> 1; if (jb.unit_off[mid] >= we) hi2 = mid; else lo2 = mid + 1u; }
                s_hi = lo2;
            }
        } else if (tid == 0u) { s_lo = 0u; s_hi = 0u; }
        __syncthreads();
        const uint32_t u_lo = s_lo, u_hi = s_hi;
        // 2 lanes per block (a block's AC code is 1-3 words in ordinary pictures): lane 0 of the pair also places the DC code
        for (uint32_t ub = u_lo; ub < u_hi; ub += T / 2u) {
            const uint32_t u = ub + (tid >> 1), j = tid & 1u;
            if (u < u_hi) {
                const PackUnit p = take_pack_unit<k420>(load_pack_unit<k420>(jb, u, u_hi), u, u_hi);
                const uint32_t m = p.rec.x, off = jb.unit_off[u];
                uint32_t dl;
                const uint32_t dcw = dc_code<k420>(s_dc, u, m, p.prev, &dl);
                if (j == 0u) win_or(s_win, wbase, off, dcw);
                const uint32_t nw = ((m >> 16) + 31u) >> 5;
                // words j and j + 2 of the pair's split: lane 0 takes ac[0] and ac[2], lane 1 ac[1] (unused words are zero)
                win_or(s_win, wbase, (uint64_t)off + dl + 32u * j, j ? p.rec.z : p.rec.y);
                if (j == 0u) win_or(s_win, wbase, (uint64_t)off + dl + 64u, p.rec.w);
                for (uint32_t w = j ? 3u : 4u; w < nw; w += 2u) // the words past the record: lane 1 goes on with 3, lane 0 with 4
                    win_or(s_win, wbase, (uint64_t)off + dl + 32u * w, ((const global_u32 *)jb.acbits)[(size_t)u * kAcWordsPerUnit + w]);
            }
        }
        __syncthreads();
        // BitWriter::pad_byte = write_bits(0x7F, 7): the last partial byte is filled with ones
        if (tid == 0u && (total_bits & 7u) && (total_bits >> 5) >= wbase && (total_bits >> 5) < wbase + kWinWords)
            s_win[(total_bits >> 5) - wbase] |= (0xFFu >> (total_bits & 7u)) << (24u - 8u * ((total_bits >> 3) & 3u));
        __syncthreads();
        // 0xFF -> 0xFF 0x00 stuffing: scan of the 0xFF counts, then every thread writes its four bytes
        const uint32_t win_bytes = (uint32_t)min((uint64_t)kWinWords * 4u, (uint64_t)nbytes - (uint64_t)wbase * 4u);
        if (tid == 0u) s_carry = 0u;
        __syncthreads();
        for (uint32_t base = 0; base < win_bytes; base += 4u * T) {
            const uint32_t i = base + tid * 4u;
            const uint32_t word = i < win_bytes ? s_win[i >> 2] : 0u;     // stream order = most significant byte first
            const uint32_t valid = i < win_bytes ? (win_bytes - i < 4u ? win_bytes - i : 4u) : 0u;
            uint32_t ff = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) ff += (k < valid && ((word >> (24u - 8u * k)) & 255u) == 255u) ? 1u : 0u;
            uint32_t chunk;
            const uint32_t ex = wg_exclusive_scan(ff, s_w, &chunk);
            const uint32_t carry = s_carry;
            uint64_t o = (uint64_t)hdr_bytes + (uint64_t)wbase * 4u + i + ff_before + carry + ex;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                if (k < valid) {
                    const uint32_t b = (word >> (24u - 8u * k)) & 255u;
                    if (o < limit) jb.dst[o] = (uint8_t)b;
                    ++o;
                    if (b == 255u) { if (o < limit) jb.dst[o] = 0u; ++o; }
                }
            }
            __syncthreads();
            if (tid == 0u) s_carry = carry + chunk;
            __syncthreads();
        }
        ff_before += s_carry;
        __syncthreads();
    }
    if (tid == 0u) {
        const uint64_t end = (uint64_t)hdr_bytes + nbytes + ff_before;
        if (end + 2u <= limit) {
            jb.dst[end] = 0xFF; jb.dst[end + 1u] = 0xD9; // EOI
            jb.result[1] = (uint32_t)(end + 2u);
            if constexpr (kOwn) { if (own[kJpegOptFlag]) atomicOr(&jb.result[0], FL_JPEG_RESULT_OPTIMIZED); }
        } else {
            jb.result[1] = 0u;
            atomicOr(&jb.result[0], FL_JPEG_RESULT_OVERFLOW);
        }
    }
}

} // namespace

} // namespace fl
