// fl_batch.cpp -- the batch planner and launcher: geometry, buffer chain, table lookups, descriptor staging and kernel
// launches of one batch on ONE device context (reference order of operations: src/handler.rs:221-278), the read-back of
// per-image result words, and the host-memory batch built on top of it.  Resample and blur are planned here; a picture's
// front end (planes, an encoded stream) is fl_encode.cpp's.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <memory>
#include <optional>

#include "fl_context.h"

using namespace fl;

namespace {

// ---- batch execution -------------------------------------------------------

enum Stage1Kind { S1_NONE = 0, S1_PLACE = 1, S1_GENERIC = 2, S1_STREAM = 3, S1_NEAREST = 4, S1_MFMA = 5, S1_TILE = 6, S1_WTILE = 7 };
constexpr size_t kNoScratch = ~(size_t)0; // Work: an output that does not go to scratch

struct Work {
    flgpu_plan plan;
    const flgpu_params *p;
    uint32_t cs, pre, sw, sh;
    Stage1Kind s1;
    const uint8_t *src;
    uint8_t *s1_dst = nullptr;   // output of stage 1 (== src when S1_NONE)
    uint8_t *blur_dst = nullptr; // output of the blur stage (or null)
    uint8_t *final_dst;
    size_t s1_off = kNoScratch, blur_off = kNoScratch; // where stage 1's / the blur's output goes to scratch A / B: its offset there
    AxisKey vk, hk;
    const HostAxis *va = nullptr, *ha = nullptr;
    uint32_t vtab = 0, htab = 0;
    const StreamPlan *splan = nullptr;
    const MfmaPlan *mplan = nullptr;
    const std::vector<MfmaItem> *mitems = nullptr; // its workgroups for the band count of this batch
    bool unaligned = false;
    uint32_t jpeg_tab = 0;
    uint32_t orient = 0, raw_w = 0, raw_h = 0; // EXIF orientation pre-pass (2..8), source size before it
    size_t orient_off = 0;
    uint32_t tile_w = 0;        // S1_TILE: output columns per tile (power of two)
    uint32_t tile_vplan = 0;    // S1_TILE: arena offset of the vertical band tables (build_tile_vplan)
    size_t align_off = kNoScratch; // misaligned device source of a matrix-pipe geometry: offset of its aligned copy in d_tmp_al
    const uint8_t *raw_src = nullptr;
    const WtPlan *wplan = nullptr;   // S1_WTILE: the window-tile matrix-pipe kernel's tables
    const WtPlan *bwplan = nullptr;  // ... for the blur stage, where that kernel serves it
    bool luma_mid = false;           // grey picture on a grey frame + blur on that kernel: stage 1 leaves the UNFRAMED Luma8 picture, the blur reads it through a virtual frame and writes Rgba8
};

// A stage-1 launch: pictures one kernel instantiation serves together.  S1_WTILE: nslot register sets; S1_MFMA: the plans'
// layout and arithmetic (ops_in_lds, wide, full, compact); S1_STREAM: nacc accumulator slots, rows that are not dword aligned
// (unaligned: the funnel-shift variant); lb: a letterboxed destination.
struct ResampleKey {
    Stage1Kind s1;
    uint32_t nslot, nacc, cs, pre;
    bool ops_in_lds, wide, full, compact, unaligned, lb;
    // Launches go out in the order they always have: by this word (the stage kind, its flags from bit 8 up), then cs, pre, lb.
    uint32_t rank() const { return s1 | nslot << 8 | ops_in_lds << 8 | wide << 9 | full << 10 | compact << 11 | nacc << 8 | unaligned << 16; }
    bool operator<(const ResampleKey &o) const { return std::make_tuple(rank(), cs, pre, lb) < std::make_tuple(o.rank(), o.cs, o.pre, o.lb); }
};

// A blur launch: the window-tile kernel (nslot register sets; luma_mid: one channel read through a virtual frame) or blur_tile_kernel
// (lanes per workgroup, channels filtered); c = channels of the blurred picture.  blur_tile_kernel's launches go out first.
struct BlurKey {
    bool wtile;
    uint32_t nslot, lanes, c, filtered;
    bool luma_mid;
    bool operator<(const BlurKey &o) const { return std::tie(wtile, nslot, lanes, c, filtered, luma_mid) < std::tie(o.wtile, o.nslot, o.lanes, o.c, o.filtered, o.luma_mid); }
};

// One launch of stage 1 or of the blur: its jobs and work items in the batch's arrays, and what its kernel needs besides
// (matrix-pipe kernel: widest strip, persistent workgroups and their item lists; blur_tile_kernel: grid, whether it serves the launch).
template <class Key> struct Launch {
    Key k;
    uint32_t job_base = 0, njobs = 0, item_base = 0, nitems = 0, max_nout = 0, grid = 0, wg_base = 0, blur_grid_x = 0;
    bool blur_tiled = false;
    LaunchGeneric g{};
    size_t lds = 0, mid_floats = 0;
};

// Bytes (or records) of every scratch buffer a batch needs; while pictures are added, the running totals are their offsets.
struct ScratchSizes {
    size_t a = 0, b = 0, o = 0, al = 0; // stage 1's output, the blur's, oriented sources, aligned copies
    EncodeScratch enc;
};

// What passes between the phases of run_batch_device.
struct Batch {
    size_t n;
    flgpu_image *dsts;
    const DebugSwitches &dbg; // the context's switches (flgpu_debug_set; tests and A/B runs)
    std::vector<Work> work;
    ScratchSizes scratch;
    // launches, and the arrays their descriptor block holds
    std::vector<LaunchGeneric> orient_launches; // EXIF orientation pre-pass, one per channel count
    std::vector<Launch<ResampleKey>> s1_launches;
    std::vector<Launch<BlurKey>> blur_launches;
    std::vector<Job> jobs;
    std::vector<StreamItem> items;
    std::vector<MfmaItem> mitems;
    std::vector<MfmaReq> mreqs;
    std::vector<uint32_t> mwg; // matrix-pipe launches with persistent workgroups: {first item, items} of every workgroup
    EncodeJobs enc; // the front ends' jobs and launches (fl_encode.h)
    size_t mid_floats_max = 0;
    bool has_results = false, has_err_word = false;
    // the staged descriptor block
    DescSlot *slot = nullptr;
    uint32_t *status_dev = nullptr;
    struct {
        const Job *jobs; const StreamItem *items; const MfmaItem *mitems; const MfmaReq *mreqs; const uint32_t *mwg;
    } d{}; // the arrays' device copies (the front ends': enc.d)
    Batch(flgpu_ctx *c, size_t n_, flgpu_image *dsts_) : n(n_), dsts(dsts_), dbg(*c->dbg), work(n_) {}
};

// The window-tile matrix-pipe kernel (fl_wtile.h) for mild ratios, up-scales and blurs: full-width arithmetic only (mfma_arith = 1
// asks for rounds 2-3's packed arithmetic: A/B runs and the tests that keep the packed kernel's bars); no_wtile keeps the f32 vector kernels.
bool use_wtile(const DebugSwitches &dbg) { return !dbg.on(DBG_NO_WTILE) && !dbg.on(DBG_NO_MFMA) && !dbg.on(DBG_FORCE_GENERIC) && !dbg.on(DBG_MFMA_ARITH); }

// Channels the blur really has to filter: a letterboxed picture of an opaque source has alpha == 255 everywhere,
// and a grey one on a grey fill has R == G == B (see blur_tile_kernel).
uint32_t blur_channels(const Work &w)
{
    uint32_t ce = w.plan.out_c;
    if (w.plan.letterboxed && (w.cs == 1 || w.cs == 3)) {
        const bool grey = mid_channels(w.cs, w.pre) == 1 && w.p->fill_r == w.p->fill_g && w.p->fill_g == w.p->fill_b;
        ce = grey ? 1u : 3u;
    }
    return ce;
}

// Row bands per picture for the window-tile kernel: small batches are cut so that the chip still sees a few hundred workgroups
// (the result does not depend on the cut: every M-tile is computed from the same rows by the same instructions).
uint32_t wtile_bands(const DebugSwitches &dbg, const WtPlan &p, size_t pictures)
{
    if (const int64_t b = dbg.get(DBG_FORCE_BANDS)) return (uint32_t)std::max<int64_t>(1, b);
    const size_t wgs = std::max<size_t>(1, pictures * p.n_strips);
    return (uint32_t)std::min<size_t>(p.n_mt, std::max<size_t>(1, (512 + wgs - 1) / wgs));
}

// Which items each persistent workgroup of a matrix-pipe launch walks (full-width arithmetic, fl_mfma.hip): `items` come in the classic
// order (pictures x strips [x bands], longest first, strips of a picture on one XCD) and leave in WORKGROUP-MAJOR order; lists[2 b],
// lists[2 b + 1] = first item and item count of workgroup b.
//
// General launch: workgroup b takes items b, b + G, b + 2 G, ... of the classic order.
//
// Uniform launch (every picture the same plan, cut into the same S strips, whole pictures): a workgroup keeps ONE strip, so that its walk
// goes from one picture's rows into the next one's without a new set-up (fl_mfma.hip: a "light" transition -- no operand copy, no tile
// table, no barrier, the last tile converted on the way), and the S strips of a picture run on one XCD at the same time (hardware
// deals workgroup b to XCD (b + const) mod 8; the strips share their halo columns through that XCD's L2): per XCD floor(slots / S)
// triples of neighbouring slots, the slots left over form cross-XCD triples, and G mod S workgroups stay free.  Every triple takes
// R = floor(pictures / triples) pictures.  The pictures left over are cut into row bands of `plan` (an item each: a band computes
// exactly what the full walk computes for its rows) and dealt to the workgroups with the least work -- the free ones first --, so
// that the launch ends within one band of its average instead of one picture.
void assign_items(std::vector<MfmaItem> &mitems, size_t base, uint32_t &nitems, uint32_t G, MfmaPlan *plan, std::vector<uint32_t> &lists)
{
    MfmaItem *items = mitems.data() + base;
    const uint32_t n = nitems;
    std::vector<std::vector<MfmaItem>> per_wg(G);
    // General launch: the classic order has the strips of a picture at positions that agree modulo 8 (the XCD they should run on);
    // item k goes to the least-loaded workgroup of ITS class b = k (mod 8) -- round-robin would do for equal items, but a mixed
    // launch (config 4: 4K items walk twice the K-blocks of 1080p ones) needs the balance a dynamic dispatch used to give
    auto classic = [&]() {
        std::vector<uint64_t> load(G, 0);
        for (uint32_t k = 0; k < n; ++k) {
            uint32_t best = k % 8u < G ? k % 8u : 0u;
            for (uint32_t b = best; b < G; b += 8u) if (load[b] < load[best]) best = b;
            per_wg[best].push_back(items[k]);
            load[best] += items[k].kb1 - items[k].kb0 + 2u;
        }
    };
    // uniform?  (the classic order of a uniform launch: 8 pictures interleaved strip by strip; recover pictures x strips from the jobs)
    bool uniform = plan && n >= 2 && G >= 16;
    std::vector<uint32_t> strips, jobs_in_order;
    if (uniform) {
        std::map<uint32_t, std::vector<MfmaItem>> by_job;
        for (uint32_t k = 0; k < n; ++k) {
            if (!by_job.count(items[k].job)) jobs_in_order.push_back(items[k].job);
            by_job[items[k].job].push_back(items[k]);
        }
        for (const MfmaItem &a : by_job[jobs_in_order[0]]) strips.push_back(a.strip_off);
        const uint32_t S = (uint32_t)strips.size();
        uniform = S >= 2 && S <= 8 && G >= 8u * S && n == S * jobs_in_order.size();
        for (uint32_t j : jobs_in_order) {
            if (!uniform) break;
            const auto &v = by_job[j];
            if (v.size() != S) { uniform = false; break; }
            for (uint32_t s2 = 0; s2 < S; ++s2)
                if (v[s2].strip_off != strips[s2] || v[s2].vplan_off != items[0].vplan_off || v[s2].kb0 != items[0].kb0 || v[s2].kb1 != items[0].kb1 ||
                    v[s2].tile0 != items[0].tile0 || v[s2].tile1 != items[0].tile1 || v[s2].tile0 != 0u || v[s2].tile1 != (uint32_t)plan->tiles.size())
                    uniform = false;
        }
        if (uniform) {
            const uint32_t P = (uint32_t)jobs_in_order.size();
            // triples of workgroups: inside an XCD first, then across
            std::vector<std::vector<uint32_t>> triples;
            std::vector<uint32_t> leftover;
            for (uint32_t x = 0; x < 8; ++x) {
                const uint32_t slots = (G - x + 7u) / 8u, t_x = slots / S;
                for (uint32_t j = 0; j < slots; ++j) {
                    const uint32_t b = 8u * j + x;
                    if (j < t_x * S) { if (j % S == 0) triples.emplace_back(); triples.back().push_back(b); }
                    else leftover.push_back(b);
                }
            }
            std::sort(leftover.begin(), leftover.end());
            for (uint32_t q = 0; q + S <= leftover.size(); q += S) triples.emplace_back(leftover.begin() + q, leftover.begin() + q + S);
            const uint32_t T = (uint32_t)triples.size(), R = T ? P / T : 0u;
            if (!R) uniform = false;
            else {
                for (uint32_t r = 0; r < R; ++r)
                    for (uint32_t t = 0; t < T; ++t) {
                        const auto &v = by_job[jobs_in_order[r * T + t]];
                        for (uint32_t s2 = 0; s2 < S; ++s2) per_wg[triples[t][s2]].push_back(v[s2]);
                    }
                // the pictures left over, in bands
                const uint32_t Lp = P - R * T;
                if (Lp) {
                    const uint32_t nt = (uint32_t)plan->tiles.size();
                    const uint32_t nb = std::max(1u, std::min(nt, (2u * G + Lp * S - 1u) / (Lp * S)));
                    const std::vector<MfmaItem> &bands = plan->items_for(nb);
                    std::vector<MfmaItem> units;
                    for (uint32_t p2 = R * T; p2 < P; ++p2)
                        for (MfmaItem u : bands) { u.job = jobs_in_order[p2]; units.push_back(u); }
                    std::stable_sort(units.begin(), units.end(), [](const MfmaItem &x, const MfmaItem &y) { return x.kb1 - x.kb0 > y.kb1 - y.kb0; });
                    // least-loaded workgroup first (load in K-blocks; a transition counts like two)
                    std::vector<uint64_t> load(G, 0);
                    for (uint32_t b = 0; b < G; ++b) for (const MfmaItem &a : per_wg[b]) load[b] += a.kb1 - a.kb0;
                    for (const MfmaItem &u : units) {
                        uint32_t best = 0;
                        for (uint32_t b = 1; b < G; ++b) if (load[b] < load[best]) best = b;
                        per_wg[best].push_back(u);
                        load[best] += u.kb1 - u.kb0 + 2u;
                    }
                }
            }
        }
    }
    if (!uniform) { for (auto &v : per_wg) v.clear(); classic(); }
    // flatten, workgroup-major
    std::vector<MfmaItem> flat;
    lists.assign(2u * G, 0u);
    for (uint32_t b = 0; b < G; ++b) {
        lists[2 * b] = (uint32_t)flat.size();
        lists[2 * b + 1] = (uint32_t)per_wg[b].size();
        flat.insert(flat.end(), per_wg[b].begin(), per_wg[b].end());
    }
    mitems.resize(base);
    mitems.insert(mitems.end(), flat.begin(), flat.end());
    nitems = (uint32_t)flat.size();
}

void fill_job(const Work &w, Job &j)
{
    memset(&j, 0, sizeof(j));
    const flgpu_plan &pl = w.plan;
    j.src = w.src;
    j.dst = w.s1_dst;
    j.src_bytes = w.sw * w.sh * w.cs;
    j.sw = w.sw; j.sh = w.sh;
    j.rw = pl.resized_w; j.rh = pl.resized_h;
    j.cx = pl.crop_x; j.cy = pl.crop_y;
    if (pl.letterboxed) {
        j.cw = std::min(pl.resized_w - pl.crop_x, pl.out_w - pl.place_x);
        j.ch = std::min(pl.resized_h - pl.crop_y, pl.out_h - pl.place_y);
    } else {
        j.cw = pl.out_w; j.ch = pl.out_h;
    }
    j.dw = pl.out_w; j.dh = pl.out_h;
    j.ox = pl.place_x; j.oy = pl.place_y;
    if (w.luma_mid) { j.dw = j.cw; j.dh = j.ch; j.ox = 0; j.oy = 0; } // (the picture alone, tightly packed: the blur supplies the frame)
    j.fill = (uint32_t)w.p->fill_r | ((uint32_t)w.p->fill_g << 8) | ((uint32_t)w.p->fill_b << 16) | (255u << 24);
    j.vtab = w.vtab; j.htab = w.htab;
    j.pad1 = w.tile_w;
    j.pad0 = w.tile_vplan;
    if (w.s1 == S1_NEAREST) {
        // sample.rs: ratio = in as f32 / out as f32, carried as bits where the Lanczos3 jobs carry table offsets
        const float ry = (float)w.sh / (float)pl.resized_h, rx = (float)w.sw / (float)pl.resized_w;
        memcpy(&j.vtab, &ry, 4); memcpy(&j.htab, &rx, 4);
    }
}


// Tile width of the tiled two-pass kernel for output columns [cx, cx + cw) of axis h: the largest power of two (256 .. 16) whose
// tiles all have a source column window that fits the kernel's LDS tile (kTileLdsFloats / (8 rows x channels)); 0 = none does
// (ratios beyond ~7 with four channels: those geometries belong to the other kernels anyway), or a band of 8 output rows [cy + 8 k, ...)
// of axis v touches more source rows than the kernel's table of vertical weights holds.
uint32_t tile_width_for(const HostAxis &h, const HostAxis &v, uint32_t cx, uint32_t cw, uint32_t cy, uint32_t ch, uint32_t mc)
{
    for (uint32_t y0 = cy; y0 < cy + ch; y0 += 8u) {
        const uint32_t y1 = std::min(y0 + 8u, cy + ch);
        if (v.left[y1 - 1] + v.count[y1 - 1] - v.left[y0] > kTileVRows) return 0;
    }
    const uint32_t nc_max = kTileLdsFloats / (8u * mc); // (8 = the kernel's rows per tile)
    for (uint32_t tw = 256; tw >= 16; tw >>= 1) {
        bool fits = true;
        for (uint32_t x0 = cx; x0 < cx + cw && fits; x0 += tw) {
            const uint32_t x1 = std::min(x0 + tw, cx + cw);
            if (h.left[x1 - 1] + h.count[x1 - 1] - h.left[x0] > nc_max) fits = false;
            if (h.woff[x1 - 1] + h.count[x1 - 1] - h.woff[x0] > kTileWeightFloats) fits = false;
        }
        if (fits) return tw;
    }
    return 0;
}

// The tiled two-pass kernel's vertical tables for output rows [cy, cy + ch) of axis v: every band of 8 rows gets its source row
// range and a dense [source row][output row] weight block, so that the kernel's band loop starts with one coalesced copy instead
// of three dependent table look-ups per weight.
void build_tile_vplan(const HostAxis &v, uint32_t cy, uint32_t ch, std::vector<uint32_t> &blk)
{
    const uint32_t nb = (ch + 7u) / 8u;
    uint32_t stride = 1;
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t y0 = cy + 8u * b, y1 = std::min(y0 + 8u, cy + ch);
        stride = std::max(stride, v.left[y1 - 1] + v.count[y1 - 1] - v.left[y0]);
    }
    TileVPlanHeader hd{nb, stride, (uint32_t)(sizeof(TileVPlanHeader) / 4), (uint32_t)(sizeof(TileVPlanHeader) / 4) + 2u * nb};
    blk.assign((size_t)hd.dense_off + (size_t)nb * stride * 8u, 0u);
    memcpy(blk.data(), &hd, sizeof(hd));
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t y0 = cy + 8u * b, y1 = std::min(y0 + 8u, cy + ch);
        const uint32_t top = v.left[y0], rv = v.left[y1 - 1] + v.count[y1 - 1] - top;
        blk[hd.bands_off + 2u * b] = top;
        blk[hd.bands_off + 2u * b + 1u] = rv;
        float *dense = reinterpret_cast<float *>(blk.data() + hd.dense_off) + (size_t)b * stride * 8u;
        for (uint32_t oy = y0; oy < y1; ++oy)
            for (uint32_t k = 0; k < v.count[oy]; ++k) dense[(size_t)(v.left[oy] + k - top) * 8u + (oy - y0)] = v.weights[v.woff[oy] + k];
    }
}

// XCD-aware numbering: workgroups are dealt to the 8 XCDs round-robin in launch order and each XCD has its own L2.
// The strips of one picture re-read each other's halo columns, so inside every run of equally long workgroups the
// items of 8 pictures are interleaved: picture p's strips get launch indices congruent modulo 8 (same XCD, close
// in time) and the halo is served by that XCD's L2 instead of HBM.  Speed only; any placement is correct.
template <class Item, class Len>
void xcd_interleave(Item *first, uint32_t nitems, Len len_of)
{
#ifdef FL_EXPERIMENT
    static const bool no_xcd_order = [] { const char *e = getenv("FLGPU_NO_XCD_ORDER"); return e && e[0] == '1'; }(); // A/B experiments (experiment builds only)
#else
    constexpr bool no_xcd_order = false;
#endif
    std::vector<Item> tmp;
    for (uint32_t a = 0; a < nitems && !no_xcd_order;) {
        uint32_t b = a;
        const uint32_t len = len_of(first[a]);
        while (b < nitems && len_of(first[b]) == len) ++b;
        // items of one job are consecutive inside the run (stable sort): collect up to 8 jobs at a time
        for (uint32_t g0 = a; g0 < b;) {
            uint32_t g1 = g0, njob = 0, prev = 0xffffffffu, per = 0, cur = 0;
            bool uniform = true;
            while (g1 < b) {
                if (first[g1].job != prev) {
                    if (njob == 8) break;
                    if (njob >= 1) { if (per == 0) per = cur; else if (cur != per) uniform = false; }
                    ++njob; prev = first[g1].job; cur = 0;
                }
                ++cur; ++g1;
            }
            if (per == 0) per = cur; else if (cur != per) uniform = false;
            if (uniform && njob > 1 && per > 1) {
                tmp.assign(first + g0, first + g1);
                for (uint32_t s2 = 0; s2 < per; ++s2)
                    for (uint32_t j2 = 0; j2 < njob; ++j2) first[g0 + s2 * njob + j2] = tmp[j2 * per + s2];
            }
            g0 = g1;
        }
        a = b;
    }
}


// ---- planning ------------------------------------------------------------------------------------------------------------------

// Validates and plans every picture of the batch and sizes its scratch.  Nothing is enqueued before all of them have passed.
int plan_pictures(Batch &B, const flgpu_image *srcs, const flgpu_params *ps, bool same_params)
{
    for (size_t i = 0; i < B.n; ++i) {
        Work &w = B.work[i];
        const flgpu_image &s = srcs[i];
        w.p = same_params ? &ps[0] : &ps[i];
        if (!s.data || !B.dsts[i].data) return FLGPU_ERR_INVALID_ARG;
        int rc = flgpu_plan_output(w.p, s.width, s.height, s.channels, &w.plan);
        if (rc) return rc;
        if (s.capacity < (uint64_t)s.width * s.height * s.channels) return FLGPU_ERR_INVALID_ARG;
        if (B.dsts[i].capacity < w.plan.out_bytes) return FLGPU_ERR_BUFFER_TOO_SMALL;
        w.cs = s.channels; w.sw = w.plan.src_w; w.sh = w.plan.src_h; // size after apply_orientation
        w.raw_w = s.width; w.raw_h = s.height;
        w.orient = w.p->orientation >= 2 ? w.p->orientation : 0;
        if (w.orient) { w.orient_off = B.scratch.o; B.scratch.o += align_up((size_t)s.width * s.height * s.channels, 256); }
        w.pre = w.p->grayscale ? PRE_GRAY : (w.p->inverse ? PRE_INVERT : PRE_NONE);
        w.src = s.data;
        w.final_dst = B.dsts[i].data;
        const flgpu_plan &pl = w.plan;
        const bool cropped = pl.crop_x || pl.crop_y || pl.out_w != pl.resized_w || pl.out_h != pl.resized_h;
        // grayscale of Luma/LumaA and "no-op" pre-ops change nothing
        const bool pre_changes = (w.pre == PRE_INVERT) || (w.pre == PRE_GRAY && w.cs >= 3);
        if (!pre_changes) w.pre = PRE_NONE;
        if (pl.resampled) w.s1 = w.p->filter == FLGPU_FILTER_NEAREST ? S1_NEAREST : S1_GENERIC;
        else if (pre_changes || pl.letterboxed || cropped) w.s1 = S1_PLACE;
        else w.s1 = S1_NONE;
        // Which resample kernel serves a request is a function of the REQUEST (geometry, channels, pre-op), never of where the
        // caller's buffer happens to start: the matrix-pipe kernel moves 16-byte pieces of a row, so a source whose rows qualify
        // but whose base is not 16-byte aligned (only possible through the device-batch entry point; staged and decoded sources
        // are 256-byte aligned) is copied to aligned scratch first.  The two kernels may differ by 1 LSB; an HTTP cache in front of
        // the service must not see that difference come and go with an address.
        // (only where that kernel can be the one: its own gate below -- no pre-op, rows of at least 64 bytes, not switched off -- and a
        // ratio above the window-tile kernel's range, which takes any alignment; everything else is served by kernels that do not care)
        // (from ratio 2 up whether or not the window-tile kernel is on: that kernel takes any alignment, but where ITS planner refuses
        // a geometry below ratio 2.5 the request falls through to the matrix-pipe branch -- which must not then depend on the address)
        const bool mfma_candidate = !B.dbg.on(DBG_NO_MFMA) && !B.dbg.on(DBG_FORCE_GENERIC) && (size_t)w.sw * w.cs >= 64u && (uint64_t)w.sh >= 2u * (uint64_t)pl.resized_h;
        if (pl.resampled && w.s1 == S1_GENERIC && !pre_changes && !w.orient && mfma_candidate && ((size_t)w.sw * w.cs) % 16u == 0 && (uintptr_t)s.data % 16u != 0) {
            w.align_off = B.scratch.al;
            B.scratch.al += align_up((size_t)s.width * s.height * s.channels, 256);
        }
        const bool blur = w.p->blur_sigma > 0.0f;
        const bool fe = w.p->front_end != FLGPU_FE_NONE;
        // buffer chain: stage 1 -> blur -> front end, each writing the final destination if it is the last stage, else scratch
        if (w.s1 != S1_NONE && !blur && !fe) w.s1_dst = w.final_dst;
        else if (w.s1 != S1_NONE) { w.s1_off = B.scratch.a; B.scratch.a += align_up(pl.pixel_bytes, 256); }
        if (blur && !fe) w.blur_dst = w.final_dst;
        else if (blur) { w.blur_off = B.scratch.b; B.scratch.b += align_up(pl.pixel_bytes, 256); }
        if ((rc = encode_plan_picture(*w.p, pl, B.scratch.enc))) return rc;
    }
    return FLGPU_OK;
}

// Reserves the batch's scratch, points every picture at its part of it, and enqueues the copies of the sources that the
// orientation pre-pass and the alignment rule move.
int reserve_scratch(flgpu_ctx *c, Batch &B, hipStream_t st)
{
    const ScratchSizes &sz = B.scratch;
    if (int rc = encode_reserve(c, sz.enc)) return rc;
    FL_HIP(c, c->d_tmp_o.reserve(sz.o), "orientation scratch");
    FL_HIP(c, c->d_tmp_al.reserve(sz.al), "alignment scratch");
    for (auto &w : B.work)
        if (w.align_off != kNoScratch) {
            uint8_t *al = static_cast<uint8_t *>(c->d_tmp_al.p) + w.align_off;
            FL_HIP(c, hipMemcpyAsync(al, w.src, (size_t)w.sw * w.sh * w.cs, hipMemcpyDeviceToDevice, st), "alignment copy");
            w.src = al;
        }
    FL_HIP(c, c->d_tmp_a.reserve(sz.a), "scratch A");
    FL_HIP(c, c->d_tmp_b.reserve(sz.b), "scratch B");
    for (auto &w : B.work) {
        if (w.orient) { w.raw_src = w.src; w.src = static_cast<uint8_t *>(c->d_tmp_o.p) + w.orient_off; }
        if (w.s1 == S1_NONE) w.s1_dst = const_cast<uint8_t *>(w.src);
        if (w.s1_off != kNoScratch) w.s1_dst = static_cast<uint8_t *>(c->d_tmp_a.p) + w.s1_off;
        if (w.blur_off != kNoScratch) w.blur_dst = static_cast<uint8_t *>(c->d_tmp_b.p) + w.blur_off;
    }
    return FLGPU_OK;
}

// ---- tables ----------------------------------------------------------------------------------------------------------------------

// Planning stops short of the arena's last 1024 words: the batch starts over after a reset instead.
bool arena_nearly_full(const flgpu_ctx *c) { return c->h_arena.size() >= c->arena_cap_words - 1024; }

// The arena offset of the table block `cache` holds under `key`; on a miss build(blk) makes the block and it is appended.
// 0 = the arena is full.
template <class Map, class Build> uint32_t cached_block(flgpu_ctx *c, Map &cache, const typename Map::key_type &key, Build &&build)
{
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    std::vector<uint32_t> blk;
    build(blk);
    const uint32_t off = arena_append(c, blk.data(), blk.size());
    if (off) cache.emplace(key, off);
    return off;
}

// One resample kernel asked for picture w (j: its job, for the kept window): w.s1 becomes that kernel's if its planner accepts the
// geometry.  false = the table arena is full.
bool try_wtile(flgpu_ctx *c, Work &w, const Job &j)
{
    WtPlan *wp = get_wtile_plan(c, w.vk, *w.va, w.hk, *w.ha, j.cx, j.cy, j.cw, j.ch, w.cs);
    if (wp->arena_full || arena_nearly_full(c)) return false;
    if (wp->ok) { w.s1 = S1_WTILE; w.wplan = wp; }
    return true;
}

bool try_mfma(flgpu_ctx *c, const DebugSwitches &dbg, size_t n_resample, Work &w, const Job &j)
{
    MfmaPlan *mp = get_mfma_plan(c, w.vk, *w.va, w.hk, *w.ha, j.cx, j.cy, j.cw, j.ch, w.cs, dbg.on(DBG_MFMA_ARITH) ? MFMA_ARITH_PACKED : MFMA_ARITH_FULL);
    if (mp->arena_full || arena_nearly_full(c)) return false;
    if (!mp->ok) return true;
    uint32_t nbands = (uint32_t)std::max<int64_t>(0, dbg.get(DBG_FORCE_BANDS));
    if (!nbands && n_resample < 128) {
        // A small launch: bands of rows so that every CU has an item -- and so that the items come out in whole rounds of the
        // workgroups.  (Until round 5: ceil(256 / (3 n)) bands; 13 files x 3 strips x 7 bands = 273 items on 256 workgroups,
        // i.e. two rounds of items a seventh of a strip long where one round of sixths does: 84 us per batch of file requests.)
        // The cost of a band count: rounds x (the longest item's K-blocks -- the bands' halos are in there -- + a transition's two).
        const uint64_t G = std::max(1u, c->cu_count);
        uint64_t best = ~0ull;
        for (uint32_t b = 1; b <= std::min<uint32_t>(16u, (uint32_t)mp->tiles.size()); ++b) {
            const std::vector<MfmaItem> &cand = mp->items_for(b);
            uint32_t longest = 0;
            for (const MfmaItem &mi : cand) longest = std::max(longest, mi.kb1 - mi.kb0);
            const uint64_t cost = (((uint64_t)n_resample * cand.size() + G - 1) / G) * (longest + 2u);
            if (cost < best) { best = cost; nbands = b; }
        }
    }
    w.s1 = S1_MFMA; w.mplan = mp; w.mitems = &mp->items_for(std::max(nbands, 1u));
    return true;
}

bool try_stream(flgpu_ctx *c, const DebugSwitches &dbg, size_t n_resample, Work &w, const Job &j)
{
    uint32_t nbands = (uint32_t)std::max<int64_t>(0, dbg.get(DBG_FORCE_BANDS));
    // small batches: split images into row bands so that the chip still gets >= ~1024 workgroups
    if (!nbands && n_resample < 512) nbands = std::min((uint32_t)((1024 + n_resample * 2 - 1) / (n_resample * 2)), j.ch / 24u);
    nbands = std::min(std::max(nbands, 1u), std::max(1u, j.ch));
    const StreamPlan *sp = get_stream_plan(c, w.vk, *w.va, w.hk, *w.ha, j.cx, j.cy, j.cw, j.ch, nbands, w.cs, w.pre);
    if (arena_nearly_full(c)) return false;
    if (sp->ok) { w.s1 = S1_STREAM; w.splan = sp; }
    return true;
}

bool try_tile(flgpu_ctx *c, Work &w, const Job &j)
{
    const uint32_t tw = tile_width_for(*w.ha, *w.va, j.cx, j.cw, j.cy, j.ch, mid_channels(w.cs, w.pre));
    if (!tw) return true;
    const uint32_t off = cached_block(c, c->tile_vplans, std::make_tuple(w.vk, j.cy, j.ch), [&](std::vector<uint32_t> &blk) { build_tile_vplan(*w.va, j.cy, j.ch, blk); });
    if (off) { w.s1 = S1_TILE; w.tile_w = tw; w.tile_vplan = off; }
    return off != 0;
}

// Stage 1's resample kernel for picture w: sets w.s1 and its plan, the HBM two-pass kernels (S1_GENERIC) if no other takes it.
// false = the table arena is full.
bool route_resample(flgpu_ctx *c, const DebugSwitches &dbg, size_t n_resample, Work &w)
{
    w.vtab = get_axis(c, w.sh, w.plan.resized_h, FILTER_LANCZOS3, 0.0f, &w.vk, &w.va);
    w.htab = get_axis(c, w.sw, w.plan.resized_w, FILTER_LANCZOS3, 0.0f, &w.hk, &w.ha);
    if (!w.vtab || !w.htab) return false;
    w.s1 = S1_GENERIC;
    // rows that are not dword aligned: Rgb8 has a funnel-shift variant of the kernel, others use the generic path
    w.unaligned = ((w.sw * w.cs) % 4u != 0) || ((uintptr_t)w.src % 4u != 0);
    const bool force_generic = dbg.on(DBG_FORCE_GENERIC), lb_ok = !w.plan.letterboxed || (uintptr_t)w.s1_dst % 4u == 0;
    const bool wtile_ok = use_wtile(dbg) && (w.pre == PRE_NONE || w.pre == PRE_INVERT) && lb_ok;
    Job j; fill_job(w, j);
    // The matrix-pipe kernel takes down-scales (any channel count, no pre-op) whose rows are 16-byte aligned (it moves 16-byte pieces of a row
    // straight into LDS).  The choice depends on the request's geometry only, never on the batch around it.
    // Ratios below 2.5 (up-scales included) go to the window-tile kernel BEFORE the fused ones: measured 1.00 vs 1.03 ms per 256 at ratio 2.4 and -- against the
    // streaming f32 kernel, which serves what the matrix-pipe planner refuses down there -- 1.16 vs 2.10 at 2.13.  From 2.67 up the
    // streaming matrix-pipe kernel wins since its wide layout keeps operands in LDS (0.78 vs 0.92 at 2.67, 0.72 vs 0.80 at 3;
    // profiles/r04_wtile_experiments.txt); where ITS planner refuses a geometry below ratio 3.4, the window-tile kernel is asked again.
    // (wt_first, experiments: the window-tile kernel before the streaming matrix-pipe kernel)
    bool ok = true;
    if ((dbg.on(DBG_WTILE_FIRST) || 2u * w.sh < 5u * w.plan.resized_h) && wtile_ok) ok = try_wtile(c, w, j);
    if (ok && w.s1 == S1_GENERIC && w.pre == PRE_NONE && !force_generic && !dbg.on(DBG_NO_MFMA) && (w.sw * w.cs) % 16u == 0 && (uintptr_t)w.src % 16u == 0 &&
        lb_ok && w.sw * w.cs >= 64u)
        ok = try_mfma(c, dbg, n_resample, w, j);
    // (ratio 2.5 .. 3.4 and no streaming matrix-pipe plan: unaligned rows, a pre-op, a refused geometry)
    if (ok && w.s1 == S1_GENERIC && wtile_ok && 2u * w.sh >= 5u * w.plan.resized_h && 10u * w.sh < 34u * w.plan.resized_h) ok = try_wtile(c, w, j);
    if (ok && w.s1 == S1_GENERIC && stream_supported(w.cs, w.pre) && (!w.unaligned || w.cs == 3) && lb_ok && !force_generic) ok = try_stream(c, dbg, n_resample, w, j);
    // What neither fused kernel takes and no pre-op precedes: the window-tile matrix-pipe kernel (any pitch and alignment) -- every
    // resample its planner accepts.  (The first version measured equal to the tiled kernel on up-scales and the rule kept those
    // there; after the kernel's tuning it is ahead on them as well -- 1080p -> 2000x1000 1.23 vs 1.48 ms per 128, 720p -> 1600x900
    // 1.64 vs 1.97 per 256, 1080p -> 1600x900 1.02 vs 1.77 per 128, thumbnails 3.4 vs 3.55 per 8,192; profiles/r04_wtile_experiments.txt.)
    if (ok && w.s1 == S1_GENERIC && wtile_ok) ok = try_wtile(c, w, j);
    // what neither fused kernel takes (up-scales, mild down-scales, odd pitches, forced generic): the two passes through an
    // LDS tile instead of an f32 intermediate in HBM, if a tile width fits (FLGPU_NO_TILE=1 keeps the HBM form: tests, A/B)
    if (ok && w.s1 == S1_GENERIC && !dbg.on(DBG_NO_TILE)) ok = try_tile(c, w, j);
    return ok;
}

// The blur stage's tables for picture w: the window-tile kernel's where its planner takes the picture, else blur_tile_kernel's.
// false = the table arena is full.
bool plan_blur(flgpu_ctx *c, const DebugSwitches &dbg, Work &w)
{
    AxisKey k; const HostAxis *h;
    AxisKey kv; const HostAxis *hv;
    w.bwplan = nullptr; w.luma_mid = false; // (a second attempt after an arena reset plans again)
    if (!get_axis(c, w.plan.out_h, w.plan.out_h, FILTER_GAUSSIAN, w.p->blur_sigma, &kv, &hv) ||
        !get_axis(c, w.plan.out_w, w.plan.out_w, FILTER_GAUSSIAN, w.p->blur_sigma, &k, &h)) return false;
    if (use_wtile(dbg)) {
        // Blurs the window-tile matrix-pipe kernel takes: every one its planner accepts.  A grey picture on a grey frame (R == G == B
        // everywhere, alpha 255): ONE channel is filtered, if that plan is one of the single-register-set kind (the kernel's framed
        // source exists in that instantiation only) -- stage 1 leaves the unframed Luma8 picture, the kernel reads the frame's rows
        // and columns as the fill value and expands to Rgba8 in its store (Work::luma_mid).  no_luma_mid: the Rgba8 blur of the
        // framed picture instead (A/B runs and the tests that compare the two routes)
        const bool one = !dbg.on(DBG_NO_LUMA_MID) && w.plan.letterboxed && w.plan.out_c == 4u && blur_channels(w) == 1u && w.s1 != S1_NONE && w.s1 != S1_NEAREST;
        WtPlan *wp = one ? get_wtile_plan(c, kv, *hv, k, *h, 0, 0, w.plan.out_w, w.plan.out_h, 1u) : nullptr;
        if (wp && wp->arena_full) return false;
        if (wp && wp->ok && wp->nslot == 1u) { w.bwplan = wp; w.luma_mid = true; }
        else {
            wp = get_wtile_plan(c, kv, *hv, k, *h, 0, 0, w.plan.out_w, w.plan.out_h, w.plan.out_c);
            if (wp->arena_full || arena_nearly_full(c)) return false;
            if (wp->ok) w.bwplan = wp;
        }
        if (arena_nearly_full(c)) return false;
    }
    if (w.bwplan || !blur_tile_supported(h->max_taps) || !blur_tile_supported(hv->max_taps)) return true;
    const uint32_t ty = blur_band_rows(blur_channels(w));
    return cached_block(c, c->blur_plans, std::make_tuple(kv, k, ty), [&](std::vector<uint32_t> &blk) { build_blur_plan(*hv, *h, blur_tile_count(w.plan.out_w, h->max_taps), ty, blk); });
}

// The JPEG encoder's header and quantisation tables for picture w.  false = the table arena is full.
bool plan_jpeg_tables(flgpu_ctx *c, Work &w)
{
    const uint32_t q = clamp_quality(w.p->quality);
    const bool s420 = jpeg_420(*w.p); // the one byte of SOF0 that differs: a block of its own
    w.jpeg_tab = cached_block(c, c->jpeg_tables, std::make_tuple(w.plan.out_w, w.plan.out_h, q, s420), [&](std::vector<uint32_t> &blk) { build_jpeg_tables(w.plan.out_w, w.plan.out_h, q, s420, blk); });
    return w.jpeg_tab != 0;
}

// Every table the batch's kernels read, in the arena; the first pass may overflow it: reset once and retry.
int plan_tables(flgpu_ctx *c, Batch &B, hipStream_t st)
{
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool ok = true;
        size_t n_resample = 0;
        for (auto &w : B.work) n_resample += (w.plan.resampled && w.s1 != S1_NEAREST) ? 1 : 0;
        for (auto &w : B.work)
            if (w.plan.resampled && w.s1 != S1_NEAREST && !(ok = route_resample(c, B.dbg, n_resample, w))) break;
        for (auto &w : B.work)
            if (ok && w.p->blur_sigma > 0.0f) ok = plan_blur(c, B.dbg, w);
        for (auto &w : B.work)
            if (ok && w.p->front_end == FLGPU_FE_JPEG) ok = plan_jpeg_tables(c, w);
        if (ok) break;
        if (attempt == 1) return FLGPU_ERR_OOM;
        FL_HIP(c, hipStreamSynchronize(st), "arena reset sync");
        FL_HIP(c, hipDeviceSynchronize(), "arena reset sync");
        arena_reset(c);
    }
    return arena_flush(c, st);
}

// ---- launch groups and job arrays ------------------------------------------------------------------------------------------------

const size_t kMidCapFloats = (size_t)256 << 20; // 1 GiB of f32 intermediate per launch group

// Longest work items first (in a mixed batch a 4K band walks four times the rows of a 1080p one, and the hardware hands out
// workgroups in index order -- started last, the long ones would be the launch's tail), strips of a picture on one XCD.
template <class Item, class Len> void order_items(Item *first, uint32_t n, Len len)
{
    std::stable_sort(first, first + n, [&](const Item &a, const Item &b) { return len(a) > len(b); });
    xcd_interleave(first, n, len);
}

void add_resample_launch(flgpu_ctx *c, Batch &B, const ResampleKey &k, const std::vector<size_t> &pics)
{
    auto fresh = [&] {
        Launch<ResampleKey> L{k, (uint32_t)B.jobs.size(), 0, (uint32_t)(k.s1 == S1_MFMA || k.s1 == S1_WTILE ? B.mitems.size() : B.items.size())};
        L.g.cs = k.cs; L.g.pre = k.pre; L.g.letterbox = k.lb; L.g.grouped = 1;
        return L;
    };
    Launch<ResampleKey> L = fresh();
    const MfmaPlan *launch_plan = B.work[pics[0]].mplan; // S1_MFMA: the plan every picture of the launch shares, if they all do
    for (size_t idx : pics) {
        const Work &w = B.work[idx];
        Job j; fill_job(w, j);
        const size_t mid = k.s1 == S1_GENERIC ? (size_t)w.sw * w.plan.resized_h * mid_channels(w.cs, w.pre) : 0;
        if (k.s1 == S1_GENERIC && L.njobs && L.mid_floats + mid > kMidCapFloats) {
            B.s1_launches.push_back(L);
            L = fresh();
        }
        j.mid_off = (uint32_t)L.mid_floats;
        L.mid_floats += mid;
        B.mid_floats_max = std::max(B.mid_floats_max, L.mid_floats);
        L.g.max_sw = std::max(L.g.max_sw, j.sw); L.g.max_rh = std::max(L.g.max_rh, j.rh);
        L.g.max_cw = std::max(L.g.max_cw, j.cw); L.g.max_ch = std::max(L.g.max_ch, j.ch);
        L.g.max_dw = std::max(L.g.max_dw, j.dw); L.g.max_dh = std::max(L.g.max_dh, j.dh);
        const uint32_t job = (uint32_t)B.jobs.size();
        const size_t mitems_before = B.mitems.size(), items_before = B.items.size();
        if (k.s1 == S1_TILE) L.g.tile_w_min = L.g.tile_w_min ? std::min(L.g.tile_w_min, w.tile_w) : w.tile_w;
        if (k.s1 == S1_WTILE) {
            w.wplan->items_for(wtile_bands(B.dbg, *w.wplan, pics.size()), job, B.mitems);
            L.lds = std::max(L.lds, (size_t)w.wplan->lds_bytes);
        }
        if (k.s1 == S1_MFMA) {
            if (launch_plan != w.mplan) launch_plan = nullptr;
            for (MfmaItem it2 : *w.mitems) { it2.job = job; B.mitems.push_back(it2); }
            L.max_nout = std::max(L.max_nout, w.mplan->max_nout);
        }
        if (k.s1 == S1_STREAM) {
            for (StreamItem it2 : w.splan->items) { it2.job = job; B.items.push_back(it2); }
            L.lds = std::max(L.lds, w.splan->lds_bytes);
        }
        L.nitems += (uint32_t)(B.mitems.size() - mitems_before + B.items.size() - items_before);
        if (k.s1 == S1_TILE || k.s1 == S1_WTILE || k.s1 == S1_MFMA || k.s1 == S1_STREAM) {
            c->stats.resample_src_bytes += (uint64_t)j.src_bytes;
            c->stats.resample_dst_bytes += w.plan.pixel_bytes;
        }
        B.jobs.push_back(j);
        L.njobs++;
    }
    if (k.s1 == S1_MFMA && L.nitems > 1) order_items(&B.mitems[L.item_base], L.nitems, [](const MfmaItem &x) { return x.kb1 - x.kb0; });
    if (k.s1 == S1_MFMA && k.full) {
        // full-width arithmetic: persistent workgroups, each with its own list of items
        L.grid = std::max(1u, std::min(L.nitems, c->cu_count));
        L.wg_base = (uint32_t)B.mwg.size();
        std::vector<uint32_t> lists;
        assign_items(B.mitems, L.item_base, L.nitems, L.grid, const_cast<MfmaPlan *>(launch_plan), lists);
        B.mwg.insert(B.mwg.end(), lists.begin(), lists.end());
    }
    // (window-tile items: strips and bands of a picture on one XCD -- their source windows overlap, the halo then comes from that XCD's L2)
    if (k.s1 == S1_WTILE && L.nitems > 1) xcd_interleave(&B.mitems[L.item_base], L.nitems, [](const MfmaItem &) { return 1u; });
    if (k.s1 == S1_STREAM && L.nitems > 1) order_items(&B.items[L.item_base], L.nitems, [](const StreamItem &x) { return x.r1 - x.r0; });
    B.s1_launches.push_back(L);
}

void add_blur_launch(flgpu_ctx *c, Batch &B, const BlurKey &k, const std::vector<size_t> &pics)
{
    auto fresh = [&] {
        Launch<BlurKey> L{k, (uint32_t)B.jobs.size(), 0, (uint32_t)(k.wtile ? B.mitems.size() : B.items.size())};
        L.g.cs = k.c;
        return L;
    };
    Launch<BlurKey> L = fresh();
    for (size_t idx : pics) {
        const Work &w = B.work[idx];
        const flgpu_plan &pl = w.plan;
        Job j; memset(&j, 0, sizeof(j));
        j.src = w.s1_dst; j.dst = w.blur_dst; j.src_bytes = (uint32_t)pl.pixel_bytes;
        j.sw = pl.out_w; j.sh = pl.out_h; j.rw = pl.out_w; j.rh = pl.out_h; j.cw = pl.out_w; j.ch = pl.out_h;
        j.dw = pl.out_w; j.dh = pl.out_h;
        AxisKey vkey, hkey;
        j.vtab = get_axis(c, pl.out_h, pl.out_h, FILTER_GAUSSIAN, w.p->blur_sigma, &vkey, nullptr);
        j.htab = get_axis(c, pl.out_w, pl.out_w, FILTER_GAUSSIAN, w.p->blur_sigma, &hkey, nullptr);
        const uint32_t filtered = k.wtile ? pl.out_c : k.filtered;
        auto bt = c->blur_plans.find(std::make_tuple(vkey, hkey, blur_band_rows(filtered)));
        j.pad0 = bt != c->blur_plans.end() ? bt->second : 0u; // table block of the blur kernel
        if (k.wtile) {
            if (w.luma_mid) {
                // the source is stage 1's unframed Luma8 picture (rw x rh) at (cx, cy) of a virtual sw x sh frame of value `fill`
                j.rw = std::min(pl.resized_w - pl.crop_x, pl.out_w - pl.place_x); j.rh = std::min(pl.resized_h - pl.crop_y, pl.out_h - pl.place_y);
                j.cx = pl.place_x; j.cy = pl.place_y;
                j.src_bytes = j.rw * j.rh;
                j.fill = (uint32_t)w.p->fill_r * 0x01010101u;
            }
            const size_t before = B.mitems.size();
            w.bwplan->items_for(wtile_bands(B.dbg, *w.bwplan, pics.size()), (uint32_t)B.jobs.size(), B.mitems);
            L.nitems += (uint32_t)(B.mitems.size() - before);
            L.lds = std::max(L.lds, (size_t)w.bwplan->lds_bytes);
        } else {
            const size_t mid = (size_t)pl.out_w * pl.out_h * pl.out_c;
            if (L.njobs && L.mid_floats + mid > kMidCapFloats) { B.blur_launches.push_back(L); L = fresh(); }
            const AxisTable *vh = reinterpret_cast<const AxisTable *>(c->h_arena.data() + j.vtab);
            const AxisTable *hh = reinterpret_cast<const AxisTable *>(c->h_arena.data() + j.htab);
            const size_t lds = blur_lds_bytes(pl.out_w, filtered, vh->max_taps, hh->max_taps);
            L.blur_tiled = (L.njobs == 0 || L.blur_tiled) && blur_tile_supported(hh->max_taps) && blur_tile_supported(vh->max_taps) && lds <= 150 * 1024 && j.pad0;
            L.lds = std::max(L.lds, lds);
            L.blur_grid_x = std::max(L.blur_grid_x, blur_grid_x(pl.out_w, pl.out_h, hh->max_taps, filtered));
            j.mid_off = (uint32_t)L.mid_floats;
            L.mid_floats += mid;
            B.mid_floats_max = std::max(B.mid_floats_max, L.mid_floats);
            L.g.max_sw = std::max(L.g.max_sw, j.sw); L.g.max_rh = std::max(L.g.max_rh, j.rh);
            L.g.max_cw = std::max(L.g.max_cw, j.cw); L.g.max_ch = std::max(L.g.max_ch, j.ch);
        }
        B.jobs.push_back(j);
        L.njobs++;
    }
    if (k.wtile && L.nitems > 1) xcd_interleave(&B.mitems[L.item_base], L.nitems, [](const MfmaItem &) { return 1u; });
    B.blur_launches.push_back(L);
}

// Groups the pictures into launches (each group in key order) and builds the job and item arrays the kernels read.
int build_launches(flgpu_ctx *c, Batch &B)
{
    std::map<ResampleKey, std::vector<size_t>> s1_groups;
    std::map<BlurKey, std::vector<size_t>> blur_groups;
    std::vector<EncodeInput> fe_inputs; // the pictures that have a front end, in batch order
    for (size_t i = 0; i < B.n; ++i) {
        const Work &w = B.work[i];
        if (w.s1 != S1_NONE) {
            ResampleKey k{};
            k.s1 = w.s1; k.cs = w.cs; k.pre = w.pre; k.lb = w.plan.letterboxed && !w.luma_mid;
            if (w.s1 == S1_WTILE) k.nslot = w.wplan->nslot;
            else if (w.s1 == S1_MFMA) { k.ops_in_lds = w.mplan->ops_in_lds; k.wide = w.mplan->wide; k.full = w.mplan->full; k.compact = w.mplan->compact; }
            else { k.nacc = w.splan ? w.splan->nacc : 0u; k.unaligned = w.s1 == S1_STREAM && w.unaligned; }
            s1_groups[k].push_back(i);
        }
        if (w.p->blur_sigma > 0.0f && w.bwplan) blur_groups[{true, w.bwplan->nslot, 0u, w.luma_mid ? 1u : w.plan.out_c, 0u, w.luma_mid}].push_back(i);
        else if (w.p->blur_sigma > 0.0f) {
            // pictures of one launch share the workgroup width the kernel is instantiated for
            AxisKey hk; const HostAxis *hh = nullptr;
            const bool tiled = get_axis(c, w.plan.out_w, w.plan.out_w, FILTER_GAUSSIAN, w.p->blur_sigma, &hk, &hh) && hh && blur_tile_supported(hh->max_taps);
            blur_groups[{false, 0u, tiled ? blur_lanes(w.plan.out_w, hh->max_taps) : 256u, w.plan.out_c, blur_channels(w), false}].push_back(i);
        }
        if (w.p->front_end != FLGPU_FE_NONE) fe_inputs.push_back({w.blur_dst ? w.blur_dst : w.s1_dst, w.final_dst, B.dsts[i].capacity, &w.plan, w.p, w.jpeg_tab, i});
    }
    // EXIF orientation pre-pass jobs, one launch per channel count
    for (uint32_t cs = 1; cs <= 4; ++cs) {
        LaunchGeneric O{};
        O.cs = cs; O.job_base = (uint32_t)B.jobs.size();
        for (auto &w : B.work) {
            if (!w.orient || w.cs != cs) continue;
            Job j; memset(&j, 0, sizeof(j));
            j.src = w.raw_src; j.dst = const_cast<uint8_t *>(w.src);
            j.sw = w.raw_w; j.sh = w.raw_h; j.dw = w.sw; j.dh = w.sh; j.fill = w.orient;
            O.max_dw = std::max(O.max_dw, j.dw); O.max_dh = std::max(O.max_dh, j.dh);
            B.jobs.push_back(j);
            O.njobs++;
        }
        if (O.njobs) B.orient_launches.push_back(O);
    }
    for (auto &g : s1_groups) add_resample_launch(c, B, g.first, g.second);
    for (auto &g : blur_groups) add_blur_launch(c, B, g.first, g.second);
    // result words: two per image of the batch, see flgpu_ctx::last_fe
    // ... followed by the batch's device error word (fl_mfma.h FLGPU_DEVERR_*): kernels that wait on one another inside a
    // workgroup bound their waits and report an expired one here instead of delivering pixels that were never synchronised
    B.has_results = !fe_inputs.empty();
    for (auto &L : B.s1_launches) B.has_err_word |= L.k.s1 == S1_MFMA;
    encode_build_jobs(c, fe_inputs, B.enc);
    FL_HIP(c, c->d_mid.reserve(B.mid_floats_max * 4), "f32 intermediate");
    return FLGPU_OK;
}

// ---- descriptor block ------------------------------------------------------------------------------------------------------------

// The batch's descriptor block, one upload: every array a 256-byte aligned region, then the result words and the device error
// word.  f(array, pointer) is called for each region in layout order; the pointer receives the array's device address.
template <class F> void desc_regions(Batch &B, F &&f)
{
    f(B.jobs, B.d.jobs);
    f(B.items, B.d.items);
    B.enc.head_regions(f);
    f(B.mitems, B.d.mitems);
    f(B.mreqs, B.d.mreqs);
    f(B.mwg, B.d.mwg);
    B.enc.tail_regions(f);
}

// Lays the batch's arrays out in one descriptor block and sends it to the device.
int stage_descriptors(flgpu_ctx *c, Batch &B, hipStream_t st)
{
    // The matrix-pipe kernel's persistent workgroups request the first K-block of their NEXT item in the last pass of the current
    // one: what that request needs (source, pitch, last row, the strip's first byte, the first K-block), one record per item in item
    // order, so that it is ONE scalar load at that point and nothing of the next item occupies registers before (fl_mfma.h MfmaReq).
    for (auto &L : B.s1_launches) {
        if (L.k.s1 != S1_MFMA) continue;
        B.mreqs.resize(B.mitems.size());
        for (uint32_t k = L.item_base; k < L.item_base + L.nitems; ++k) {
            const MfmaItem &mi = B.mitems[k];
            const Job &j = B.jobs[mi.job];
            MfmaReq &r = B.mreqs[k];
            r.src = j.src; r.pitch = j.sw * L.k.cs; r.last_row = j.sh - 1u; r.kb0 = mi.kb0; r.kb1 = mi.kb1; r.job = mi.job;
            r.strip_off = mi.strip_off; r.vplan_off = mi.vplan_off; r.pad[0] = r.pad[1] = 0;
            r.byte0 = reinterpret_cast<const MfmaStrip *>(c->h_arena.data() + mi.strip_off)->byte0;
        }
    }
    size_t bytes = 0;
    desc_regions(B, [&](const auto &v, auto &) { bytes += align_up(v.size() * sizeof(v[0]), 256); });
    // (the result words arrive zeroed with the block: a clear of their own was two fill kernels and two engine switches between
    // one batch's last kernel and the next one's first)
    const size_t words_off = bytes, words_b = (B.has_results || B.has_err_word) ? align_up(B.n * 8 + 8, 256) : 0;
    bytes += words_b;
    if (!bytes) return FLGPU_OK;
    DescSlot *slot = B.slot = &c->slots[c->next_slot];
    c->next_slot = (c->next_slot + 1) % 4;
    if (slot->busy) { FL_HIP(c, hipEventSynchronize(slot->done), "descriptor slot wait"); slot->busy = false; }
    if (!slot->done) FL_HIP(c, hipEventCreateWithFlags(&slot->done, hipEventDisableTiming), "event");
    FL_HIP(c, slot->host.reserve(bytes), "pinned descriptors");
    FL_HIP(c, slot->dev.reserve(bytes), "device descriptors");
    char *hp = static_cast<char *>(slot->host.p), *dp = static_cast<char *>(slot->dev.p);
    if (words_b) {
        B.status_dev = reinterpret_cast<uint32_t *>(dp + words_off);
        memset(hp + words_off, 0, words_b);
        B.enc.point_results(B.status_dev);
    }
    size_t off = 0;
    desc_regions(B, [&](const auto &v, auto &dev) {
        dev = reinterpret_cast<std::remove_reference_t<decltype(dev)>>(dp + off);
        if (!v.empty()) memcpy(hp + off, v.data(), v.size() * sizeof(v[0]));
        off += align_up(v.size() * sizeof(v[0]), 256);
    });
    // While a previous batch is still running, the block goes up on the context's upload stream: the slot is free (its last
    // batch has ended, see above), so the copy runs under that batch's kernels, and this batch's first kernel follows its
    // last one without a copy engine in between.  A lone request on an idle device sends the block down its own stream (no
    // second stream, no wait: the 15 us would be 3 % of its latency).
    if (c->last_done && hipEventQuery(c->last_done) == hipErrorNotReady) {
        if (!c->up_stream) FL_HIP(c, hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking), "upload stream");
        if (!slot->uploaded) FL_HIP(c, hipEventCreateWithFlags(&slot->uploaded, hipEventDisableTiming), "event");
        FL_HIP(c, hipMemcpyAsync(slot->dev.p, hp, bytes, hipMemcpyHostToDevice, c->up_stream), "descriptor upload");
        FL_HIP(c, hipEventRecord(slot->uploaded, c->up_stream), "event record");
        // (the HOST waits the ~15 us the 130 KB take: a device-side wait on the event is a barrier packet between the previous
        // batch's last kernel and this one's first, 7 us of idle chip per batch; the host has the previous batch's 2 ms to spare)
        FL_HIP(c, hipEventSynchronize(slot->uploaded), "descriptor upload wait");
    } else {
        FL_HIP(c, hipMemcpyAsync(slot->dev.p, hp, bytes, hipMemcpyHostToDevice, st), "descriptor upload");
    }
    return FLGPU_OK;
}

// ---- launches --------------------------------------------------------------------------------------------------------------------

// Enqueues the batch's kernels in their order -- orientation, stage 1, blur, planar front ends, JPEG, PNG, lossless WebP, lossy WebP --, then the
// plain copies of the requests that change nothing, and records the batch's events.
int enqueue_launches(flgpu_ctx *c, Batch &B, hipStream_t st)
{
    for (auto &g : B.orient_launches) {
        g.jobs = B.d.jobs;
        FL_HIP(c, launch_orient(g, st), "orientation kernel");
    }
    for (auto &L : B.s1_launches) {
        const ResampleKey &k = L.k;
        L.g.jobs = B.d.jobs; L.g.arena = c->d_arena; L.g.mid = static_cast<float *>(c->d_mid.p);
        L.g.job_base = L.job_base; L.g.njobs = L.njobs;
        L.g.no_place4 = B.dbg.on(DBG_NO_PLACE4) ? 1u : 0u;
        L.g.nearest = k.s1 == S1_NEAREST ? 1u : 0u;
        // (the matrix-pipe and streaming kernels paint the letterbox frame themselves)
        if (k.lb && (k.s1 == S1_TILE || k.s1 == S1_WTILE || k.s1 == S1_GENERIC)) FL_HIP(c, launch_place(L.g, true, st), "border fill");
        // the resample kernels proper are timed (ProfileScope kind 0), the placements and border fills are not
        const bool resample = k.s1 == S1_TILE || k.s1 == S1_WTILE || k.s1 == S1_MFMA || k.s1 == S1_STREAM;
        std::optional<ProfileScope> ps;
        if (resample) ps.emplace(c, st, 0);
        LaunchWtile wt{};
        LaunchMfma m{};
        LaunchStream s{};
        switch (k.s1) {
        case S1_NEAREST:
            FL_HIP(c, launch_place(L.g, false, st), "nearest kernel");
            break;
        case S1_PLACE:
            FL_HIP(c, launch_place(L.g, false, st), "place kernel");
            break;
        case S1_TILE:
            FL_HIP(c, launch_tile_resample(L.g, st), "tiled two-pass resample kernel");
            break;
        case S1_WTILE:
            wt.jobs = B.d.jobs; wt.items = reinterpret_cast<const WtItem *>(B.d.mitems + L.item_base); wt.arena = c->d_arena; wt.nitems = L.nitems;
            wt.nslot = k.nslot; wt.nkmax = kWtOperandRegs / wt.nslot; wt.letterbox = k.lb; wt.lds_bytes = (uint32_t)L.lds; wt.invert = k.pre == PRE_INVERT;
            FL_HIP(c, launch_wtile(wt, st), "window-tile matrix-pipe kernel");
            break;
        case S1_GENERIC:
            FL_HIP(c, launch_vpass_generic(L.g, st), "generic vertical pass");
            FL_HIP(c, launch_hpass_generic(L.g, st), "generic horizontal pass");
            break;
        case S1_MFMA:
            m.jobs = B.d.jobs; m.items = B.d.mitems + L.item_base; m.reqs = B.d.mreqs + L.item_base; m.arena = c->d_arena; m.nitems = L.nitems;
            m.grid = L.grid; m.wg_lists = L.grid ? B.d.mwg + L.wg_base : nullptr;
            m.cs = k.cs; m.letterbox = k.lb; m.ops_in_lds = k.ops_in_lds; m.wide = k.wide; m.full = k.full; m.compact = k.compact; m.max_nout = L.max_nout;
            m.spin_limit = (uint32_t)std::max<int64_t>(0, B.dbg.get(DBG_MFMA_SPIN_LIMIT)); // tests: 0 = every bounded wait expires
            m.err_word = B.status_dev + 2 * B.n;
            FL_HIP(c, launch_mfma(m, st), "matrix-pipe resample kernel");
            break;
        case S1_STREAM:
            s.jobs = B.d.jobs; s.items = B.d.items + L.item_base; s.arena = c->d_arena; s.nitems = L.nitems;
            s.cs = k.cs; s.pre = k.pre; s.letterbox = k.lb; s.lds_bytes = L.lds; s.nacc = k.nacc; s.unaligned = k.unaligned;
            FL_HIP(c, launch_stream(s, st), "streaming resample kernel");
            break;
        case S1_NONE:
            break;
        }
        c->stats.resample_launches += resample;
        c->stats.generic_launches += k.s1 == S1_TILE || k.s1 == S1_GENERIC; // (S1_TILE: the two-pass generic resample, LDS form)
        c->stats.mfma_launches += k.s1 == S1_WTILE || k.s1 == S1_MFMA;
        c->stats.wtile_launches += k.s1 == S1_WTILE;
    }
    for (auto &L : B.blur_launches) {
        L.g.jobs = B.d.jobs; L.g.arena = c->d_arena; L.g.mid = static_cast<float *>(c->d_mid.p);
        L.g.job_base = L.job_base; L.g.njobs = L.njobs;
        ProfileScope ps(c, st, 1);
        if (L.k.wtile) {
            LaunchWtile m{};
            m.jobs = B.d.jobs; m.items = reinterpret_cast<const WtItem *>(B.d.mitems + L.item_base); m.arena = c->d_arena; m.nitems = L.nitems;
            m.nslot = L.k.nslot; m.nkmax = kWtOperandRegs / m.nslot; m.letterbox = L.k.luma_mid; m.framed = L.k.luma_mid; m.lds_bytes = (uint32_t)L.lds; m.half_waves = L.k.c == 1u; // (one-channel pictures: little work per step, two 4-wave workgroups per CU hide each other's barriers; Rgba8 blurs measured 2 % slower that way)
            FL_HIP(c, launch_wtile(m, st), "window-tile matrix-pipe kernel (blur)");
            c->stats.mfma_launches++;
            c->stats.wtile_launches++;
            c->blur_wtile_launches++;
        } else if (L.blur_tiled && !B.dbg.on(DBG_FORCE_GENERIC)) {
            L.g.pre = L.k.filtered; // channels to filter, see blur_tile_kernel
            L.g.blur_lanes = L.k.lanes;
            FL_HIP(c, launch_blur_tile(L.g, L.blur_grid_x, L.lds, st), "blur kernel");
            c->blur_tile_launches++;
        } else {
            FL_HIP(c, launch_vpass_generic(L.g, st), "blur vertical pass");
            FL_HIP(c, launch_hpass_generic(L.g, st), "blur horizontal pass");
            c->blur_generic_launches++;
        }
        c->stats.blur_launches++;
    }
    if (int rc = encode_enqueue(c, B.enc, st)) return rc;
    // plain copies for requests that change nothing
    for (const Work &w : B.work)
        if (w.s1 == S1_NONE && !(w.p->blur_sigma > 0.0f) && w.p->front_end == FLGPU_FE_NONE)
            FL_HIP(c, hipMemcpyAsync(w.final_dst, w.src, w.plan.pixel_bytes, hipMemcpyDeviceToDevice, st), "copy");
    if (B.slot) { FL_HIP(c, hipEventRecord(B.slot->done, st), "event record"); B.slot->busy = true; }
    if (!c->last_done) FL_HIP(c, hipEventCreateWithFlags(&c->last_done, hipEventDisableTiming), "event");
    FL_HIP(c, hipEventRecord(c->last_done, st), "event record");
    c->last_stream = st;
    return FLGPU_OK;
}

} // namespace

namespace fl {

int run_batch_device(flgpu_ctx *c, size_t n, const flgpu_image *srcs, const flgpu_params *ps, bool same_params,
                     flgpu_image *dsts, hipStream_t st)
{
    if (n == 0) return FLGPU_OK;
    if (!srcs || !ps || !dsts) return FLGPU_ERR_INVALID_ARG;
    FL_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    if (!st) st = c->stream;
    if (c->last_stream && c->last_stream != st && c->last_done) FL_HIP(c, hipStreamWaitEvent(st, c->last_done, 0), "stream handoff");

    RoctxRange range_batch("flgpu batch");
    Batch B(c, n, dsts);
    {
        RoctxRange range_plan("flgpu plan + tables");
        if (int rc = plan_pictures(B, srcs, ps, same_params)) return rc;
        if (int rc = reserve_scratch(c, B, st)) return rc;
        if (int rc = plan_tables(c, B, st)) return rc;
        if (int rc = build_launches(c, B)) return rc;
        if (int rc = stage_descriptors(c, B, st)) return rc;
    }
    RoctxRange range_launch("flgpu launches");
    if (int rc = enqueue_launches(c, B, st)) return rc;
    // what the caller gets back at once, and what collect_results reads later
    for (size_t i = 0; i < n; ++i) {
        const flgpu_plan &pl = B.work[i].plan;
        dsts[i].width = pl.out_w; dsts[i].height = pl.out_h; dsts[i].channels = pl.out_c;
        encode_dst_header(B.work[i].p->front_end, pl, dsts[i]);
    }
    c->last_n = n;
    c->last_status_dev = B.status_dev;
    c->last_has_results = B.has_results;
    c->last_has_err_word = B.has_err_word;
    c->last_fe.resize(n);
    for (size_t i = 0; i < n; ++i) c->last_fe[i] = B.work[i].p->front_end;
    c->stats.images += n;
    c->stats.batches++;
    return FLGPU_OK;
}

// Reads the result words of the batch that was just enqueued on `st` (synchronises) and completes dsts[]:
// the alpha flag of the WebP front end, the length of an encoded stream.
int collect_results(flgpu_ctx *c, size_t n, flgpu_image *dsts, hipStream_t st)
{
    if ((!c->last_has_results && !c->last_has_err_word) || n != c->last_n) { FL_HIP(c, hipStreamSynchronize(st), "batch sync"); return FLGPU_OK; }
    FL_HIP(c, c->h_results.reserve(n * 8 + 8), "pinned result words");
    if (c->last_has_results) FL_HIP(c, hipMemcpyAsync(c->h_results.p, c->last_status_dev, n * 8 + 8, hipMemcpyDeviceToHost, st), "result words D2H");
    else FL_HIP(c, hipMemcpyAsync(static_cast<char *>(c->h_results.p) + n * 8, reinterpret_cast<char *>(c->last_status_dev) + n * 8, 8, hipMemcpyDeviceToHost, st), "error word D2H");
    FL_HIP(c, hipStreamSynchronize(st), "batch sync");
    const uint32_t *r = static_cast<const uint32_t *>(c->h_results.p);
    if (c->last_has_err_word && r[2 * n]) {
        c->set_error((r[2 * n] & FLGPU_DEVERR_MFMA_WAIT) ? "matrix-pipe resample kernel: a bounded wait on an LDS hand-off expired; the batch's pixels are not valid"
                                                         : "device error word set");
        return FLGPU_ERR_DEVICE;
    }
    if (!c->last_has_results) return FLGPU_OK;
    int rc = FLGPU_OK;
    for (size_t i = 0; i < n; ++i)
        if (int e = encode_collect(c, c->last_fe[i], r[2 * i], r[2 * i + 1], dsts[i])) rc = e;
    return rc;
}

// Host-memory batch: stage in, run, stage out, wait.
int run_batch_host(flgpu_ctx *c, size_t n, const flgpu_image *srcs, const flgpu_params *ps, flgpu_image *dsts)
{
    if (n == 0) return FLGPU_OK;
    if (!srcs || !ps || !dsts) return FLGPU_ERR_INVALID_ARG;
    FL_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    std::vector<flgpu_image> dsrc(n), ddst(n);
    std::vector<flgpu_plan> plans(n);
    // file sources (JPEG, PNG, lossless WebP): the serial half -- parsing, entropy decoding, inflate -- runs here, on the host; what is
    // staged is the blob (fl_source.h)
    std::vector<std::vector<uint8_t>> blobs(n);
    std::vector<StagedSource> staged(n);
    std::vector<const StagedSource *> staged_of(n);
    size_t in_b = 0, out_b = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!srcs[i].data || !dsts[i].data) return FLGPU_ERR_INVALID_ARG;
        int rc = flgpu_plan_output(&ps[i], srcs[i].width, srcs[i].height, srcs[i].channels, &plans[i]);
        if (rc) return rc;
        SourceProbe probe;
        rc = source_probe(c, &srcs[i], probe);
        if (rc) return rc;
        uint64_t sb = probe.capacity;
        if (probe.kind != SRC_PIXELS) {
            blobs[i].resize(probe.capacity);
            rc = source_stage(c, &srcs[i], probe, blobs[i].data(), blobs[i].size(), staged[i]);
            if (rc) return rc;
            sb = staged[i].used;
        }
        staged_of[i] = &staged[i];
        if (dsts[i].capacity < plans[i].out_bytes && !fe_encoded(ps[i].front_end)) return FLGPU_ERR_BUFFER_TOO_SMALL;
        dsrc[i] = srcs[i]; ddst[i] = dsts[i];
        dsrc[i].data = reinterpret_cast<uint8_t *>(in_b); dsrc[i].capacity = sb; in_b += align_up(sb, 256);
        const uint64_t ob = plans[i].max_out_bytes; // JPEG: the format's worst case, so the device side never overflows
        ddst[i].data = reinterpret_cast<uint8_t *>(out_b); ddst[i].capacity = ob; out_b += align_up(ob, 256);
    }
    FL_HIP(c, c->d_in.reserve(in_b), "device input staging");
    FL_HIP(c, c->d_out.reserve(out_b), "device output staging");
    FL_HIP(c, c->h_stage_in.reserve(in_b), "pinned input staging");
    FL_HIP(c, c->h_stage_out.reserve(out_b), "pinned output staging");
    hipStream_t st = c->stream;
    for (size_t i = 0; i < n; ++i) {
        const size_t off = reinterpret_cast<size_t>(dsrc[i].data);
        memcpy(static_cast<char *>(c->h_stage_in.p) + off, staged[i].kind != SRC_PIXELS ? blobs[i].data() : srcs[i].data, dsrc[i].capacity);
        dsrc[i].data = static_cast<uint8_t *>(c->d_in.p) + off;
        ddst[i].data = static_cast<uint8_t *>(c->d_out.p) + reinterpret_cast<size_t>(ddst[i].data);
    }
    FL_HIP(c, hipMemcpyAsync(c->d_in.p, c->h_stage_in.p, in_b, hipMemcpyHostToDevice, st), "H2D");
    { int drc = decode_sources(c, n, dsrc.data(), staged_of.data(), st); if (drc) return drc; }
    int rc = run_batch_device(c, n, dsrc.data(), ps, false, ddst.data(), st);
    if (rc) return rc;
    FL_HIP(c, hipMemcpyAsync(c->h_stage_out.p, c->d_out.p, out_b, hipMemcpyDeviceToHost, st), "D2H");
    rc = collect_results(c, n, ddst.data(), st);
    {   // pictures the device entropy decoder gave up on (states that did not settle, an invalid code word): the whole batch once
        // more with the host decoder -- which either decodes them or says what is wrong with the file
        std::vector<uint8_t> bad;
        const int nbad = entropy_failures(c, n, bad, st);
        if (nbad < 0) return -nbad;
        if (nbad > 0 && !ForceHostHuffman::active()) {
            ForceHostHuffman force;
            return run_batch_host(c, n, srcs, ps, dsts);
        }
    }
    for (size_t i = 0; i < n; ++i) {
        const size_t off = static_cast<uint8_t *>(ddst[i].data) - static_cast<uint8_t *>(c->d_out.p);
        if (ddst[i].bytes > dsts[i].capacity) { // only now is the length of an encoded stream known
            c->set_error("encoded stream does not fit the destination");
            if (rc == FLGPU_OK) rc = FLGPU_ERR_BUFFER_TOO_SMALL;
            dsts[i].bytes = 0; dsts[i].flags = ddst[i].flags;
            continue;
        }
        memcpy(dsts[i].data, static_cast<char *>(c->h_stage_out.p) + off, std::min<uint64_t>(ddst[i].bytes, ddst[i].capacity));
        dsts[i].width = ddst[i].width; dsts[i].height = ddst[i].height; dsts[i].channels = ddst[i].channels; dsts[i].flags = ddst[i].flags;
        dsts[i].bytes = ddst[i].bytes;
    }
    return rc;
}

} // namespace fl

// ---- diagnostics -----------------------------------------------------------------------------------------------------------------
extern "C" int flgpu_debug_assign_items(uint32_t pictures, uint32_t strips, uint32_t tiles, uint32_t workgroups, uint32_t capacity, uint32_t *job_of, uint32_t *strip_of,
                                        uint32_t *tile0_of, uint32_t *tile1_of, uint32_t *lists, uint32_t *nitems)
{
    if (!pictures || !strips || !tiles || !workgroups || !job_of || !strip_of || !tile0_of || !tile1_of || !lists || !nitems) return FLGPU_ERR_INVALID_ARG;
    MfmaPlan plan;
    plan.ok = true; plan.vplan_off = 7u;
    for (uint32_t s = 0; s < strips; ++s) plan.strip_offs.push_back(1000u + s);
    for (uint32_t t = 0; t < tiles; ++t) plan.tiles.push_back({3u * t, 3u * t + 4u}); // (a tile needs five K-blocks, a new one ends every third)
    std::vector<MfmaItem> v;
    for (uint32_t p = 0; p < pictures; ++p)
        for (MfmaItem m : plan.items_for(1)) { m.job = p; v.push_back(m); }
    uint32_t n = (uint32_t)v.size();
    order_items(v.data(), n, [](const MfmaItem &x) { return x.kb1 - x.kb0; });
    const uint32_t G = std::max(1u, std::min(n, workgroups));
    std::vector<uint32_t> l;
    assign_items(v, 0, n, G, &plan, l);
    *nitems = n;
    if (n > capacity) return FLGPU_ERR_BUFFER_TOO_SMALL;
    for (uint32_t k = 0; k < n; ++k) { job_of[k] = v[k].job; strip_of[k] = v[k].strip_off - 1000u; tile0_of[k] = v[k].tile0; tile1_of[k] = v[k].tile1; }
    for (uint32_t k = 0; k < 2u * G; ++k) lists[k] = l[k];
    return FLGPU_OK;
}
