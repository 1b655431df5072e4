// fl_source.cpp -- JPEG / PNG / lossless WebP / lossy WebP files as sources of a batch (fl_source.h): what a file may make the library reserve, the host
// half on the thread that stages the file, and the decode launches in front of run_batch_device.
#include <stdio.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "fl_context.h"
#include "fl_vp8_core.h"

namespace fl {

// What a JPEG file's own header may make this library allocate is decided here, before anything is allocated: the header
// must describe the picture the caller announced, the decoded picture must respect the limit the reference's decoder runs
// under (image::Limits::default(): max_alloc 512 MiB -- ImageReader rejects larger pictures, handler.rs:205-220), and the file
// must be long enough to hold that many blocks at all (a block costs at least a DC and an end-of-block code, two bits), so a
// few hundred hostile bytes cannot reserve gigabytes of pinned or host memory.
static int jpeg_source_precheck(flgpu_ctx *c, const flgpu_image *src, const JpegInfo &info)
{
    if (info.width != src->width || info.height != src->height) {
        c->set_error("FLGPU_IMG_JPEG_SOURCE: width / height do not match the file (see flgpu_jpeg_info_of)");
        return FLGPU_ERR_INVALID_ARG;
    }
    const uint64_t decoded = (uint64_t)info.width * info.height * std::max<uint32_t>(info.components, 1u);
    if (decoded > (512ull << 20)) {
        c->set_error("JPEG source: the decoded picture exceeds the 512 MiB the reference's decoder allows (image::Limits)");
        return FLGPU_ERR_UNSUPPORTED;
    }
    const uint64_t blocks = ((uint64_t)(info.width + 7u) / 8u) * ((info.height + 7u) / 8u) * std::max<uint32_t>(info.components, 1u);
    // How short can a file be for that many blocks?  Sequential coding spends at least a DC and an end-of-block code on a block
    // (two bits); a progressive file needs only its first DC scan (one bit per block), every later scan may end 32767 blocks
    // with one end-of-band run.  Below that the header lies about the picture.  (Chroma sub-sampling only lowers the count:
    // the test is repeated on the smallest count the frame could mean.)
    const uint64_t bits_per_block = info.progressive ? 1u : 2u;
    const uint64_t fewest = ((uint64_t)(info.width + 15u) / 16u) * ((info.height + 15u) / 16u) * 3u;
    if (std::min(blocks, std::max<uint64_t>(fewest, 1u)) * bits_per_block > 8ull * src->capacity + 512ull) {
        c->set_error("malformed JPEG stream: shorter than its header's picture needs");
        return FLGPU_ERR_INVALID_ARG;
    }
    // multi-scan files are assembled in a full coefficient array first (128 bytes per block, fl_jpeghuff.cpp): it counts
    // against the same 512 MiB
    if (info.progressive && blocks * 128ull > (512ull << 20)) {
        c->set_error("JPEG source: the coefficient array of this progressive picture exceeds 512 MiB");
        return FLGPU_ERR_UNSUPPORTED;
    }
    return FLGPU_OK;
}

thread_local bool tl_force_host_huffman = false;

// Whether JPEG sources are entropy-decoded on the device where the file allows it.
// 0 = this file is Huffman-decoded on the host, 1 = on the device if the caller has no idle CPU for it, 2 = on the device in any case.
// Switches (flgpu_debug_set; tests and A/B runs): host_huffman = never on the device, device_huffman_always = always,
// device_huffman_min_bytes = files below it are decoded faster by the thread that holds them than by six kernel launches.
int device_huffman_policy(const flgpu_ctx *c, uint64_t file_bytes)
{
    const DebugSwitches &dbg = *c->dbg;
    if (tl_force_host_huffman || dbg.on(DBG_HOST_HUFFMAN)) return 0;
    if (file_bytes < (uint64_t)std::max<int64_t>(0, dbg.get(DBG_DEVICE_HUFFMAN_MIN_BYTES))) return 0;
    return dbg.on(DBG_DEVICE_HUFFMAN_ALWAYS) ? 2 : 1;
}

// The buffer of a JPEG source holds the coefficient blob (sized by the picture's blocks) or, for the device entropy decoder, the staged file:
// four code tables and the segment itself -- more than the blob of a small picture or of a dense one.  Sized by the blob alone, whether the
// device decoded such a file depended on how far the allocator happened to round the buffer up (tests/test_jpeg_layouts.py).
static size_t jpeg_source_capacity(const flgpu_ctx *c, const flgpu_image *src, const JpegInfo &info)
{
    const size_t blob = jpeg_blob_bound(info);
    return device_huffman_policy(c, src->capacity) != 0 ? std::max(blob, jpeg_stage_bound((size_t)src->capacity)) : blob;
}

static int jpeg_source_to_blob(flgpu_ctx *c, const flgpu_image *src, uint8_t *blob, size_t cap, JpegBlobHeader *hdr, size_t *used, bool host_huffman)
{
    int rc = -2;
    // files the device entropy decoder takes (sequential, one interleaved scan) are only STAGED here: header,
    // code tables, the segment without its stuffing -- tens of microseconds instead of ~2 ms of Huffman decoding on this thread
    if (!host_huffman && device_huffman_policy(c, src->capacity) != 0) rc = jpeg_entropy_stage(src->data, (size_t)src->capacity, blob, cap, used);
    if (rc == -2) rc = jpeg_entropy_decode(src->data, (size_t)src->capacity, blob, cap, used);
    if (rc == -2) { c->set_error("JPEG stream not covered by the device decoder (arithmetic coding, 12-bit samples, lossless or hierarchical processes)"); return FLGPU_ERR_UNSUPPORTED; }
    if (rc) { c->set_error("malformed JPEG stream"); return FLGPU_ERR_INVALID_ARG; }
    memcpy(hdr, blob, sizeof(*hdr));
    if (hdr->width != src->width || hdr->height != src->height || (hdr->nc == 4 ? 3u : hdr->nc) != src->channels) {
        c->set_error("FLGPU_IMG_JPEG_SOURCE: width / height / channels do not match the file (see flgpu_jpeg_info_of)");
        return FLGPU_ERR_INVALID_ARG;
    }
    return FLGPU_OK;
}

static int decode_jpeg_sources(flgpu_ctx *c, size_t n, flgpu_image *dsrc, const StagedSource *const *srcs, hipStream_t st)
{
    size_t nj = 0, scratch = 0;
    for (size_t i = 0; i < n; ++i) {
        if (srcs[i]->kind != SRC_JPEG) continue;
        const JpegBlobHeader *H = &srcs[i]->jpeg;
        ++nj;
        const size_t px = (size_t)H->width * H->height;
        scratch += align_up(H->plane_bytes, 256) + align_up(px * H->nc + 64, 256);
        if (H->nc == 4) scratch += align_up((px + 3) / 4 * 12, 256); // the Rgb8 picture after the CMYK table
    }
    c->last_jh_slot.assign(n, -1);
    c->last_jh_n = 0;
    if (!nj) return FLGPU_OK;
    { const int brc = clut_batch_begin(c); if (brc) return brc; } // tables selected below stay resident until the batch's kernels are launched
    // ---- staged sources (kJhMagic): the entropy-coded segment is decoded on the device first, into a blob of its own ----
    {
        size_t njh = 0, bytes = 0, nitems = 0;
        for (size_t i = 0; i < n; ++i) {
            const JpegBlobHeader *H = &srcs[i]->jpeg;
            if (srcs[i]->kind != SRC_JPEG || H->magic != kJhMagic) continue;
            ++njh;
        }
        if (njh) {
            // per picture: the blob, states (nsub + 1 x 8), counts and prefix (nsub x 16 each)
            std::vector<JhJob> jobs;
            std::vector<JhItem> items;
            std::vector<size_t> blob_off, scratch_off;
            uint32_t max_blocks = 0;
            for (size_t i = 0; i < n; ++i) {
                const JpegBlobHeader *H = &srcs[i]->jpeg;
                if (srcs[i]->kind != SRC_JPEG || H->magic != kJhMagic) continue;
                const JpegHuffStage &S = srcs[i]->stage;
                const uint32_t nsub = jh_subsequences(S);
                blob_off.push_back(bytes); bytes += align_up(jh_blob_bytes(*H), 256);
                scratch_off.push_back(bytes); bytes += align_up((size_t)(nsub + 2) * 8 + (size_t)nsub * 8 + (size_t)nsub * 32 + 32, 256);
                JhJob j{};
                j.stage = static_cast<const uint8_t *>(dsrc[i].data);
                j.nsub = nsub;
                for (uint32_t f = 0; f < nsub; f += kJhSubsPerItem) items.push_back({(uint32_t)jobs.size(), f});
                c->last_jh_slot[i] = (int32_t)jobs.size();
                jobs.push_back(j);
                max_blocks = std::max(max_blocks, H->nblocks);
            }
            nitems = items.size();
            FL_HIP(c, c->d_jh.reserve(bytes), "device entropy decode scratch");
            FL_HIP(c, c->d_jherr.reserve(njh * 4), "device entropy decode error words");
            FL_HIP(c, c->h_jherr.reserve(njh * 4), "device entropy decode error words");
            const size_t jobs_b = align_up(njh * sizeof(JhJob), 256);
            FL_HIP(c, c->h_jhjobs.reserve(jobs_b + nitems * sizeof(JhItem)), "device entropy decode descriptors");
            FL_HIP(c, c->d_jhjobs.reserve(jobs_b + nitems * sizeof(JhItem)), "device entropy decode descriptors");
            size_t k = 0;
            for (size_t i = 0; i < n; ++i) {
                if (c->last_jh_slot[i] < 0) continue;
                JhJob &j = jobs[k];
                uint8_t *base = static_cast<uint8_t *>(c->d_jh.p);
                j.blob = base + blob_off[k];
                j.states = reinterpret_cast<uint64_t *>(base + scratch_off[k]);
                j.used = j.states + (j.nsub + 2u);
                j.counts = reinterpret_cast<int32_t *>(base + scratch_off[k] + align_up((size_t)(2u * j.nsub + 2u) * 8, 16));
                j.prefix = j.counts + (size_t)j.nsub * 4;
                j.err = static_cast<uint32_t *>(c->d_jherr.p) + k;
                dsrc[i].data = j.blob; // what the IDCT kernel reads from here on
                c->stats.jpeg_device_huffman++;
                ++k;
            }
            memcpy(c->h_jhjobs.p, jobs.data(), njh * sizeof(JhJob));
            memcpy(static_cast<char *>(c->h_jhjobs.p) + jobs_b, items.data(), nitems * sizeof(JhItem));
            FL_HIP(c, hipMemcpyAsync(c->d_jhjobs.p, c->h_jhjobs.p, jobs_b + nitems * sizeof(JhItem), hipMemcpyHostToDevice, st), "device entropy decode descriptors");
            FL_HIP(c, launch_jpeg_huff(static_cast<const JhJob *>(c->d_jhjobs.p), jobs.data(), (uint32_t)njh,
                                       reinterpret_cast<const JhItem *>(static_cast<const char *>(c->d_jhjobs.p) + jobs_b), (uint32_t)nitems, max_blocks, st),
                   "device entropy decode kernels");
            c->last_jh_n = (uint32_t)njh;
        }
    }
    FL_HIP(c, c->d_dec.reserve(scratch), "JPEG decode scratch");
    FL_HIP(c, c->h_decjobs.reserve(nj * sizeof(JpegDecJob)), "JPEG decode descriptors");
    FL_HIP(c, c->d_decjobs.reserve(nj * sizeof(JpegDecJob)), "JPEG decode descriptors");
    JpegDecJob *jobs = static_cast<JpegDecJob *>(c->h_decjobs.p);
    size_t off = 0, k = 0;
    uint32_t max_blocks = 0, max_w = 0, max_h = 0;
    struct Cmyk { const void *raw; void *rgb; const void *clut; uint64_t px; bool ycck; };
    std::vector<Cmyk> cmyk;
    for (size_t i = 0; i < n; ++i) {
        if (srcs[i]->kind != SRC_JPEG) continue;
        const JpegBlobHeader &H = srcs[i]->jpeg;
        const size_t px = (size_t)H.width * H.height;
        JpegDecJob &j = jobs[k++];
        j.blob = dsrc[i].data;
        j.planes = static_cast<uint8_t *>(c->d_dec.p) + off; off += align_up(H.plane_bytes, 256);
        j.dst = static_cast<uint8_t *>(c->d_dec.p) + off; off += align_up(px * H.nc + 64, 256);
        jpeg_color_job(H, j);
        max_blocks = std::max(max_blocks, H.nblocks); max_w = std::max(max_w, H.width); max_h = std::max(max_h, H.height);
        c->stats.jpeg_sources++;
        c->stats.jpeg_upload_bytes += H.total_bytes;
        uint8_t *pixels = j.dst;
        uint32_t channels = H.nc;
        if (H.nc == 4) {
            // convert_jpeg_color_if_needed (handler.rs:398-466): raw CMYK / YCCK samples -> (YCCK loop) -> the profile's table
            const void *clut = nullptr;
            const int rc = select_clut(c, srcs[i]->icc.empty() ? nullptr : srcs[i]->icc.data(), srcs[i]->icc.size(), &clut);
            if (rc) return rc;
            uint8_t *rgb = static_cast<uint8_t *>(c->d_dec.p) + off; off += align_up((px + 3) / 4 * 12, 256);
            cmyk.push_back({j.dst, rgb, clut, px, H.adobe_transform == 3u});
            pixels = rgb;
            channels = 3;
            c->stats.cmyk_pixels += px;
        }
        dsrc[i].data = pixels;
        dsrc[i].channels = channels;
        dsrc[i].capacity = (uint64_t)px * channels;
        dsrc[i].flags &= ~FLGPU_IMG_JPEG_SOURCE;
    }
    FL_HIP(c, hipMemcpyAsync(c->d_decjobs.p, jobs, nj * sizeof(JpegDecJob), hipMemcpyHostToDevice, st), "JPEG decode descriptors");
    for (size_t base = 0; base < nj; base += 32768) { // grid.y / .z limits
        const uint32_t cnt = (uint32_t)std::min<size_t>(32768, nj - base);
        FL_HIP(c, launch_jpeg_decode(static_cast<const JpegDecJob *>(c->d_decjobs.p) + base, cnt, max_blocks, max_w, max_h, st), "JPEG decode kernels");
    }
    for (const Cmyk &m : cmyk) FL_HIP(c, launch_cmyk_clut(m.raw, m.rgb, m.clut, kCmykGrid, m.px, m.ycck, st), "CMYK kernel");
    return FLGPU_OK;
}

// ---- the header of a file, whatever its format ---------------------------------------------------------------------------------------

// the picture of a WebP file is a `VP8 ` chunk (the first chunk, or the first image chunk behind VP8X)
static bool webp_is_lossy(const uint8_t *d, uint64_t n)
{
    if (!d || n < 20 || memcmp(d, "RIFF", 4) || memcmp(d + 8, "WEBP", 4)) return false;
    for (uint64_t pos = 12; n - pos >= 8;) {
        if (!memcmp(d + pos, "VP8 ", 4)) return true;
        if (!memcmp(d + pos, "VP8L", 4) || !memcmp(d + pos, "ANMF", 4)) return false;
        const uint64_t len = (uint64_t)d[pos + 4] | (uint64_t)d[pos + 5] << 8 | (uint64_t)d[pos + 6] << 16 | (uint64_t)d[pos + 7] << 24;
        if (len > n - pos - 8) return false;
        pos += 8u + len + (len & 1u);
        if (pos > n) return false;
    }
    return false;
}

// the orientation ImageDecoder::orientation() reports for a WebP, lossless or lossy: from the EXIF chunk, whose payload usually starts at the
// TIFF header, without the "Exif\0\0" a JPEG APP1 segment has; both forms are taken.  0 = no tag.
static uint32_t webp_orientation(const uint8_t *file, size_t exif_off, size_t exif_len)
{
    if (!exif_len) return 0;
    const uint8_t *p = file + exif_off;
    size_t n = exif_len;
    if (n >= 6 && !memcmp(p, "Exif\0\0", 6)) { p += 6; n -= 6; }
    return (uint32_t)tiff_orientation(p, n);
}

int file_head(SourceKind kind, const uint8_t *file, size_t n, uint32_t opts, SourceProbe &out)
{
    const bool full = (opts & HEAD_FULL) != 0, adam7 = (opts & HEAD_ADAM7) != 0, inflate = (opts & HEAD_INFLATE) != 0;
    if (kind == SRC_WEBP && (opts & HEAD_SNIFF) && webp_is_lossy(file, n)) kind = SRC_VP8;
    out.kind = kind;
    FileHead &h = out.head;
    h = FileHead();
    auto fill = [&h](const auto &I, uint32_t channels, uint32_t flags, int input_format, uint32_t orientation) {
        h.width = I.width; h.height = I.height; h.supported = I.supported;
        h.channels = channels; h.flags = flags; h.input_format = input_format; h.orientation = orientation;
    };
    switch (kind) {
    case SRC_JPEG: // (announces 1 or 3 channels whether supported or not: plan_file plans it before it refuses it)
        if (jpeg_parse_info(file, n, out.jpeg) != 0) return FLGPU_ERR_PARSE;
        fill(out.jpeg, out.jpeg.components == 1 ? 1u : 3u, FLGPU_IMG_JPEG_SOURCE, FLGPU_IN_JPEG, out.jpeg.exif_orientation);
        break;
    case SRC_PNG: // (the PNG decoder reports no orientation, handler.rs:206)
        if (png_parse_info(file, n, out.png, full, adam7) != 0) return FLGPU_ERR_PARSE;
        fill(out.png, out.png.channels, FLGPU_IMG_PNG_SOURCE | (adam7 ? FLGPU_IMG_PNG_ADAM7 : 0u) | (inflate ? FLGPU_IMG_PNG_INFLATE : 0u), FLGPU_IN_PNG, 0);
        break;
    case SRC_WEBP:
        if (webp_parse_info(file, n, out.webp, full) != 0) return FLGPU_ERR_PARSE;
        fill(out.webp, out.webp.channels, FLGPU_IMG_WEBP_SOURCE, FLGPU_IN_WEBP, webp_orientation(file, out.webp.exif_off, out.webp.exif_len));
        break;
    case SRC_VP8:
        if (vp8_parse_info(file, n, out.vp8, full) != 0) return FLGPU_ERR_PARSE;
        fill(out.vp8, out.vp8.channels, FLGPU_IMG_VP8_SOURCE, FLGPU_IN_WEBP, webp_orientation(file, out.vp8.exif_off, out.vp8.exif_len));
        break;
    case SRC_PIXELS: return FLGPU_ERR_INVALID_ARG;
    }
    return FLGPU_OK;
}

// A PNG / WebP file as a source: the container walk has bounded what the file may make the library reserve (png_parse_info: below 2^31 bytes, and
// no more than 1032 x its IDAT payload); here the file is held against what the caller announced.  (Layout only: *_source_to_blob verifies the
// CRCs and reads the streams, so the file is summed once per request.)
static int file_source_check(flgpu_ctx *c, const flgpu_image *src, SourceProbe &out)
{
    static const struct { const char *malformed, *refused, *mismatch; } kTexts[] = { // [kind - SRC_PNG]
        {"malformed PNG file (signature, chunk layout, CRC, IHDR or too few bytes)",
         "PNG file not covered by the device decoder (16-bit samples, Adam7 interlace, or 2^31 bytes and more)",
         "FLGPU_IMG_PNG_SOURCE: width / height / channels do not match the file (see flgpu_png_info_of)"},
        {"malformed WebP file (RIFF size, chunk layout, VP8L signature or version)",
         "WebP file not covered by the device decoder (lossy VP8, ALPH, animation)",
         "FLGPU_IMG_WEBP_SOURCE: width / height / channels do not match the file (see flgpu_webp_info_of)"},
        {"malformed lossy WebP file (RIFF size, chunk layout, frame tag, start code, partition sizes or too few bytes)",
         "lossy WebP file not covered by the device decoder: ",
         "FLGPU_IMG_VP8_SOURCE: width / height / channels do not match the file (see flgpu_vp8_info_of)"}};
    const auto &t = kTexts[out.kind - SRC_PNG];
    const bool adam7 = (src->flags & FLGPU_IMG_PNG_ADAM7) != 0;
    if (file_head(out.kind, src->data, (size_t)src->capacity, png_head_opts(src->flags), out) != 0) { c->set_error(t.malformed); return FLGPU_ERR_PARSE; }
    const FileHead &h = out.head;
    if (!h.supported) {
        // the two refusals with a text of their own: a lossy WebP names the feature, a PNG asked for with Adam7 does not list it
        if (out.kind == SRC_VP8) c->set_error(std::string(t.refused) + (out.vp8.refused ? out.vp8.refused : "unknown feature"));
        else c->set_error(adam7 ? "PNG file not covered by the device decoder (16-bit samples, or 2^31 bytes and more)" : t.refused);
        return FLGPU_ERR_UNSUPPORTED;
    }
    if (h.width != src->width || h.height != src->height || h.channels != src->channels) { c->set_error(t.mismatch); return FLGPU_ERR_INVALID_ARG; }
    return FLGPU_OK;
}

// ---- PNG sources -----------------------------------------------------------------------------------------------------------------

// whether the deflate stream of a source with these flags goes to the device (not in the second run after the device said no)
static bool png_device_inflate(uint32_t src_flags) { return (src_flags & FLGPU_IMG_PNG_INFLATE) != 0 && !tl_force_host_huffman; }

static int png_source_to_blob(flgpu_ctx *c, const flgpu_image *src, uint8_t *blob, size_t cap, PngBlobHeader *hdr, size_t *used)
{
    if (cap < sizeof(PngBlobHeader)) return FLGPU_ERR_BUFFER_TOO_SMALL;
    if (png_device_inflate(src->flags)) {
        // only the container walk (with its CRCs) and one copy here: the device inflates the stream, and whatever it says no to comes back for the host inflate
        const int rc = png_stage_compressed(src->data, (size_t)src->capacity, blob, cap, hdr, (src->flags & FLGPU_IMG_PNG_ADAM7) != 0);
        if (rc == kPngParse) c->set_error("malformed PNG file (chunk CRC, Huffman code, distance, length, Adler-32 or filter byte)");
        if (rc) return png_status(rc);
        *used = hdr->total_bytes;
        return FLGPU_OK;
    }
    const int rc = png_decode_scanlines(src->data, (size_t)src->capacity, blob + sizeof(PngBlobHeader), cap - sizeof(PngBlobHeader), hdr,
                                        (src->flags & FLGPU_IMG_PNG_ADAM7) != 0);
    if (rc == kPngParse) c->set_error("malformed PNG file (chunk CRC, Huffman code, distance, length, Adler-32 or filter byte)");
    if (rc == kPngUnsupported) c->set_error("PNG stream holds more scanline data than its IHDR implies");
    if (rc) return png_status(rc);
    memcpy(blob, hdr, sizeof(*hdr));
    *used = hdr->total_bytes;
    return FLGPU_OK;
}

// The pictures staged compressed (kPngzMagic): one launch inflates them all, each into a scratch laid out like the blob of the host path, and
// dsrc[i].data is pointed at it.  Without such a picture nothing is reserved and nothing launched.
static int inflate_png_sources(flgpu_ctx *c, size_t n, flgpu_image *dsrc, const StagedSource *const *srcs, hipStream_t st)
{
    size_t ni = 0, bytes = 0;
    for (size_t i = 0; i < n; ++i)
        if (srcs[i]->kind == SRC_PNG && srcs[i]->png.magic == kPngzMagic) { ++ni; bytes += align_up(sizeof(PngBlobHeader) + png_header_scan_bytes(srcs[i]->png) + 64, 256); }
    if (!ni) return FLGPU_OK;
    FL_HIP(c, c->d_inf.reserve(bytes), "PNG inflate scratch");
    FL_HIP(c, c->d_inferr.reserve(ni * 4), "PNG inflate error words");
    FL_HIP(c, c->h_inferr.reserve(ni * 4), "PNG inflate error words");
    FL_HIP(c, c->h_infjobs.reserve(ni * sizeof(InfJob)), "PNG inflate descriptors");
    FL_HIP(c, c->d_infjobs.reserve(ni * sizeof(InfJob)), "PNG inflate descriptors");
    InfJob *jobs = static_cast<InfJob *>(c->h_infjobs.p);
    size_t off = 0, k = 0;
    for (size_t i = 0; i < n; ++i) {
        if (srcs[i]->kind != SRC_PNG || srcs[i]->png.magic != kPngzMagic) continue;
        const PngBlobHeader &H = srcs[i]->png;
        const size_t scan = png_header_scan_bytes(H);
        if (H.total_bytes < sizeof(PngBlobHeader) + kPngzPad || H.total_bytes > dsrc[i].capacity || scan >= kPngMaxDecoded) { c->set_error("PNG source: damaged blob header"); return FLGPU_ERR_INVALID_ARG; }
        InfJob &j = jobs[k];
        memset(&j, 0, sizeof(j));
        j.stage = dsrc[i].data;
        j.scratch = static_cast<uint8_t *>(c->d_inf.p) + off; off += align_up(sizeof(PngBlobHeader) + scan + 64, 256);
        j.err = static_cast<uint32_t *>(c->d_inferr.p) + k;
        j.payload_bytes = (uint32_t)(H.total_bytes - sizeof(PngBlobHeader) - kPngzPad);
        j.expected = (uint32_t)scan;
        dsrc[i].data = j.scratch; // what the unfilter, expand and Adam7 kernels read from here on
        c->last_inf_slot[i] = (int32_t)k++;
    }
    FL_HIP(c, hipMemcpyAsync(c->d_infjobs.p, jobs, ni * sizeof(InfJob), hipMemcpyHostToDevice, st), "PNG inflate descriptors");
    FL_HIP(c, launch_png_inflate(static_cast<const InfJob *>(c->d_infjobs.p), (uint32_t)ni, st), "PNG inflate kernel");
    c->last_inf_n = (uint32_t)ni;
    return FLGPU_OK;
}

static int decode_png_sources(flgpu_ctx *c, size_t n, flgpu_image *dsrc, const StagedSource *const *srcs, hipStream_t st)
{
    // np pictures; nu unfilter jobs (one per picture, one per non-empty pass of an Adam7 picture), nx_all expand and na_all de-interlace jobs
    size_t np = 0, nu = 0, nx_all = 0, na_all = 0, scratch = 0;
    for (size_t i = 0; i < n; ++i) {
        if (srcs[i]->kind != SRC_PNG) continue;
        const PngBlobHeader *H = &srcs[i]->png;
        ++np;
        scratch += align_up((size_t)H->width * H->height * H->channels + 64, 256);
        if (H->interlaced) {
            scratch += align_up((size_t)adam7_rows_bytes(H->width, H->height, png_pixel_bits(*H)) + 64, 256);
            for (uint32_t p = 0; p < kAdam7Passes; ++p) {
                const Adam7Pass P = adam7_pass(H->width, H->height, png_pixel_bits(*H), p);
                if (P.w && P.h) ++nu;
            }
            ++na_all;
            continue;
        }
        ++nu;
        if (!H->direct) { scratch += align_up((size_t)H->height * H->row_bytes + 64, 256); ++nx_all; }
    }
    c->last_inf_slot.assign(n, -1);
    c->last_inf_n = 0;
    if (!np) return FLGPU_OK;
    if (int rc = inflate_png_sources(c, n, dsrc, srcs, st)) return rc;
    FL_HIP(c, c->d_pngdec.reserve(scratch), "PNG decode scratch");
    FL_HIP(c, c->h_pngjobs.reserve((nu + nx_all + na_all) * sizeof(PngDecJob)), "PNG decode descriptors");
    FL_HIP(c, c->d_pngjobs.reserve((nu + nx_all + na_all) * sizeof(PngDecJob)), "PNG decode descriptors");
    // unfilter jobs ordered by bpp (one launch per pixel size), behind them once more the pictures the expand kernel takes, then the Adam7 pictures
    PngDecJob *jobs = static_cast<PngDecJob *>(c->h_pngjobs.p), *xjobs = jobs + nu, *ajobs = xjobs + nx_all;
    uint32_t per_bpp[4] = {0, 0, 0, 0}, nx = 0, na = 0, max_px = 0, max_apx = 0;
    size_t off = 0, k = 0, seen = 0;
    for (uint32_t bpp = 1; bpp <= 4; ++bpp)
        for (size_t i = 0; i < n; ++i) {
            if (srcs[i]->kind != SRC_PNG || srcs[i]->png.bpp != bpp) continue;
            const PngBlobHeader &H = srcs[i]->png;
            PngDecJob j;
            memset(&j, 0, sizeof(j));
            j.blob = dsrc[i].data;
            j.width = H.width; j.height = H.height; j.row_bytes = H.row_bytes; j.bpp = H.bpp;
            j.pixels = static_cast<uint8_t *>(c->d_pngdec.p) + off; off += align_up((size_t)H.width * H.height * H.channels + 64, 256);
            j.rows = j.pixels;
            if (H.interlaced) {
                // every non-empty pass is a picture of its own to the unfilter kernel; the de-interlace kernel takes the whole one
                j.rows = static_cast<uint8_t *>(c->d_pngdec.p) + off; off += align_up((size_t)adam7_rows_bytes(H.width, H.height, png_pixel_bits(H)) + 64, 256);
                for (uint32_t p = 0; p < kAdam7Passes; ++p) {
                    const Adam7Pass P = adam7_pass(H.width, H.height, png_pixel_bits(H), p);
                    if (!P.w || !P.h) continue;
                    PngDecJob &u = jobs[k++];
                    u = j;
                    u.width = P.w; u.height = P.h; u.row_bytes = P.row_bytes;
                    u.scan_off = (uint32_t)P.scan_off; u.rows = j.rows + P.rows_off;
                    per_bpp[bpp - 1]++;
                }
                ajobs[na++] = j;
                max_apx = std::max(max_apx, H.width * H.height);
            } else {
                if (!H.direct) {
                    j.rows = static_cast<uint8_t *>(c->d_pngdec.p) + off; off += align_up((size_t)H.height * H.row_bytes + 64, 256);
                    xjobs[nx++] = j;
                    max_px = std::max(max_px, H.width * H.height);
                }
                jobs[k++] = j;
                per_bpp[bpp - 1]++;
            }
            ++seen;
            if (!tl_force_host_huffman) { c->png_sources++; c->png_upload_bytes += H.total_bytes; } // (not twice when a batch is run again with the host Huffman decoder)
            dsrc[i].data = j.pixels;
            dsrc[i].channels = H.channels;
            dsrc[i].capacity = (uint64_t)H.width * H.height * H.channels;
            dsrc[i].flags &= ~(FLGPU_IMG_PNG_SOURCE | FLGPU_IMG_PNG_ADAM7 | FLGPU_IMG_PNG_INFLATE);
        }
    if (seen != np) { c->set_error("PNG source: pixel size outside 1..4 bytes"); return FLGPU_ERR_INVALID_ARG; }
    FL_HIP(c, hipMemcpyAsync(c->d_pngjobs.p, jobs, (nu + nx + na) * sizeof(PngDecJob), hipMemcpyHostToDevice, st), "PNG decode descriptors");
    const PngDecJob *d_jobs = static_cast<const PngDecJob *>(c->d_pngjobs.p);
    FL_HIP(c, launch_png_unfilter(d_jobs, per_bpp, st), "PNG unfilter kernel");
    if (nx) FL_HIP(c, launch_png_expand(d_jobs + nu, nx, max_px, st), "PNG expand kernel");
    if (na) FL_HIP(c, launch_png_adam7(d_jobs + nu + nx, na, max_apx, st), "PNG Adam7 kernel");
    return FLGPU_OK;
}

// ---- lossless WebP sources ---------------------------------------------------------------------------------------------------------

static int webp_source_to_blob(flgpu_ctx *c, const flgpu_image *src, uint8_t *blob, size_t cap, WebpBlobHeader *hdr, size_t *used)
{
    const int rc = webp_decode_residuals(src->data, (size_t)src->capacity, blob, cap, hdr);
    if (rc == kWebpParse) c->set_error("malformed lossless WebP stream (prefix code, transform, backward reference, colour cache index or too few bytes)");
    if (rc == kWebpUnsupported) c->set_error("lossless WebP stream with more code tables than the decoder's work area holds");
    if (rc) return webp_status(rc);
    *used = hdr->total_bytes;
    return FLGPU_OK;
}

// The job lists of a batch's lossless pictures: the runs in front of a predictor transform, the runs that end in pixels, the predictor transforms.
struct WebpJobLists {
    WebpRunJob *ra = nullptr, *rb = nullptr;
    WebpPredictJob *pj = nullptr;
    uint32_t na = 0, nb = 0, npred = 0, max_a = 0, max_b = 0;
};

// The inverse transforms of one picture, last to first, as jobs on L: `pixels` receives H.channels interleaved bytes, the intermediate
// pictures of dwords are taken from base + off.  (A lossless WebP source, and the VP8L-coded alpha plane of a lossy one.)
static int webp_picture_jobs(flgpu_ctx *c, const WebpBlobHeader &H, const uint8_t *blob, uint8_t *base, size_t &off, uint8_t *pixels, WebpJobLists &L)
{
    const uint32_t *cur = reinterpret_cast<const uint32_t *>(blob + H.res_off);
    uint32_t cw = H.xsize;
    WebpRunJob run;
    auto begin_run = [&] { memset(&run, 0, sizeof(run)); run.src = cur; run.src_w = cw; run.height = H.height; };
    begin_run();
    if (H.ntransforms > 4) { c->set_error("WebP source: damaged blob header"); return FLGPU_ERR_INVALID_ARG; }
    for (uint32_t k = H.ntransforms; k-- > 0;) { // the inverse transforms, last to first
        if (H.ttype[k] == kWtPredictor) {
            if (run.nops) { // what is pointwise in front of it goes into a picture of dwords first
                uint32_t *mid = reinterpret_cast<uint32_t *>(base + off); off += align_up((size_t)cw * H.height * 4u + 64, 256);
                run.dst = mid; run.dst_w = cw; run.out_c = 0;
                L.ra[L.na++] = run;
                L.max_a = std::max(L.max_a, cw * H.height);
                cur = mid;
            }
            uint32_t *out = reinterpret_cast<uint32_t *>(base + off); off += align_up((size_t)cw * H.height * 4u + 64, 256);
            WebpPredictJob &p = L.pj[L.npred++];
            memset(&p, 0, sizeof(p));
            p.res = cur; p.modes = reinterpret_cast<const uint32_t *>(blob + H.toff[k]); p.out = out;
            p.width = cw; p.height = H.height; p.bits = H.tbits[k];
            if (H.twidth[k] != cw || p.bits < 2u || p.bits > 9u) { c->set_error("WebP source: damaged blob header"); return FLGPU_ERR_INVALID_ARG; }
            cur = out;
            begin_run();
            continue;
        }
        WebpOp &op = run.ops[run.nops++];
        op.type = H.ttype[k];
        op.data = reinterpret_cast<const uint32_t *>(blob + H.toff[k]);
        if (op.type == kWtCrossColor) { op.bits = H.tbits[k]; op.width = H.twidth[k]; }
        if (op.type == kWtColorIndexing) { op.bits = run.shift = webp_index_shift(H.tbits[k]); cw = H.twidth[k]; }
    }
    if (cw != H.width) { c->set_error("WebP source: damaged blob header"); return FLGPU_ERR_INVALID_ARG; }
    run.dst = pixels; run.dst_w = cw; run.out_c = H.channels;
    L.rb[L.nb++] = run;
    L.max_b = std::max(L.max_b, cw * H.height);
    return FLGPU_OK;
}

static int decode_webp_sources(flgpu_ctx *c, size_t n, flgpu_image *dsrc, const StagedSource *const *srcs, hipStream_t st)
{
    size_t np = 0, scratch = 0;
    for (size_t i = 0; i < n; ++i) {
        if (srcs[i]->kind != SRC_WEBP) continue;
        const WebpBlobHeader *H = &srcs[i]->webp;
        ++np;
        // the pixels, and at most two intermediate pictures of dwords (in front of and behind the predictor transform)
        scratch += align_up((size_t)H->width * H->height * H->channels + 64, 256) + 2 * align_up((size_t)H->width * H->height * 4u + 64, 256);
    }
    if (!np) return FLGPU_OK;
    const size_t run_bytes = 2 * np * sizeof(WebpRunJob), job_bytes = run_bytes + np * sizeof(WebpPredictJob);
    FL_HIP(c, c->d_webpdec.reserve(scratch), "WebP decode scratch");
    FL_HIP(c, c->h_webpjobs.reserve(job_bytes), "WebP decode descriptors");
    FL_HIP(c, c->d_webpjobs.reserve(job_bytes), "WebP decode descriptors");
    // descriptors: the runs in front of a predictor transform, the runs that end in pixels, the predictor transforms
    WebpJobLists L;
    L.ra = static_cast<WebpRunJob *>(c->h_webpjobs.p); L.rb = L.ra + np;
    L.pj = reinterpret_cast<WebpPredictJob *>(static_cast<uint8_t *>(c->h_webpjobs.p) + run_bytes);
    size_t off = 0;
    for (size_t i = 0; i < n; ++i) {
        if (srcs[i]->kind != SRC_WEBP) continue;
        const WebpBlobHeader &H = srcs[i]->webp;
        const uint8_t *blob = dsrc[i].data;
        uint8_t *base = static_cast<uint8_t *>(c->d_webpdec.p);
        uint8_t *pixels = base + off; off += align_up((size_t)H.width * H.height * H.channels + 64, 256);
        if (int rc = webp_picture_jobs(c, H, blob, base, off, pixels, L)) return rc;
        if (!tl_force_host_huffman) { c->webp_sources++; c->webp_upload_bytes += H.total_bytes; } // (not twice when a batch is run again with the host Huffman decoder)
        dsrc[i].data = pixels;
        dsrc[i].channels = H.channels;
        dsrc[i].capacity = (uint64_t)H.width * H.height * H.channels;
        dsrc[i].flags &= ~FLGPU_IMG_WEBP_SOURCE;
    }
    FL_HIP(c, hipMemcpyAsync(c->d_webpjobs.p, c->h_webpjobs.p, job_bytes, hipMemcpyHostToDevice, st), "WebP decode descriptors");
    const WebpRunJob *d_ra = static_cast<const WebpRunJob *>(c->d_webpjobs.p);
    const WebpPredictJob *d_pj = reinterpret_cast<const WebpPredictJob *>(static_cast<const uint8_t *>(c->d_webpjobs.p) + run_bytes);
    if (L.na) { ProfileScope ps(c, st, 4); FL_HIP(c, launch_webp_run(d_ra, L.na, L.max_a, st), "WebP pointwise transform kernel"); }
    if (L.npred) { ProfileScope ps(c, st, 3); FL_HIP(c, launch_webp_predict(d_pj, L.npred, st), "WebP predictor kernel"); }
    { ProfileScope ps(c, st, 4); FL_HIP(c, launch_webp_run(d_ra + np, L.nb, L.max_b, st), "WebP pointwise transform kernel"); }
    return FLGPU_OK;
}

// ---- lossy WebP sources ------------------------------------------------------------------------------------------------------------

static int vp8_source_to_blob(flgpu_ctx *c, const flgpu_image *src, uint8_t *blob, size_t cap, Vp8BlobHeader *hdr, size_t *used)
{
    const int rc = vp8_decode_levels(src->data, (size_t)src->capacity, blob, cap, hdr);
    if (rc == kVp8Parse) c->set_error("malformed lossy WebP stream (a partition ends before its last macroblock, or a damaged ALPH stream)");
    if (rc == kVp8Unsupported) c->set_error("lossy WebP file: ALPH stream with more code tables than the decoder's work area holds");
    if (rc) return vp8_status(rc);
    *used = hdr->total_bytes;
    return FLGPU_OK;
}

// scratch of one picture: the padded planes, the alpha plane, the pixels
static size_t vp8_scratch_bytes(const Vp8BlobHeader &H)
{
    // (a VP8L-coded alpha plane: its R, G, B, A bytes and at most two intermediate pictures of dwords, as for a lossless source)
    return align_up((size_t)vp8_rec_bytes(H.mbw, H.mbh) + 64, 256) + (H.alpha ? align_up((size_t)H.width * H.height + 64, 256) : 0) +
           (H.alpha == 2u ? 3 * align_up((size_t)H.width * H.height * 4u + 64, 256) : 0) + align_up((size_t)H.width * H.height * H.channels + 64, 256);
}

// jobs[0 .. n) over `scratch`: per picture the planes, the alpha plane where the blob has one, the pixels
static void vp8_jobs(Vp8DecJob *jobs, uint8_t *scratch, const Vp8BlobHeader *const *H, const uint8_t *const *blobs, size_t n)
{
    size_t off = 0;
    for (size_t k = 0; k < n; ++k) {
        Vp8DecJob &j = jobs[k];
        memset(&j, 0, sizeof(j));
        j.blob = blobs[k];
        j.planes = scratch + off; off += align_up((size_t)vp8_rec_bytes(H[k]->mbw, H[k]->mbh) + 64, 256);
        if (H[k]->alpha) {
            j.alpha = scratch + off; off += align_up((size_t)H[k]->width * H[k]->height + 64, 256);
            j.alpha_src = blobs[k] + H[k]->alpha_off; j.alpha_stride = 1; // (a VP8L-coded plane: decode_vp8_sources points it at the green bytes)
        }
        j.dst = scratch + off; off += align_up((size_t)H[k]->width * H[k]->height * H[k]->channels + 64, 256);
        j.width = H[k]->width; j.height = H[k]->height; j.channels = H[k]->channels; j.filtered = H[k]->filter_type != 0u;
    }
}

static int decode_vp8_sources(flgpu_ctx *c, size_t n, flgpu_image *dsrc, const StagedSource *const *srcs, hipStream_t st)
{
    // the pictures the loop filter runs on go first: its kernel is launched for that many workgroups
    std::vector<size_t> order;
    for (int filtered = 1; filtered >= 0; --filtered)
        for (size_t i = 0; i < n; ++i)
            if (srcs[i]->kind == SRC_VP8 && (srcs[i]->vp8.filter_type != 0u) == (filtered != 0)) order.push_back(i);
    const size_t np = order.size();
    if (!np) return FLGPU_OK;
    size_t scratch = 0;
    std::vector<const Vp8BlobHeader *> H(np);
    std::vector<const uint8_t *> blobs(np);
    for (size_t k = 0; k < np; ++k) {
        H[k] = &srcs[order[k]]->vp8; blobs[k] = dsrc[order[k]].data;
        if (H[k]->magic != kVp8BlobMagic || H[k]->mbw != vp8_mbs(H[k]->width) || H[k]->mbh != vp8_mbs(H[k]->height)) { c->set_error("lossy WebP source: damaged blob header"); return FLGPU_ERR_INVALID_ARG; }
        scratch += vp8_scratch_bytes(*H[k]);
    }
    // descriptors: the decode jobs, and for the VP8L-coded alpha planes the lossless decoder's three job lists behind them
    size_t ncoded = 0;
    for (size_t k = 0; k < np; ++k) ncoded += H[k]->alpha == 2u;
    const size_t dec_bytes = align_up(np * sizeof(Vp8DecJob), 256), run_bytes = 2 * ncoded * sizeof(WebpRunJob);
    const size_t job_bytes = dec_bytes + run_bytes + ncoded * sizeof(WebpPredictJob);
    FL_HIP(c, c->d_vp8dec.reserve(scratch), "lossy WebP decode scratch");
    FL_HIP(c, c->h_vp8jobs.reserve(job_bytes), "lossy WebP decode descriptors");
    FL_HIP(c, c->d_vp8jobs.reserve(job_bytes), "lossy WebP decode descriptors");
    Vp8DecJob *jobs = static_cast<Vp8DecJob *>(c->h_vp8jobs.p);
    uint8_t *base = static_cast<uint8_t *>(c->d_vp8dec.p);
    vp8_jobs(jobs, base, H.data(), blobs.data(), np);
    WebpJobLists L;
    L.ra = reinterpret_cast<WebpRunJob *>(static_cast<uint8_t *>(c->h_vp8jobs.p) + dec_bytes); L.rb = L.ra + ncoded;
    L.pj = reinterpret_cast<WebpPredictJob *>(static_cast<uint8_t *>(c->h_vp8jobs.p) + dec_bytes + run_bytes);
    size_t off = 0;
    for (size_t k = 0; k < np; ++k) off += vp8_scratch_bytes(*H[k]) - (H[k]->alpha == 2u ? 3 * align_up((size_t)H[k]->width * H[k]->height * 4u + 64, 256) : 0);
    for (size_t k = 0; k < np; ++k) { // the alpha planes' own scratch lies behind every picture's planes and pixels
        if (H[k]->alpha != 2u) continue;
        const WebpBlobHeader &W = srcs[order[k]]->vp8_alpha;
        if (W.magic != kWebpMagic || W.width != H[k]->width || W.height != H[k]->height || W.channels != 4u) { c->set_error("lossy WebP source: damaged alpha blob header"); return FLGPU_ERR_INVALID_ARG; }
        uint8_t *rgba = base + off; off += align_up((size_t)W.width * W.height * 4u + 64, 256);
        if (int rc = webp_picture_jobs(c, W, blobs[k] + H[k]->alpha_off, base, off, rgba, L)) return rc;
        jobs[k].alpha_src = rgba + 1; jobs[k].alpha_stride = 4; // the green byte of R, G, B, A
    }
    for (size_t k = 0; k < np; ++k) {
        const size_t i = order[k];
        if (!tl_force_host_huffman) { c->vp8_sources++; c->vp8_upload_bytes += H[k]->total_bytes; } // (not twice when a batch is run again with the host Huffman decoder)
        dsrc[i].data = jobs[k].dst;
        dsrc[i].channels = H[k]->channels;
        dsrc[i].capacity = (uint64_t)H[k]->width * H[k]->height * H[k]->channels;
        dsrc[i].flags &= ~FLGPU_IMG_VP8_SOURCE;
    }
    FL_HIP(c, hipMemcpyAsync(c->d_vp8jobs.p, c->h_vp8jobs.p, job_bytes, hipMemcpyHostToDevice, st), "lossy WebP decode descriptors");
    ProfileScope ps(c, st, 8);
    if (ncoded) { // the existing inverse transforms on the alpha planes' residuals
        const WebpRunJob *d_ra = reinterpret_cast<const WebpRunJob *>(static_cast<const uint8_t *>(c->d_vp8jobs.p) + dec_bytes);
        const WebpPredictJob *d_pj = reinterpret_cast<const WebpPredictJob *>(static_cast<const uint8_t *>(c->d_vp8jobs.p) + dec_bytes + run_bytes);
        if (L.na) FL_HIP(c, launch_webp_run(d_ra, L.na, L.max_a, st), "WebP pointwise transform kernel (alpha plane)");
        if (L.npred) FL_HIP(c, launch_webp_predict(d_pj, L.npred, st), "WebP predictor kernel (alpha plane)");
        FL_HIP(c, launch_webp_run(d_ra + ncoded, L.nb, L.max_b, st), "WebP pointwise transform kernel (alpha plane)");
    }
    FL_HIP(c, launch_vp8_decode(static_cast<const Vp8DecJob *>(c->d_vp8jobs.p), jobs, (uint32_t)np, st), "lossy WebP decode kernels");
    return FLGPU_OK;
}

int debug_vp8_planes(flgpu_ctx *c, const uint8_t *file, size_t n, int filter, uint8_t *out, size_t capacity, size_t *used)
{
    SourceProbe probe;
    if (int rc = file_head(SRC_VP8, file, n, 0, probe)) return rc;
    if (!probe.head.supported) return FLGPU_ERR_UNSUPPORTED;
    const size_t planes = (size_t)vp8_rec_bytes(vp8_mbs(probe.head.width), vp8_mbs(probe.head.height));
    *used = planes;
    if (!out) return FLGPU_OK;
    if (capacity < planes) return FLGPU_ERR_BUFFER_TOO_SMALL;
    const size_t cap = vp8_blob_capacity(probe.vp8);
    WorkBuf work(cap);
    uint8_t *blob = work.p;
    Vp8BlobHeader H;
    if (int rc = vp8_decode_levels(file, n, blob, cap, &H)) return vp8_status(rc);
    std::lock_guard<std::mutex> g(c->mu);
    FL_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    DeviceBuf d_blob, d_scratch, d_job;
    struct Release { DeviceBuf &a, &b, &c; ~Release() { a.release(); b.release(); c.release(); } } release{d_blob, d_scratch, d_job};
    FL_HIP(c, d_blob.reserve(H.total_bytes), "lossy WebP blob");
    FL_HIP(c, d_scratch.reserve(vp8_scratch_bytes(H)), "lossy WebP decode scratch");
    FL_HIP(c, d_job.reserve(sizeof(Vp8DecJob)), "lossy WebP decode descriptors");
    Vp8DecJob job;
    const Vp8BlobHeader *hp = &H;
    const uint8_t *bp = static_cast<const uint8_t *>(d_blob.p);
    vp8_jobs(&job, static_cast<uint8_t *>(d_scratch.p), &hp, &bp, 1);
    FL_HIP(c, hipMemcpy(d_blob.p, blob, H.total_bytes, hipMemcpyHostToDevice), "lossy WebP blob H2D");
    FL_HIP(c, hipMemcpy(d_job.p, &job, sizeof(job), hipMemcpyHostToDevice), "lossy WebP decode descriptors");
    FL_HIP(c, launch_vp8_decode(static_cast<const Vp8DecJob *>(d_job.p), &job, 1, nullptr, filter ? 2 : 1), "lossy WebP decode kernels");
    FL_HIP(c, hipMemcpy(out, job.planes, planes, hipMemcpyDeviceToHost), "lossy WebP planes D2H");
    return FLGPU_OK;
}

// ---- what every caller does with a source: probe, stage, decode ------------------------------------------------------------------------

int source_probe(flgpu_ctx *c, const flgpu_image *src, SourceProbe &out)
{
    out.kind = source_kind(src->flags);
    if ((src->flags & FLGPU_IMG_PNG_ADAM7) && !(src->flags & FLGPU_IMG_PNG_SOURCE)) {
        c->set_error("FLGPU_IMG_PNG_ADAM7 without FLGPU_IMG_PNG_SOURCE");
        return FLGPU_ERR_INVALID_ARG;
    }
    if ((src->flags & FLGPU_IMG_PNG_INFLATE) && !(src->flags & FLGPU_IMG_PNG_SOURCE)) {
        c->set_error("FLGPU_IMG_PNG_INFLATE without FLGPU_IMG_PNG_SOURCE");
        return FLGPU_ERR_INVALID_ARG;
    }
    switch (out.kind) {
    case SRC_JPEG: // its own statuses: FLGPU_ERR_INVALID_ARG, not _PARSE, for a file that does not parse; its own checks against the caller's announcement
        if (file_head(SRC_JPEG, src->data, (size_t)src->capacity, 0, out) != 0) return FLGPU_ERR_INVALID_ARG;
        if (!out.head.supported) return FLGPU_ERR_UNSUPPORTED; // (no text from here: flgpu_transform adds its own, a host batch has none)
        if (int rc = jpeg_source_precheck(c, src, out.jpeg)) return rc;
        out.capacity = jpeg_source_capacity(c, src, out.jpeg);
        break;
    case SRC_PNG: case SRC_WEBP: case SRC_VP8:
        if (int rc = file_source_check(c, src, out)) return rc;
        out.capacity = out.kind == SRC_PNG ? (png_device_inflate(src->flags) ? png_stage_bytes(out.png) : png_blob_bytes(out.png)) : out.kind == SRC_WEBP ? webp_blob_capacity(out.webp, (size_t)src->capacity) : vp8_blob_capacity(out.vp8);
        break;
    case SRC_PIXELS:
        out.capacity = (size_t)src->width * src->height * src->channels;
        if (src->capacity < out.capacity) return FLGPU_ERR_INVALID_ARG;
        break;
    }
    return FLGPU_OK;
}

int source_stage(flgpu_ctx *c, const flgpu_image *src, SourceProbe &probe, void *buf, size_t cap, StagedSource &out, bool host_huffman)
{
    uint8_t *blob = static_cast<uint8_t *>(buf);
    int rc = FLGPU_OK;
    switch (probe.kind) {
    case SRC_JPEG:
        rc = jpeg_source_to_blob(c, src, blob, cap, &out.jpeg, &out.used, host_huffman);
        if (rc) return rc;
        if (out.jpeg.magic == kJhMagic) memcpy(&out.stage, blob + sizeof(JpegBlobHeader), sizeof(out.stage));
        if (out.jpeg.nc == 4 && c->cfg.use_embedded_profile) out.icc.swap(probe.jpeg.icc);
        break;
    case SRC_PNG: rc = png_source_to_blob(c, src, blob, cap, &out.png, &out.used); break;
    case SRC_WEBP: rc = webp_source_to_blob(c, src, blob, cap, &out.webp, &out.used); break;
    case SRC_VP8:
        rc = vp8_source_to_blob(c, src, blob, cap, &out.vp8, &out.used);
        if (!rc && out.vp8.alpha == 2u) memcpy(&out.vp8_alpha, blob + out.vp8.alpha_off, sizeof(out.vp8_alpha));
        break;
    case SRC_PIXELS: return FLGPU_OK; // nothing to decode: the caller copies the pixels, or hands over its pinned buffer
    }
    if (rc) return rc;
    out.kind = probe.kind;
    out.file_bytes = src->capacity;
    return FLGPU_OK;
}

int decode_sources(flgpu_ctx *c, size_t n, flgpu_image *dsrc, const StagedSource *const *staged, hipStream_t st)
{
    // the files' own bytes: JPEG on every run; PNG and WebP not twice when a batch is run again with the host Huffman decoder
    for (size_t i = 0; i < n; ++i) {
        if (staged[i]->kind == SRC_JPEG) c->stats.jpeg_file_bytes += staged[i]->file_bytes;
        if (staged[i]->kind == SRC_PNG && !tl_force_host_huffman) c->png_file_bytes += staged[i]->file_bytes;
        if (staged[i]->kind == SRC_WEBP && !tl_force_host_huffman) c->webp_file_bytes += staged[i]->file_bytes;
        if (staged[i]->kind == SRC_VP8 && !tl_force_host_huffman) c->vp8_file_bytes += staged[i]->file_bytes;
    }
    if (int rc = decode_jpeg_sources(c, n, dsrc, staged, st)) return rc;
    if (int rc = decode_png_sources(c, n, dsrc, staged, st)) return rc;
    if (int rc = decode_webp_sources(c, n, dsrc, staged, st)) return rc;
    return decode_vp8_sources(c, n, dsrc, staged, st);
}

// Enqueues the copy of the device entropy decoder's and the device inflate's error words (final once their kernels have run): a caller that
// waits for the stream anyway asks for them in front of that wait and passes fetched = true below.
int entropy_failures_fetch(flgpu_ctx *c, size_t n, hipStream_t st)
{
    if (c->last_jh_n && c->last_jh_slot.size() == n)
        FL_HIP(c, hipMemcpyAsync(c->h_jherr.p, c->d_jherr.p, (size_t)c->last_jh_n * 4, hipMemcpyDeviceToHost, st), "device entropy decode: error words D2H");
    if (c->last_inf_n && c->last_inf_slot.size() == n)
        FL_HIP(c, hipMemcpyAsync(c->h_inferr.p, c->d_inferr.p, (size_t)c->last_inf_n * 4, hipMemcpyDeviceToHost, st), "PNG inflate: error words D2H");
    return FLGPU_OK;
}

int entropy_failures(flgpu_ctx *c, size_t n, std::vector<uint8_t> &bad, hipStream_t st, bool fetched)
{
    bad.assign(n, 0);
    const bool jh = c->last_jh_n && c->last_jh_slot.size() == n, inf = c->last_inf_n && c->last_inf_slot.size() == n;
    if (!jh && !inf) return 0;
    if (!fetched && (entropy_failures_fetch(c, n, st) != FLGPU_OK || hipStreamSynchronize(st) != hipSuccess)) {
        c->set_error("device entropy decode: error words D2H");
        return -FLGPU_ERR_DEVICE;
    }
    int nbad = 0;
    if (jh) {
        const uint32_t *e = static_cast<const uint32_t *>(c->h_jherr.p);
        if (c->dbg->on(DBG_DEBUG_JH)) for (uint32_t k = 0; k < c->last_jh_n; ++k) fprintf(stderr, "device entropy decode: picture %u error word %u\n", k, e[k]);
        int nj = 0;
        for (size_t i = 0; i < n; ++i)
            if (c->last_jh_slot[i] >= 0 && e[c->last_jh_slot[i]]) { bad[i] = 1; ++nj; }
        c->stats.jpeg_device_huffman_retries += (uint64_t)nj;
        nbad += nj;
    }
    if (inf) {
        const uint32_t *e = static_cast<const uint32_t *>(c->h_inferr.p);
        if (c->dbg->on(DBG_DEBUG_JH)) for (uint32_t k = 0; k < c->last_inf_n; ++k) fprintf(stderr, "PNG inflate: picture %u error word %u\n", k, e[k]);
        int ni = 0;
        for (size_t i = 0; i < n; ++i)
            if (c->last_inf_slot[i] >= 0 && e[c->last_inf_slot[i]]) { bad[i] = 1; ++ni; }
        c->png_device_inflates += (uint64_t)c->last_inf_n - (uint64_t)ni;
        c->png_inflate_retries += (uint64_t)ni;
        nbad += ni;
        c->last_inf_n = 0; // (counted once)
    }
    return nbad;
}

// One picture through the inflate kernel alone.
int debug_png_inflate_device(flgpu_ctx *c, const uint8_t *file, size_t n, uint32_t src_flags, uint8_t *out, size_t capacity, size_t *used)
{
    SourceProbe probe;
    if (int rc = file_head(SRC_PNG, file, n, HEAD_FULL | png_head_opts(src_flags), probe)) return rc;
    if (!probe.head.supported) return FLGPU_ERR_UNSUPPORTED;
    const size_t scan = png_scan_bytes(probe.png);
    *used = scan;
    if (!out) return FLGPU_OK;
    if (capacity < scan) return FLGPU_ERR_BUFFER_TOO_SMALL;
    const size_t cap = png_stage_bytes(probe.png);
    WorkBuf work(cap);
    PngBlobHeader H;
    if (int rc = png_stage_compressed(file, n, work.p, cap, &H, (src_flags & FLGPU_IMG_PNG_ADAM7) != 0)) return png_status(rc);
    std::lock_guard<std::mutex> g(c->mu);
    FL_HIP(c, hipSetDevice(c->device), "hipSetDevice");
    DeviceBuf d_stage, d_scratch, d_job;
    struct Release { DeviceBuf &a, &b, &c; ~Release() { a.release(); b.release(); c.release(); } } release{d_stage, d_scratch, d_job};
    FL_HIP(c, d_stage.reserve(cap), "PNG inflate staging");
    FL_HIP(c, d_scratch.reserve(sizeof(PngBlobHeader) + scan + 64), "PNG inflate scratch");
    FL_HIP(c, d_job.reserve(sizeof(InfJob) + 16), "PNG inflate descriptors");
    InfJob job;
    memset(&job, 0, sizeof(job));
    job.stage = static_cast<const uint8_t *>(d_stage.p);
    job.scratch = static_cast<uint8_t *>(d_scratch.p);
    job.err = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(d_job.p) + sizeof(InfJob));
    job.payload_bytes = (uint32_t)(H.total_bytes - sizeof(PngBlobHeader) - kPngzPad);
    job.expected = (uint32_t)scan;
    FL_HIP(c, hipMemcpy(d_stage.p, work.p, cap, hipMemcpyHostToDevice), "PNG inflate staging H2D");
    FL_HIP(c, hipMemcpy(d_job.p, &job, sizeof(job), hipMemcpyHostToDevice), "PNG inflate descriptors");
    FL_HIP(c, launch_png_inflate(static_cast<const InfJob *>(d_job.p), 1, nullptr), "PNG inflate kernel");
    uint32_t err = 0;
    FL_HIP(c, hipMemcpy(&err, job.err, 4, hipMemcpyDeviceToHost), "PNG inflate error word D2H");
    if (err) { c->set_error("PNG inflate kernel: no (error word " + std::to_string(err) + ")"); return FLGPU_ERR_PARSE; }
    FL_HIP(c, hipMemcpy(out, job.scratch + sizeof(PngBlobHeader), scan, hipMemcpyDeviceToHost), "PNG scanlines D2H");
    return FLGPU_OK;
}

} // namespace fl
