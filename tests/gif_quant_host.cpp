// The host twin of the GIF quantiser (csrc/fl_gifquant.hip): the functions of csrc/fl_gif_quant_core.h in plain loops, no device and
// no library.  tests/test_gif_quantize_host.py builds it (once plainly, once with -fsanitize=address,undefined), feeds it frames and
// holds what it writes against tests/gif_quant_model.py.
//
//   gif_quant_host IN OUT
//   IN:  u32 frames, h, w, c (2 | 4), then frames * h * w * c bytes
//   OUT: per frame u32 marked; for a marked frame u32 entries, transparent (0xffffffff: none), s, cells, then entries * 3 table
//        bytes and h * w index bytes
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "../fanlin-rs_amd/csrc/fl_gif_quant_core.h"

using namespace fl;

static void put32(FILE *f, uint32_t v) { fwrite(&v, 4, 1, f); }

static void quantize(const std::vector<uint32_t> &keys, FILE *out)
{
    bool clear = false;
    for (uint32_t k : keys) clear |= !(k & 255u);
    const uint32_t K = clear ? 255u : 256u;
    // the precision, then the cells in ascending order of their reduced colour (any order gives the same boxes)
    uint32_t s = 0;
    for (; s < 3u; ++s) {
        std::set<uint32_t> seen;
        for (uint32_t k : keys) if (k & 255u) seen.insert(gq_reduced(k, s));
        if (seen.size() <= kGifQuantHashCells) break;
    }
    std::map<uint32_t, uint32_t> cell_of;
    std::vector<uint32_t> n, sr, sg, sb;
    for (uint32_t k : keys) {
        if (!(k & 255u)) continue;
        const uint32_t id = s < 3u ? gq_reduced(k, s) : gq_cell15(k);
        auto it = cell_of.find(id);
        if (it == cell_of.end()) { it = cell_of.emplace(id, (uint32_t)n.size()).first; n.push_back(0); sr.push_back(0); sg.push_back(0); sb.push_back(0); }
        const uint32_t i = it->second;
        n[i] += 1u; sr[i] += k >> 24; sg[i] += (k >> 16) & 255u; sb[i] += (k >> 8) & 255u;
    }
    const uint32_t cells = (uint32_t)n.size();
    std::vector<uint32_t> rep(cells), box(cells, 0u);
    std::vector<GqBox> boxes;
    std::vector<GqChoice> choice;
    if (cells) {
        GqBox all;
        gq_box_clear(all);
        for (uint32_t i = 0; i < cells; ++i) { rep[i] = gq_pack(gq_mean(sr[i], n[i]), gq_mean(sg[i], n[i]), gq_mean(sb[i], n[i])); gq_box_add(all, n[i], rep[i]); }
        boxes.push_back(all);
        choice.push_back(gq_choice(all));
    }
    while (boxes.size() < K) {
        uint64_t word = 0;
        for (uint32_t b = 0; b < boxes.size(); ++b) word = std::max(word, gq_select_word(choice[b].rank, b));
        if (!word) break;
        const uint32_t b = gq_selected_box(word), nb = (uint32_t)boxes.size();
        GqBox up;
        gq_box_clear(up);
        for (uint32_t i = 0; i < cells; ++i)
            if (box[i] == b && gq_axis_of(rep[i], choice[b].axis) > choice[b].cut) { box[i] = nb; gq_box_add(up, n[i], rep[i]); }
        if (!up.n || up.n == boxes[b].n) { fprintf(stderr, "a split left a half empty\n"); exit(3); }
        gq_box_remove(boxes[b], up);
        boxes.push_back(up);
        choice[b] = gq_choice(boxes[b]);
        choice.push_back(gq_choice(up));
    }
    const uint32_t nb = (uint32_t)boxes.size();
    std::vector<uint32_t> sum(3u * nb, 0u), order(nb), table(nb);
    for (uint32_t i = 0; i < cells; ++i) { sum[3u * box[i]] += sr[i]; sum[3u * box[i] + 1u] += sg[i]; sum[3u * box[i] + 2u] += sb[i]; }
    for (uint32_t b = 0; b < nb; ++b) order[b] = gq_pack(gq_mean(sum[3u * b], boxes[b].n), gq_mean(sum[3u * b + 1u], boxes[b].n), gq_mean(sum[3u * b + 2u], boxes[b].n)) << 8 | b;
    std::sort(order.begin(), order.end());
    for (uint32_t b = 0; b < nb; ++b) table[b] = order[b] >> 8;
    put32(out, nb + (clear ? 1u : 0u)); put32(out, clear ? nb : 0xffffffffu); put32(out, s); put32(out, cells);
    for (uint32_t b = 0; b < nb; ++b) { const uint8_t e[3] = {(uint8_t)(table[b] >> 16), (uint8_t)(table[b] >> 8), (uint8_t)table[b]}; fwrite(e, 1, 3, out); }
    if (clear) { const uint8_t e[3] = {0, 0, 0}; fwrite(e, 1, 3, out); }
    for (uint32_t k : keys) fputc((int)((k & 255u) ? gq_nearest(table.data(), nb, k) : nb), out);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    uint32_t head[4];
    if (!in || !out || fread(head, 4, 4, in) != 4 || (head[3] != 2u && head[3] != 4u)) return 2;
    const size_t px = (size_t)head[1] * head[2];
    if (px > kGifQuantMaxPixels) return 2;
    std::vector<uint8_t> frame(px * head[3]);
    for (uint32_t f = 0; f < head[0]; ++f) {
        if (fread(frame.data(), 1, frame.size(), in) != frame.size()) return 2;
        std::vector<uint32_t> keys(px);
        for (size_t p = 0; p < px; ++p) {
            uint32_t v = 0;
            memcpy(&v, frame.data() + p * head[3], head[3]);
            keys[p] = head[3] == 4u ? gq_key_rgba(v) : gq_key_la(v);
        }
        const bool marked = std::set<uint32_t>(keys.begin(), keys.end()).size() > 256u;
        put32(out, marked ? 1u : 0u);
        if (marked) quantize(keys, out);
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
