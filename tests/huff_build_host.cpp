// huff_build_host.cpp -- csrc/fl_huff_build.h on the CPU, under AddressSanitizer and UBSan (tests/test_huff_build_host.py builds and
// runs it).  The header is device code for one thread and plain C++ apart from __brev and min, so it is included unchanged after a
// host __brev and std::min.  On the device its fold to `limit` bits almost never runs: a 32 KB deflate segment or a picture's
// residuals rarely give a Huffman tree deeper than 15, so here every (limit, alphabet) pair the two encoders use gets the
// histograms that do: every Fibonacci prefix, powers of two, all ones, two used symbols, the full alphabet, and seeded random ones.
//
// Every buffer is a heap block of exactly the size the kernels pass (num: 96 words in fl_png.hip, kMiscBuild0..kMiscBuild1; 64 in
// fl_webpll.hip, s_num[a]) and num starts as garbage, so an access outside them, the num + 40 carve-out included, stops the run.
//
// Output: one line per pair, "limit nsyms num_words cases folded"; exit status 0 if every assertion held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <queue>
#include <vector>

static inline uint32_t __brev(uint32_t v)
{
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((v >> i) & 1u) << (31 - i);
    return r;
}
using std::min;

#include "fl_huff_build.h"

namespace {

struct Pair { uint32_t limit, nsyms, num_words; const char *user; };
const Pair kPairs[] = {
    {15, 286, 96, "fl_png.hip literal/length"}, {15, 30, 96, "fl_png.hip distance"}, {7, 19, 96, "fl_png.hip code lengths"},
    {15, 280, 64, "fl_webpll.hip green + lengths"}, {15, 256, 64, "fl_webpll.hip red / blue / alpha"}, {7, 19, 64, "fl_webpll.hip code lengths"},
};

struct Rng { // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

[[noreturn]] void fail(const Pair &p, const std::vector<uint32_t> &hist, const char *what)
{
    fprintf(stderr, "FAILED (%s, limit %u, %u symbols): %s\nhistogram:", p.user, p.limit, p.nsyms, what);
    for (uint32_t f : hist) fprintf(stderr, " %u", f);
    fprintf(stderr, "\n");
    exit(1);
}

// Depths of an unlimited Huffman tree over counts in ascending (count, symbol) order, by a heap.  On equal weights a leaf goes
// before a merged node and an older merged node before a younger one: the tree of least depth among the optimal ones.
std::vector<uint32_t> heap_depths(const std::vector<uint32_t> &key)
{
    const size_t n = key.size();
    struct Node { uint64_t w; uint32_t order; };
    auto later = [](const Node &a, const Node &b) { return a.w != b.w ? a.w > b.w : a.order > b.order; };
    std::priority_queue<Node, std::vector<Node>, decltype(later)> heap(later);
    std::vector<int> parent(2 * n - 1, -1);
    for (size_t i = 0; i < n; ++i) heap.push({key[i], (uint32_t)i});
    for (size_t m = n; m < 2 * n - 1; ++m) {
        const Node a = heap.top(); heap.pop();
        const Node b = heap.top(); heap.pop();
        parent[a.order] = parent[b.order] = (int)m;
        heap.push({a.w + b.w, (uint32_t)m});
    }
    std::vector<uint32_t> depth(2 * n - 1, 0);
    for (int m = (int)(2 * n - 3); m >= 0; --m) depth[m] = depth[parent[m]] + 1u;
    depth.resize(n);
    return depth;
}

// What a deflate encoder does with a tree deeper than the limit (zlib's repair, from its description): every deeper leaf is
// moved up to the limit, which over-subscribes the code; then, while it is over-subscribed, a leaf of the deepest level above the
// limit that has one becomes an inner node, with itself and one leaf taken from the limit level as its children one level
// down.  Each such step frees exactly 2^-limit.  The lengths then go to the symbols by count: the rarest get the longest.
std::vector<uint32_t> repaired_counts(const std::vector<uint32_t> &depth, uint32_t limit)
{
    std::vector<uint32_t> per(limit + 1u, 0);
    for (uint32_t d : depth) per[std::min(d, limit)]++;
    auto kraft = [&]() { uint64_t k = 0; for (uint32_t l = 1; l <= limit; ++l) k += (uint64_t)per[l] << (limit - l); return k; };
    while (kraft() > (1ull << limit)) {
        uint32_t l = limit - 1u;
        while (l > 0u && per[l] == 0u) --l;
        if (l == 0u) return {};
        per[l] -= 1u; per[l + 1u] += 2u; per[limit] -= 1u;
    }
    return per;
}

struct Totals { uint64_t cases = 0, folded = 0; };

void check(const Pair &p, const std::vector<uint32_t> &hist, Totals &t)
{
    const uint32_t limit = p.limit, nsyms = p.nsyms;
    // rank the used symbols by (count, symbol), as the kernels do before they call the builder
    std::vector<uint32_t> order;
    for (uint32_t s = 0; s < nsyms; ++s) if (hist[s]) order.push_back(s);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return hist[a] < hist[b]; });
    const int n = (int)order.size();
    if (n < 2) fail(p, hist, "the case generator made a histogram with fewer than two used symbols");
    std::vector<uint32_t> key(n);
    for (int i = 0; i < n; ++i) key[i] = hist[order[i]];

    uint32_t *A = new uint32_t[n], *sym = new uint32_t[n], *code = new uint32_t[nsyms], *num = new uint32_t[p.num_words];
    for (int i = 0; i < n; ++i) { A[i] = key[i]; sym[i] = order[i]; }
    for (uint32_t s = 0; s < nsyms; ++s) code[s] = 0u;
    for (uint32_t i = 0; i < p.num_words; ++i) num[i] = 0xdeadbeefu;
    fl::huff_build(A, sym, n, limit, nsyms, code, num);

    // lengths: 1..limit for used symbols, 0 for the others; Kraft sum exactly 1
    uint64_t kraft = 0, cost = 0;
    std::vector<uint32_t> per(limit + 2u, 0);
    for (uint32_t s = 0; s < nsyms; ++s) {
        const uint32_t len = code[s] >> 16;
        if (hist[s] == 0u) { if (code[s] != 0u) fail(p, hist, "an unused symbol got a code"); continue; }
        if (len < 1u || len > limit) fail(p, hist, "a used symbol's length is outside 1..limit");
        kraft += 1ull << (limit - len);
        cost += (uint64_t)hist[s] * len;
        per[len]++;
    }
    if (kraft != (1ull << limit)) fail(p, hist, "the Kraft sum is not 1");
    // rarer never shorter, in the (count, symbol) order
    for (int i = 1; i < n; ++i)
        if ((code[order[i]] >> 16) > (code[order[i - 1]] >> 16)) fail(p, hist, "a length grows with the count");
    // canonical codes of RFC 1951 3.2.2, bit-reversed
    std::vector<uint32_t> next_code(limit + 2u, 0);
    for (uint32_t len = 1, c = 0; len <= limit; ++len) { c = (c + (len > 1u ? per[len - 1u] : 0u)) << 1; next_code[len] = c; }
    std::vector<std::pair<uint32_t, uint32_t>> spans; // [first, last] of every code, left-aligned to `limit` bits
    for (uint32_t s = 0; s < nsyms; ++s) {
        const uint32_t len = code[s] >> 16;
        if (!len) continue;
        const uint32_t v = next_code[len]++;
        if (v >> len) fail(p, hist, "the canonical code does not fit its length");
        uint32_t rev = 0;
        for (uint32_t b = 0; b < len; ++b) if ((v >> b) & 1u) rev |= 1u << (len - 1u - b);
        if ((code[s] & 0xffffu) != rev) fail(p, hist, "a code is not the bit-reversed canonical one");
        spans.push_back({v << (limit - len), ((v + 1u) << (limit - len)) - 1u});
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); ++i)
        if (spans[i].first <= spans[i - 1].second) fail(p, hist, "one code is a prefix of another");
    // cost: the optimum where the unlimited tree fits, the repaired tree's otherwise
    const std::vector<uint32_t> depth = heap_depths(key);
    uint64_t optimum = 0;
    uint32_t deepest = 0;
    for (int i = 0; i < n; ++i) { optimum += (uint64_t)key[i] * depth[i]; deepest = std::max(deepest, depth[i]); }
    if (cost < optimum) fail(p, hist, "cheaper than the optimal prefix code");
    if (deepest <= limit) {
        if (cost != optimum) fail(p, hist, "the unlimited tree fits the limit, yet the cost is not the optimum");
    } else {
        const std::vector<uint32_t> want = repaired_counts(depth, limit);
        if (want.empty()) fail(p, hist, "the reference repair found no leaf to move");
        uint64_t ref = 0;
        int i = 0;
        for (uint32_t len = limit; len >= 1u; --len)
            for (uint32_t k = 0; k < want[len]; ++k) ref += (uint64_t)key[i++] * len;
        if (i != n) fail(p, hist, "the reference repair lost a symbol");
        if (cost != ref) fail(p, hist, "the folded code's cost differs from the repaired tree's");
        t.folded++;
    }
    t.cases++;
    delete[] A; delete[] sym; delete[] code; delete[] num;
}

void run_pair(const Pair &p, uint32_t randoms)
{
    Totals t;
    const uint32_t N = p.nsyms;
    std::vector<uint32_t> h(N);
    auto clear = [&]() { std::fill(h.begin(), h.end(), 0u); };
    // every Fibonacci prefix whose sum fits 32 bits, in ascending and descending symbol order, and scaled
    for (uint32_t scale : {1u, 3u}) {
        for (uint32_t n = 2; n <= N; ++n) {
            std::vector<uint64_t> fib(n);
            uint64_t sum = 0;
            for (uint32_t i = 0; i < n; ++i) { fib[i] = i < 2u ? 1u : fib[i - 1] + fib[i - 2]; sum += fib[i] * scale; }
            if (sum > 0xffffffffull) break;
            clear(); for (uint32_t i = 0; i < n; ++i) h[i] = (uint32_t)fib[i] * scale;
            check(p, h, t);
            clear(); for (uint32_t i = 0; i < n; ++i) h[N - 1u - i] = (uint32_t)fib[i] * scale;
            check(p, h, t);
        }
    }
    // powers of two: 1, 1, 2, 4, ... and 1, 2, 4, ...
    for (uint32_t n = 2; n <= std::min(N, 31u); ++n) {
        clear(); for (uint32_t i = 0; i < n; ++i) h[i] = 1u << i;
        check(p, h, t);
        clear(); h[0] = 1u; for (uint32_t i = 1; i < n; ++i) h[i] = 1u << (i - 1u);
        check(p, h, t);
        clear(); for (uint32_t i = 0; i < n; ++i) h[(i * 7u) % N] += 1u << i;
        check(p, h, t);
    }
    // all ones (and all equal), every prefix
    for (uint32_t n = 2; n <= N; ++n) {
        clear(); for (uint32_t i = 0; i < n; ++i) h[i] = 1u;
        check(p, h, t);
        clear(); for (uint32_t i = 0; i < n; ++i) h[N - 1u - i] = 32768u;
        check(p, h, t);
    }
    // two used symbols
    for (uint32_t a = 0; a < N; ++a)
        for (uint32_t b : {(a + 1u) % N, (a + N / 2u) % N, N - 1u - a}) {
            if (a == b) continue;
            clear(); h[a] = 1u; h[b] = 1u; check(p, h, t);
            clear(); h[a] = 1u; h[b] = 0xfffffffeu; check(p, h, t);
            clear(); h[a] = 32767u; h[b] = 1u; check(p, h, t);
        }
    // the full alphabet: ramps, one giant, one dwarf
    clear(); for (uint32_t i = 0; i < N; ++i) h[i] = i + 1u; check(p, h, t);
    clear(); for (uint32_t i = 0; i < N; ++i) h[i] = N - i; check(p, h, t);
    clear(); for (uint32_t i = 0; i < N; ++i) h[i] = 1u; h[N / 2u] = 1u << 30; check(p, h, t);
    clear(); for (uint32_t i = 0; i < N; ++i) h[i] = 1000u; h[0] = 1u; check(p, h, t);
    clear(); for (uint32_t i = 0; i < N; ++i) h[i] = 1u << std::min(i / ((N + 23u) / 24u), 24u); check(p, h, t);
    // seeded random histograms: flat, sparse, geometric and steep ones (the steep ones are the ones that need the fold)
    Rng rng{0x5eed0000ull + p.limit * 1000u + p.nsyms + p.num_words};
    for (uint32_t k = 0; k < randoms; ++k) {
        clear();
        const uint32_t kind = k % 5u;
        const uint32_t used = kind == 1u ? 2u + rng.below(std::min(N - 1u, 12u)) : 2u + rng.below(N - 1u);
        const uint32_t top = 1u + rng.below(kind == 4u ? 30u : 22u);
        for (uint32_t i = 0; i < used; ++i) {
            uint32_t s = rng.below(N);
            while (h[s]) s = (s + 1u) % N;
            uint32_t f;
            if (kind == 0u) f = 1u + rng.below(64u);                       // flat and small: many ties
            else if (kind == 2u) f = 1u + rng.below(1u << rng.below(top)); // log-uniform
            else if (kind == 3u) f = 1u << rng.below(top);                 // powers of two with ties
            else f = 1u + (uint32_t)(rng.next() >> (64u - 1u - rng.below(top))) / (1u + (kind == 4u ? used / 8u : 0u));
            h[s] = std::max(f, 1u);
        }
        uint64_t sum = 0;
        for (uint32_t f : h) sum += f;
        if (sum > 0xffffffffull) { for (uint32_t &f : h) f = f ? (f >> 9) + 1u : 0u; } // (the builder adds counts in 32 bits)
        check(p, h, t);
    }
    printf("%u %u %u %llu %llu\n", p.limit, p.nsyms, p.num_words, (unsigned long long)t.cases, (unsigned long long)t.folded);
}

} // namespace

int main(int argc, char **argv)
{
    const uint32_t randoms = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 10) : 20000u;
    for (const Pair &p : kPairs) run_pair(p, randoms);
    return 0;
}
