// fl_huff_build.h -- the length-limited Huffman code builder shared by the PNG deflate (fl_png.hip) and the lossless WebP
// encoder (fl_webpll.hip).  Device code; one thread builds one code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fl {

// Code lengths of n >= 2 used symbols, key[] = their counts in ascending (count, symbol) order, sym[] the symbols: in-place
// minimum-redundancy lengths (Moffat & Katajainen), folded to `limit` bits with the Kraft sum restored, longest codes to the
// rarest symbols; then canonical codes, bit-reversed for the LSB-first stream: code[s] = length << 16 | reversed code.
__device__ inline void huff_build(uint32_t *A, const uint32_t *sym, int n, uint32_t limit, uint32_t nsyms, uint32_t *code, uint32_t *num)
{
    for (int i = 0; i < 34; ++i) num[i] = 0;
    if (n == 1) {
        num[1] = 1;
        A[0] = 1;
    } else {
        A[0] += A[1];
        int root = 0, leaf = 2;
        for (int next = 1; next < n - 1; ++next) {
            if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = (uint32_t)next; } else A[next] = A[leaf++];
            if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = (uint32_t)next; } else A[next] += A[leaf++];
        }
        A[n - 2] = 0;
        for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1u;
        int avbl = 1, used = 0, dpth = 0, next = n - 1;
        root = n - 2;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
            while (avbl > used) { A[next--] = (uint32_t)dpth; --avbl; }
            avbl = 2 * used; ++dpth; used = 0;
        }
        for (int i = 0; i < n; ++i) num[min(A[i], 33u)]++;
        for (uint32_t i = limit + 1u; i < 34u; ++i) { num[limit] += num[i]; num[i] = 0; }
        uint32_t total = 0;
        for (uint32_t i = limit; i > 0u; --i) total += num[i] << (limit - i);
        while (total > (1u << limit)) {
            num[limit]--;
            for (uint32_t i = limit - 1u; i > 0u; --i)
                if (num[i]) { num[i]--; num[i + 1u] += 2u; break; }
            total--;
        }
    }
    int j = n;
    for (uint32_t len = 1; len <= limit; ++len)
        for (uint32_t k = num[len]; k > 0u; --k) code[sym[--j]] = len << 16;
    // canonical codes (RFC 1951 3.2.2)
    uint32_t *next_code = num + 40, c = 0;
    num[0] = 0;
    for (uint32_t len = 1; len <= limit; ++len) { c = (c + num[len - 1u]) << 1; next_code[len] = c; }
    for (uint32_t s = 0; s < nsyms; ++s) {
        const uint32_t len = code[s] >> 16;
        if (len) { const uint32_t v = next_code[len]++; code[s] = (len << 16) | (__brev(v) >> (32u - len)); }
    }
}

} // namespace fl
