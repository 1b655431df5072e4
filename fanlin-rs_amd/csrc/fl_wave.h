// fl_wave.h -- wave (64 lanes) and workgroup reductions shared by the device encoders (fl_png.hip, fl_webpll.hip).
// (fl_jpeg.hip scans with DPP row shifts instead and says why.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fl {

// v combined over the wave with op (associative, commutative); every lane gets the result
template <typename T, class Op> __device__ __forceinline__ T wave_reduce(T v, Op op)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, (T)__shfl_xor(v, o, 64));
    return v;
}
// the sum over each group of N adjacent lanes (N a power of two, the groups aligned to N); every lane of a group gets it
template <int N> __device__ __forceinline__ uint32_t group_sum(uint32_t v)
{
#pragma unroll
    for (int o = N / 2; o > 0; o >>= 1) v += (uint32_t)__shfl_xor(v, o, 64);
    return v;
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
__device__ __forceinline__ uint32_t wave_xor(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return a ^ b; }); }
__device__ __forceinline__ uint32_t wave_max(uint32_t v) { return wave_reduce(v, [](uint32_t a, uint32_t b) { return max(a, b); }); }

// exclusive scan (sum) over a workgroup of THREADS; s_w = THREADS / 64 words of LDS; *total = the sum of all
template <uint32_t THREADS> __device__ __forceinline__ uint32_t wg_scan(uint32_t v, uint32_t *s_w, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc += t;
    }
    __syncthreads();
    if (lane == 63u) s_w[wave] = inc;
    __syncthreads();
    uint32_t base = 0, sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < THREADS / 64u; ++i) { const uint32_t t = s_w[i]; if (i < wave) base += t; sum += t; }
    *total = sum;
    return base + inc - v;
}

// The job a flat index x of a launch belongs to: the last of jobs[0 .. njobs) whose `first` (the job's first index,
// ascending over the jobs) is <= x.
template <class J> __device__ __forceinline__ uint32_t find_first_le(const J *__restrict__ jobs, uint32_t njobs, uint32_t x, uint32_t J::*first)
{
    uint32_t lo = 0, hi = njobs - 1u;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (jobs[mid].*first <= x) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

} // namespace fl
