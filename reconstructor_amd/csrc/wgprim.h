// wgprim.h -- integer scan and rank over one workgroup, shared by every unit that compacts or offsets a list.  gfx950, wave64.
//
// Integer sums only: exact in any order, so every caller gets the same bits whatever the shape of the scan.  Each
// function is called by ALL threads of a one-dimensional workgroup (it holds barriers) and ends with a barrier, so
// that `sh` can be reused at once.  tools/wgprim_check.hip checks each one against a host loop.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

// Inclusive scan of one value per thread over a workgroup of NT threads (256 or 1024); total = the workgroup's sum.
// Shuffles inside the wave, wave totals through sh[NT / 64].
template <typename T, int NT>
__device__ __forceinline__ T wg_scan_incl(T v, T *sh, T &total)
{
    static_assert(NT == 256 || NT == 1024, "4 or 16 waves");
    constexpr int NW = NT / 64;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int o = 1; o < 64; o <<= 1) { const T u = __shfl_up(v, o); if (lane >= o) v += u; }
    if (lane == 63) sh[w] = v;
    __syncthreads();
    if (t < NW) { T s = sh[t]; for (int o = 1; o < NW; o <<= 1) { const T u = __shfl_up(s, o, NW); if (t >= o) s += u; } sh[t] = s; }
    __syncthreads();
    const T base = w ? sh[w - 1] : 0;
    total = sh[NW - 1];
    __syncthreads();
    return v + base;
}

// Number of flagged threads with a lower thread index; total = the workgroup's count.  sh[NT / 64].
template <int NT>
__device__ __forceinline__ int wg_rank(bool flag, int *sh, int &total)
{
    static_assert(NT == 256 || NT == 1024, "4 or 16 waves");
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) sh[w] = (int)__popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
    for (int i = 0; i < NT / 64; ++i) { const int c = sh[i]; base += i < w ? c : 0; total += c; }
    __syncthreads();
    return base + (int)__popcll(m & ((1ull << lane) - 1ull));
}

// off[i] = base + sum(cnt[0 .. i)) for i < n, by the 1024 threads of one workgroup; returns base + sum(cnt[0 .. n)) to
// every thread.  Thread t owns the contiguous run of ceil(n / 1024) elements; off may be cnt itself.
template <typename TI, typename TO>
__device__ __forceinline__ TO wg_scan_array(const TI *cnt, long n, TO *off, TO base)
{
    __shared__ TO sh[16];
    const long per = (n + 1023) / 1024, lo = min(n, (long)threadIdx.x * per), hi = min(n, lo + per);
    TO s = 0;
    for (long i = lo; i < hi; ++i) s += cnt[i];
    TO total;
    TO run = base + wg_scan_incl<TO, 1024>(s, sh, total) - s;
    for (long i = lo; i < hi; ++i) { const TO c = cnt[i]; off[i] = run; run += c; }
    return base + total;
}

}  // namespace
